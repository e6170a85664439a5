"""The synthetic post-processing cases of tests/post_processing_cases.py, as far as a CPU can hold them.

* The oracle against the text model (tests/cuda_text_model.py, the independent Python reading of the CUDA text) on the
  tiny frames - 1 x 1, 5 x 3, 13 x 7 - for all five effects and every kind of random buffer, in a refinement pass (1: the
  buffers are what was built) and an accumulation pass (12: the divisions by pathTracingIteration - 9, over a scene that
  is all background).  Whole frames: the text model has no strips.  The `nonfinite` randoms go to ambient occlusion and
  depth of field in pass 1, where only the conversion to int sees them (in pass 12 the camera jitters with them).
* The inputs are not vacuous: for every ambient-occlusion case, moving ONE tap by a pixel changes at least 10 % of the
  oracle's image and at least 40 % of its pixels are darkened - or the case says which of the two it is let off, and
  is held to what it can show instead (post_processing_cases.AO_CASES).
* Every path of k_ambientOcclusion is reached by the case table, by ao_paths' restatement of the kernel's predicates.

Every path can be reached through the C ABI at a small size, but not on the 136 x 40 frames of most cases: no frame
136 wide or 40 high holds a steady tile (post_processing_cases.AO_CASES, the comment above its last five cases), so
frames of 200 x 56 to 224 x 200 were added for the two steady paths."""
import importlib

import numpy as np
import pytest

import cuda_text_model as M
import post_processing_cases as PC

solr = importlib.import_module("sol-r_amd")
TINY = ((1, 1), (5, 3), (13, 7))


class Prepared:
    """the flattened scene and the frame parameters of a W x H stage, kept after its kernel is gone (the host mirror
    is one engine per process)"""

    def __init__(self, W, H, background):
        k = PC.stage(solr, W, H, background=background)
        try:
            self.flat = k.flat_scene()
            self.base = np.array(self.flat.randoms, copy=True)
            self.frame = k.frame_parameters()
            self.view_distance = self.frame[0].viewDistance
        finally:
            k.finalize()

    def parameters(self, c):
        si, ppi = self.frame[0], self.frame[1]
        si.pathTracingIteration = c["iteration"]
        si.viewDistance = c.get("view_distance") or self.view_distance
        ppi.type, ppi.param1, ppi.param2, ppi.param3 = c["effect"], c["param1"], c["param2"], c["param3"]
        return self.frame


_prepared = {}


def prepared(W, H, background=False):
    key = (W, H, background)
    if key not in _prepared:
        _prepared[key] = Prepared(W, H, background)
    return _prepared[key]


def both(oracle, c):
    """case c through the oracle and through the text model -> what differs (empty: the same bits)"""
    p = prepared(c["W"], c["H"], background=c["iteration"] > M.NB_MAX_ITERATIONS)
    params = p.parameters(c)
    pp, ids = PC.case_frame(c)
    rnd = PC.randoms(p.base, c["randoms"])
    opp, oids, orgb = PC.expected(oracle, p.flat, params, c, pp, ids, rnd)
    with np.errstate(all="ignore"):
        mpp, mids, mrgb = M.render(params[0], params[1], p.flat, params[2], params[3], params[4], pp=pp, ids=ids,
                                   randoms=rnd)
    if c["iteration"] <= M.NB_MAX_ITERATIONS:
        assert np.array_equal(opp.view(np.uint32), pp.view(np.uint32)) and np.array_equal(oids, ids), \
            "a refinement pass over these buffers must leave them alone"
    differs = []
    if not np.array_equal(opp.view(np.uint32)[..., :7], mpp.view(np.uint32)[..., :7]):
        differs.append("frame buffer")
    if not np.array_equal(oids, mids):
        differs.append("ids")
    if not np.array_equal(orgb, mrgb):
        y, x = np.argwhere((orgb != mrgb).any(axis=-1))[0]
        differs.append("bitmap at (%d, %d): oracle %s, model %s" % (x, y, orgb[y, x].tolist(), mrgb[y, x].tolist()))
    return differs


def tiny_cases(effect):
    """the members of the tables on 1 x 1 and 5 x 3, the same parameters on 13 x 7, every finite kind of random buffer,
    the non-finite one where only the conversion to int sees it; and pass 12 for all of it but the non-finite"""
    cases = []
    if effect == PC.ppe_ambientOcclusion:
        for W, H in TINY:
            kinds = [(kind, 10.0) for kind in PC.RANDOMS_KINDS] + [("default", 2000.0), ("half", -10.0)]
            cases += [PC._ao(W, H, kind, p2, seed=3) for kind, p2 in kinds]
            cases += [PC._ao(W, H, "half", 10.0, depths="special", seed=3)]
    else:
        table = [c for c in PC.OTHER_CASES if c["effect"] == effect and not c["strip"] and c["W"] * c["H"] <= 15]
        cases += table
        # 13 x 7: the table's parameters again, but for the 300 taps of depth of field (the model is a Python loop)
        cases += [dict(c, W=13, H=7) for c in table if (c["W"], c["H"]) == (5, 3) and c["param3"] < 300]
        if effect == PC.ppe_depthOfField:
            cases += [PC._other(effect, W, H, None, "nonfinite", 0.0, 20.0, 16) for W, H in TINY]
    finite = [c for c in cases if c["randoms"] != "nonfinite" and c["depths"] == "levels"]
    # the accumulation pass renders: one case per frame, kind of random buffer and effect (radiosity's passes are 1 and 7)
    seen = set()
    for c in finite:
        key = (c["W"], c["H"], c["randoms"])
        if key not in seen and c["param3"] < 300:
            seen.add(key)
            cases.append(dict(c, iteration=12))
    return cases


@pytest.mark.parametrize("effect", sorted(PC.EFFECT_NAMES), ids=lambda e: PC.EFFECT_NAMES[e].replace(" ", "_"))
def test_the_oracle_equals_the_text_model_on_synthetic_frames(oracle, effect):
    cases = tiny_cases(effect)
    assert {c["iteration"] for c in cases} >= {1, 12} and {(c["W"], c["H"]) for c in cases} == set(TINY)
    failed = {PC.case_id(c): d for c in cases for d in [both(oracle, c)] if d}
    assert not failed, "%d of %d cases differ: %s" % (len(failed), len(cases), list(failed.items())[:4])


def test_the_builders_keep_their_contract():
    p = prepared(5, 3)
    assert len(p.base) >= PC.MAX_BITMAP_SIZE
    pp, ids = PC.frame(33, 9, 1, "special")
    assert pp.shape == (9, 33, 8) and pp.dtype == np.float32 and ids.shape == (9, 33, 4) and ids.dtype == np.int32
    assert not ids[..., 1].any() and not ids[..., 3].any()
    assert np.isfinite(pp[..., :3]).all() and not np.isfinite(pp[..., 3]).all()
    assert ids[..., 2].min() < 0 and ids[..., 2].max() > 256
    again = PC.frame(33, 9, 1, "special")
    assert np.array_equal(pp.view(np.uint32), again[0].view(np.uint32)) and np.array_equal(ids, again[1])
    levels = PC.frame(136, 40, 1, "levels", white=True)[0]
    assert set(np.unique(levels[..., 3].view(np.uint32))) == set(PC.LEVELS.view(np.uint32)) and (levels[..., :3] == 1).all()
    for kind in PC.RANDOMS_KINDS:
        r = PC.randoms(p.base, kind)
        assert r.shape == p.base.shape and r.dtype == np.float32
        assert np.array_equal(r[PC.NB_REPLACED:], p.base[PC.NB_REPLACED:])
        assert np.isfinite(r).all() == (kind != "nonfinite")
    half = PC.randoms(p.base, "half")[:PC.NB_REPLACED]
    assert np.array_equal(half * 2, np.round(half * 2)) and np.abs(half).max() == 1.5 and (half < 0).any()
    assert PC.randoms(p.base, "positive")[:PC.NB_REPLACED].min() == 0
    wide = PC.randoms(p.base, "wide_x")
    assert (np.abs(wide[:256]) == 1.5).all() and not wide[256:356].any()
    assert np.abs(PC.randoms(p.base, "far")[:PC.NB_REPLACED]).max() == 3.0


@pytest.fixture(scope="module")
def ao_images(oracle):
    """per ambient-occlusion case: the random buffer, the oracle's image, and its image with one tap moved by a pixel"""
    out = {}
    for c in PC.AO_CASES:
        p = prepared(c["W"], c["H"])
        params = p.parameters(c)
        pp, ids = PC.case_frame(c)
        rnd = PC.randoms(p.base, c["randoms"])
        first, count = c["strip"] if c["strip"] else (0, c["H"])
        opp, oids, image = PC.expected(oracle, p.flat, params, c, pp, ids, rnd)
        assert np.array_equal(opp.view(np.uint32), pp[first:first + count].view(np.uint32)), PC.case_id(c)
        assert np.array_equal(oids, ids[first:first + count]), PC.case_id(c)
        _, _, moved = PC.expected(oracle, p.flat, params, c, pp, ids, PC.one_tap_moved(c, rnd))
        out[PC.case_id(c)] = (rnd, image, moved)
    return out


@pytest.mark.parametrize("c", PC.AO_CASES, ids=PC.case_id)
def test_the_ambient_occlusion_inputs_are_not_vacuous(ao_images, c):
    """One tap moved by a pixel changes at least 10 % of the oracle's image, and at least 40 % of its pixels are darkened
    (first byte below 255: occ < 1, where the byte follows the count).  What a case is let off, and what it is held to
    instead, is its `exempt` (post_processing_cases.AO_CASES): "white" - no pixel can be darkened, the image is 255
    throughout; "darkened" - only the 40 % is waived, where the expected darkened share is bounded below it; "faint" -
    the moved tap must show at all."""
    rnd, image, moved = ao_images[PC.case_id(c)]
    changed = float((image != moved).any(axis=-1).mean())
    darkened = float((image[..., 0] < 255).mean())
    print("%s: %.1f %% changed, %.1f %% darkened" % (PC.case_id(c), 100 * changed, 100 * darkened))
    exempt = c["exempt"] or ""
    assert exempt in ("", "white", "darkened", "darkened, faint")
    if exempt == "white":
        assert c["randoms"] == "zero" or c["W"] * c["H"] <= 15
        assert (image == 255).all() and (moved == 255).all()
        return
    if "darkened" in exempt:
        assert PC.ao_ceiling(c, rnd) < 0.40, "the case could meet the condition: it is not exempt"
    else:
        assert darkened >= 0.40, darkened
    if "faint" in exempt:
        assert changed > 0 and darkened > 0, (changed, darkened)
    else:
        assert changed >= 0.10, changed


def test_every_path_of_the_ambient_occlusion_kernel_is_reached(ao_images):
    pixels = np.zeros(len(PC.AO_PATHS), np.int64)
    pipelined, ordered, cls_spread, crowded = set(), set(), 0, 0
    for c in PC.AO_CASES:
        rnd = ao_images[PC.case_id(c)][0]
        first, count = c["strip"] if c["strip"] else (0, c["H"])
        above, below = PC.halo_of(c, rnd)
        res = PC.ao_paths(c["W"], c["H"], first, count, above, below, rnd, c["param2"])
        assert res["paths"].shape == (count, c["W"])
        pixels += np.bincount(res["paths"].ravel(), minlength=len(PC.AO_PATHS))
        pipelined.add(res["pipelined"])
        ordered.add(res["ordered"])
        cls_spread += res["cls_spread"]
        crowded += res["crowded"]
        # the fixed-stride variant the GPU test also runs is never ordered
        assert not PC.ao_paths(c["W"], c["H"], first, count, above, below, rnd, c["param2"], heavy_first=False)["ordered"]
    reached = dict(zip(PC.AO_PATHS, pixels.tolist()))
    print(reached)
    assert all(n >= 64 for n in reached.values()), reached
    assert pipelined == {True, False} and ordered == {True, False}
    assert cls_spread > 0, "no tile whose regular columns span more than two binades (a first tile column)"
    assert crowded > 0, "no tile with more than AO_IRREGULAR_TOGETHER irregular pixels"
    # the rows a strip asks its neighbours for: taps of 1.5 x 16 = 24 pixels, + 2
    half = next(c for c in PC.AO_CASES if c["randoms"] == "half" and c["strip"] and c["halo"] == "wanted")
    assert PC.halo_of(half, ao_images[PC.case_id(half)][0]) == (26, 26)
