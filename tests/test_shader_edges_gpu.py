"""THE ENGINE's primitiveShader and shadow sum against the oracle's CUDA dialect on the cases of tests/shader_edge_cases.py:
elements placed ON the decisions of GI:916-1080 and GI:866-908 (tests/test_shader_edge_cases.py holds the oracle to the text
model on the same elements, bit for bit, on the CPU).

Every case runs
  * in the three instantiation variants tests/test_engine_probes_gpu.py uses for these functions - the renderer's row on the
    engine's lists, the renderer's row on the reference's own list, the all-features row;
  * in three orders of the same elements - sorted by family (pure waves), interleaved by a fixed stride (every wave mixes lanes
    with and without a shadow ray, inside and outside the lean power domain, shading and not), ragged (37 elements beyond a
    multiple of 64) - because the shader is called by whole waves, its lamp loop is wave-uniform, the shadow walk inside it
    wave-synchronous and pow_f decides per wave;
  * a shader case through both probes: solr_hip_probe_shader (the shader gathers the hit's records itself) and
    solr_hip_probe_shader_given (they are handed over as launchRayTracing hands them - the path every Cornell frame takes; a
    lane that shades the room's primitive without a material sends its wave back to the shader's own gather: counted).
Every output of every element must be the oracle's bits - totalBlinn included: the power families hold only pairs whose power
is a binary32 number - and the same bits in every order.  Against the oracle "the same bits" is the project's bar
(oracle.probes.same_bits: +0 equals -0, a NaN equals a NaN); how many elements differ from it in the sign of a zero alone is
printed.  Across orders and probes the comparison is of the 32-bit words themselves, and so is the oracle's against the text
model on the CPU.  The rooms must run the lean sphere + plane row, which takes the
handed-over records; the mixed stage the all-features row, which does not.  Shadow rays must have been cast and have met their
occluders: a probe that skipped the walk would otherwise pass."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_probes as E  # noqa: E402
import shader_edge_cases as G  # noqa: E402
from test_shader_edge_cases import GROUP_NAMES, PINNED  # noqa: E402

VARIANTS = (("the renderer's instantiation, walk-order + order-free lists", 0, 0),
            ("the renderer's instantiation, the reference's own list", 0, 1),
            ("all-features instantiation", E.EVERYTHING, 0))
KEYS = {"shader": ("returned", "shadow", "normal", "closest_color", "total_blinn", "attributes"), "shadow": ("result", "color")}
ROW = {"room": E.F_SPHERE | E.F_PLANE, "room split": E.F_SPHERE | E.F_PLANE, "carriers": E.F_SPHERE | E.F_PLANE, "mixed": E.EVERYTHING}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(len(a), -1)


def shadows_were_met(case, out):
    """-> the families built for it of which no element of this case has a shadow above 0 (where the frame casts shadow rays at
    all: graphicsLevel above 3 for the shader, a limit above 0)"""
    si = case["si"]
    if si.shadowIntensity <= 0 or (case["name"] == "shader" and si.graphicsLevel <= 3):
        return []
    shadow = out["shadow" if case["name"] == "shader" else "result"]
    return [int(j) for j in np.unique(case["family"][case["occluded"]]) if not (shadow[case["occluded"] & (case["family"] == j)] > 0).any()]


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUP_NAMES)
def test_the_engine_gives_the_oracles_bits_on_every_element_in_every_variant_and_order(solr, oracle, group):
    import hashlib
    from oracle import probes
    L = oracle.lib()
    assert L.oracle_get_dialect() == 0 and L.oracle_get_rounded_transcendentals() == 0
    hip = solr.hip_lib()
    E.declare(hip)
    built = G.cases(solr, group)
    h = hashlib.sha1()
    for case, _, _ in built:
        h.update(G.digest(case).encode())
    assert (len(G.families(group)), len(built), sum(len(c["origins"]) for c, _, _ in built), h.hexdigest()) == PINNED[group]
    bad, runs, elements, handed, sent_back, zero_signs = [], 0, 0, 0, 0, 0
    for case, fams, stage in built:
        kind, n = case["name"], len(case["origins"])
        want = probes._oracle_outputs(L, case)
        assert not shadows_were_met(case, want), (case["key"], shadows_were_met(case, want))     # (by the oracle first)
        elements += n
        with E.Resident(solr, case["si"], stage.boxes, stage.prims, stage.materials, stage.textures, stage.lights, stage.nb_lamps,
                        stage.randoms):
            for label, features, exact in VARIANTS:
                for given in ((False, True) if kind == "shader" else (False,)):
                    for name, order in G.orders(n).items():
                        c = G.reordered(case, order)
                        got = E.shader_outputs(hip, c, features, exact, given) if kind == "shader" else E.walk_outputs(hip, c, features, exact)
                        runs += 1
                        what = "%s | %s | %s | %s%s" % (case["key"], label, name, kind, " (given)" if given else "")
                        # which row ran, and whether it takes the records
                        assert got["features"] & ~E.F_DEEP == (features if features else ROW[stage.name]) & ~E.F_DEEP, (what, got["features"])
                        if given:
                            assert got["hands_over"] == (got["features"] & ~E.F_DEEP == E.F_SPHERE | E.F_PLANE), what
                            handed += got["hands_over"]
                            if got["hands_over"]:
                                none = (stage.prims["materialId"][c["object_id"]] < 0)
                                waves = [none[w:w + 64] for w in range(0, len(none), 64)]
                                sent_back += sum(1 for w in waves if w.any() and not w.all())
                        assert not shadows_were_met(c, got), (what, shadows_were_met(c, got))
                        for key in KEYS[kind]:
                            same = probes.same_bits(got[key], want[key][order])
                            same = same.reshape(len(same), -1).all(axis=1)
                            zero_signs += int((_bits(got[key]) != _bits(want[key][order])).any(axis=1)[same].sum())
                            if not same.all():
                                first = int(np.flatnonzero(~same)[0])
                                bad.append((what, key, int((~same).sum()), fams[c["family"][first]].decision, got[key][first].tolist(),
                                            want[key][order][first].tolist()))
    print("%s: %d cases, %d elements, %d probe runs, %d of them with the records handed over, %d waves sent back to the shader's own gather "
          "by a lane without a material, %d outputs differ, %d element outputs equal but for the sign of a zero or the bits of a NaN" %
          (group, len(built), elements, runs, handed, sent_back, len(bad), zero_signs))
    assert not bad, bad[:12]
    assert handed > 0 and sent_back > 0


@pytest.mark.gpu
def test_the_three_orders_and_the_two_probes_return_identical_bits(solr):
    """per element of the dyadic group: sorted, interleaved and ragged waves, the plain probe and the one with the records handed
    over - one answer (exact bits, a NaN's included)"""
    hip = solr.hip_lib()
    E.declare(hip)
    compared = 0
    for case, fams, stage in G.cases(solr, "dyadic"):
        kind, n = case["name"], len(case["origins"])
        with E.Resident(solr, case["si"], stage.boxes, stage.prims, stage.materials, stage.textures, stage.lights, stage.nb_lamps,
                        stage.randoms):
            base = None
            for given in ((False, True) if kind == "shader" else (False,)):
                for name, order in G.orders(n).items():
                    c = G.reordered(case, order)
                    got = E.shader_outputs(hip, c, 0, 0, given) if kind == "shader" else E.walk_outputs(hip, c, 0, 0)
                    if base is None:
                        assert name == "sorted"
                        base = got
                        continue
                    for key in KEYS[kind]:
                        assert np.array_equal(_bits(got[key]), _bits(base[key])[order]), (case["key"], name, given, key)
                        compared += 1
    assert compared > 100
