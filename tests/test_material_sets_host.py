"""Materials set on a batch of primitives, no GPU: GPUKernel::setPrimitiveMaterials (SolRx_SetPrimitiveMaterials,
Kernel.set_primitive_materials) - per record setPrimitiveMaterial, in order, then compactBoxes(false) - what the reference's
SwcScene::doAnimate does per frame to mark a sample of its morphology.

Held to: the setter that was there before, called one record at a time and followed by compactBoxes(false)
(material_set_cases.by_setter); and the rules of the journal - the "host-replay" engine claims every batch the store's side of
the engine's conditions allows (GPUKernel::materialSlots) for a device it does not have: its lazy replay against the eager
host route, what a look at a primitive's material answers meanwhile, and what a batch of edits or a morph behind a pending
material set is told.  The real engine's kernel is held to the same host route in tests/test_material_sets_gpu.py."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_cases  # noqa: E402
import material_set_cases as cases  # noqa: E402
import move_cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWC = os.path.join(ROOT, "tests", "golden", "pyramidal.swc")
ENGINE = ("solr_hip_set_primitive_materials", "solr_hip_device_material_sets")
f32 = np.float32


def _same(a, b):
    """field by field: the structs carry padding that no one initialises"""
    return len(a) == len(b) and all(
        np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8))
        for f in a.dtype.names)


def _differing(a, b):
    return [f for f in a.dtype.names
            if not np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8))]


def _assert_same_scene(a, b, what=""):
    assert _same(a.primitives, b.primitives), (what, _differing(a.primitives, b.primitives))
    assert _same(a.boxes, b.boxes), (what, _differing(a.boxes, b.boxes))
    assert _same(a.lights, b.lights), (what, _differing(a.lights, b.lights))
    assert a.nb_lamps == b.nb_lamps


def _kernel(solr, name, engine="host-only"):
    return cases.build(solr.Kernel(engine=engine, deterministic_seed=1), name)


def _frame(k):
    """one frame of the frame protocol; without a device it renders nothing and says so"""
    k.L.SolRx_Render(0.0)


def _batches(flat, extra):
    """a batch of 1, a leaf's first primitive with one that is not, a lamp among others, every primitive behind the lamps"""
    p = flat.primitives
    last = int(p["index"][-1])
    first, other = cases.leaf_first_and_other(flat, strict=False)
    lamp = int(p["index"][0])
    return [([last], [extra["plain"]]),
            ([first, other], [extra["clear"], cases.other_wall(flat, other)]),
            ([other, lamp, first], [extra["procedural"], cases.other_wall(flat, lamp), cases.emissive(flat)]),
            cases.recolour_all(flat)]


@pytest.mark.parametrize("name", cases.NAMES)
def test_a_batch_equals_the_setter_record_by_record(solr, name):
    """primitives, boxes and lights, field by field, after each of the batches; the materials are the batch's"""
    k = _kernel(solr, name)
    try:
        start = k.flat_scene()
        batches = _batches(start, k.extra)
        mine = []
        for indices, materials in batches:
            assert k.set_primitive_materials(indices, materials) == 0
            assert k.pending_moves() == 0
            mine.append(k.flat_scene())
    finally:
        k.finalize()
    h = _kernel(solr, name)
    try:
        for n, batch in enumerate(batches):
            cases.by_setter(h, ("materials", batch), None)
            theirs = h.flat_scene()
            _assert_same_scene(mine[n], theirs, "batch %d of %s" % (n, name))
            for index, material in zip(*batch):
                assert theirs.primitives["materialId"][theirs.primitives["index"] == index][0] == material
    finally:
        h.finalize()
    # the boxes follow no material, and a lamp's light record does: made again from the lamp when the frame is flattened
    assert _same(mine[-1].boxes, start.boxes)
    assert mine[2].lights["materialId"][0] == batches[2][1][1] != start.lights["materialId"][0]


@pytest.mark.parametrize("engine", ["host-only", "host-replay"])
def test_an_unknown_index_refuses_the_batch(solr, engine):
    k = _kernel(solr, "mix", engine)
    try:
        _frame(k)
        before = k.flat_scene()
        known = [int(i) for i in before.primitives["index"][3:6]]
        for bad in (len(before.primitives), -1, 1 << 20):
            assert k.set_primitive_materials(known + [bad], [k.extra["plain"]] * 4) == -1
            assert k.set_primitive_materials([bad] + known, [k.extra["plain"]] * 4) == -1
        assert k.pending_moves() == 0
        _assert_same_scene(before, k.flat_scene(), "a refused batch")
        assert k.set_primitive_materials([], []) == 0 and k.pending_moves() == 0
        with pytest.raises(solr.SolrError):
            k.set_primitive_materials(known, [1])
        # the fast path is still open behind a refusal
        assert k.set_primitive_materials(known, [k.extra["plain"]] * 3) == 0
        assert k.pending_moves() == (1 if engine == "host-replay" else 0)
    finally:
        k.finalize()


@pytest.mark.parametrize("engine", ["host-only", "host-replay"])
def test_the_last_record_for_an_index_wins(solr, engine):
    k = _kernel(solr, "sticks", engine)
    try:
        _frame(k)
        p = k.flat_scene().primitives
        a, b = int(p["index"][5]), int(p["index"][9])
        assert k.set_primitive_materials([a, b, a, a], [k.extra["plain"], k.extra["clear"], k.extra["procedural"], 4]) == 0
        assert k.pending_moves() == (1 if engine == "host-replay" else 0)
        assert k.get_primitive_material(a) == 4 and k.get_primitive_material(b) == k.extra["clear"]
        after = k.flat_scene().primitives
        assert after["materialId"][after["index"] == a][0] == 4 and after["materialId"][after["index"] == b][0] == k.extra["clear"]
    finally:
        k.finalize()


def _lazy_and_eager(solr, name, make_steps):
    """the steps on the double, a frame first and after each, every step claimed; the same on the host-only engine through
    the setters that were there before; the flattened scenes of both at the end"""
    k = _kernel(solr, name, engine="host-replay")
    try:
        lamps = move_cases.lamp_indices(k)
        steps = make_steps(k.flat_scene(), k.extra)
        _frame(k)
        for n, step in enumerate(steps):
            cases.apply(k, step, lamps)
            assert k.pending_moves() == n + 1, "step %d, %s, took the host route" % (n, step[0])
            assert k.compact_boxes(False) > 0        # returns as with rotations pending: nothing to flatten here
            assert k.pending_moves() == n + 1
            _frame(k)
        lazy = k.flat_scene()
        assert k.pending_moves() == 0
    finally:
        k.finalize()
    h = _kernel(solr, name)
    try:
        for step in steps:
            cases.by_setter(h, step, lamps)
            assert h.pending_moves() == 0
        eager = h.flat_scene()
    finally:
        h.finalize()
    return lazy, eager, steps


def test_lazy_replay_of_material_sets_among_the_other_moves_equals_the_eager_host_route(solr):
    """material sets, rotations, a translation, a lamp move and batches of edits - the second naming the materials the sets
    before it left - in one journal: pending_moves counts every one, and the replay leaves what the eager route leaves"""
    lazy, eager, steps = _lazy_and_eager(solr, "sticks", cases.mixed_steps)
    assert sum(1 for s in steps if s[0] == "materials") == 3
    _assert_same_scene(lazy, eager, "the mixed journal")


def test_more_than_eight_rotations_with_a_material_set_are_replayed(solr):
    """past eight rotations a store fetches the primitives from its engine, which hands back no material (and the double
    nothing at all): a journal that holds a material set is replayed"""
    def steps(flat, extra):
        sphere = cases.first_of_type(flat, solr.ptSphere, 1)
        out = [("rotate", edit_cases.TURNS[n % 3]) for n in range(10)]
        out.insert(4, ("materials", ([sphere], [extra["clear"]])))
        return out
    lazy, eager, _ = _lazy_and_eager(solr, "mix", steps)
    _assert_same_scene(lazy, eager, "ten rotations and a material set")


def test_a_look_at_the_material_sees_what_is_pending(solr):
    k = _kernel(solr, "mix", engine="host-replay")
    try:
        _frame(k)
        p = k.flat_scene().primitives
        a, b = int(p["index"][4]), int(p["index"][7])
        was = k.get_primitive_material(b)
        assert k.set_primitive_materials([a], [k.extra["plain"]]) == 0
        assert k.pending_moves() == 1
        assert k.get_primitive_material(a) == k.extra["plain"]
        assert k.pending_moves() == 1, "the look woke the store"
        assert k.set_primitive_materials([a, b], [k.extra["clear"], k.extra["plain"]]) == 0
        assert k.get_primitive_material(a) == k.extra["clear"] and k.pending_moves() == 2
        assert k.get_primitive_material(1 << 20) == -1
        k.sync_host()
        assert k.pending_moves() == 0
        assert k.get_primitive_material(a) == k.extra["clear"] and k.get_primitive_material(b) == k.extra["plain"] != was
        # the setter that was there before, behind a pending set: replayed first, then applied
        assert k.set_primitive_materials([a], [k.extra["plain"]]) == 0 and k.pending_moves() == 1
        k.L.SolR_SetPrimitiveMaterial(a, was)
        assert k.pending_moves() == 0 and k.get_primitive_material(a) == was
    finally:
        k.finalize()


def test_edits_behind_a_material_set_name_the_material_the_primitive_has_now(solr):
    """GPUKernel::editSlots declines another material than the primitive's: behind a pending material set that is the new
    one"""
    k = _kernel(solr, "sticks", engine="host-replay")
    try:
        _frame(k)
        flat = k.flat_scene()
        slot = flat.nb_lamps + 3
        index, old = int(flat.primitives["index"][slot]), int(flat.primitives["materialId"][slot])
        new = (old + 1) % 6
        assert k.set_primitive_materials([index], [new]) == 0 and k.pending_moves() == 1
        record = edit_cases.record(flat.primitives[slot], seed=5)
        assert record["materialId"] == old
        renamed = record.copy()
        renamed["materialId"] = new
        assert k.set_primitives(edit_cases.records([renamed])) == 0
        assert k.pending_moves() == 2, "an edit that names the new material took the host route"
        assert k.set_primitives(edit_cases.records([record])) == 0
        assert k.pending_moves() == 0, "an edit that names the old material was served over there"
        after = k.flat_scene().primitives
        assert after["materialId"][slot] == old and np.array_equal(after["p0"][slot], record["p0"])
    finally:
        k.finalize()


def test_a_morph_behind_a_material_set_takes_the_host_route(solr):
    """the blend on the device keeps the materials it finds, where morphPrimitives' loop takes the first key's: behind a
    material set over there the host serves the morph.  A material set behind a pending morph is fine: the morph is
    replayed first"""
    def run(k, claimed):
        p = k.flat_scene().primitives
        indices = [int(p["index"][5]), int(p["index"][8])]
        _frame(k)
        assert k.morph_frame(0.25) == 0 and k.pending_morph() == claimed
        assert k.set_primitive_materials(indices, [k.extra["plain"]] * 2) == 0
        assert k.pending_moves() == (1 if claimed else 0) and k.pending_morph() == claimed
        behind_a_morph = k.flat_scene()
        assert k.pending_moves() == 0 and not k.pending_morph()
        assert k.set_primitive_materials(indices[:1], [k.extra["clear"]]) == 0
        assert k.pending_moves() == (1 if claimed else 0)
        assert k.morph_frame(0.75) == 0
        assert not k.pending_morph() and k.pending_moves() == 0, "the morph was served behind a material set"
        after = k.flat_scene()
        _frame(k)                                                  # uploaded again: morphs are served again
        assert k.morph_frame(0.25) == 0 and k.pending_morph() == claimed
        return behind_a_morph, after

    k = _kernel(solr, "mix", engine="host-replay")
    try:
        lazy = run(k, True)
    finally:
        k.finalize()
    h = _kernel(solr, "mix")
    try:
        eager = run(h, False)
    finally:
        h.finalize()
    _assert_same_scene(lazy[0], eager[0], "a material set behind a morph")
    _assert_same_scene(lazy[1], eager[1], "a morph behind a material set")


def test_a_lamp_or_a_material_nobody_added_is_not_claimed(solr):
    """the store's side of the engine's conditions (GPUKernel::materialSlots): a lamp's light record carries its material, a
    material beyond the active ones was never uploaded; the host route serves both"""
    k = _kernel(solr, "sticks", engine="host-replay")
    try:
        _frame(k)
        flat = k.flat_scene()
        lamp, other = int(flat.primitives["index"][0]), int(flat.primitives["index"][6])
        assert flat.nb_lamps == 1 and move_cases.lamp_indices(k) == [lamp]
        assert k.set_primitive_materials([other, lamp], [2, 2]) == 0 and k.pending_moves() == 0
        assert k.get_primitive_material(lamp) == 2
        _frame(k)
        assert k.set_primitive_materials([other], [k.extra["plain"] + 1]) == 0 and k.pending_moves() == 0
        _frame(k)
        assert k.set_primitive_materials([other], [k.extra["plain"]]) == 0 and k.pending_moves() == 1
    finally:
        k.finalize()


def _walk_by_the_old_calls(k, samples, lamp, light_material, steps):
    """SwcScene::doAnimate restated with the setters that were there before"""
    by_id = {int(s["id"]): s for s in samples}
    marked = None
    for step in range(steps):
        s = by_id.get(step % len(samples))
        primitive = int(s["primitiveId"]) if s is not None else 0
        x, y, z = ((f32(s["x"]), f32(s["y"]), f32(s["z"])) if s is not None else (f32(0), f32(0), f32(0)))
        if marked is not None:
            k.L.SolR_SetPrimitiveMaterial(*marked)
        marked = (primitive, k.L.SolR_GetPrimitiveMaterial(primitive))
        k.L.SolR_SetPrimitiveMaterial(primitive, light_material)
        k.set_primitive_center(lamp, (float(x), float(y), float(f32(z - f32(50.0)))))
    return k.flat_scene()


def swc_scene(solr, engine):
    k = solr.Kernel(engine=engine, deterministic_seed=1)
    n = solr.scenes.swc_morphology(k, SWC, width=64, height=48, iterations=2)
    return k, n


@pytest.mark.parametrize("engine", ["host-only", "host-replay"])
def test_the_walk_along_a_morphology(solr, engine):
    """Kernel.swc_samples hands over what the reader kept; scenes.swc_walk marks one sample a frame and drags the lamp along,
    eight frames of it, and leaves what SwcScene::doAnimate's own calls leave"""
    k, n = swc_scene(solr, engine)
    try:
        samples = k.swc_samples()
        assert samples.dtype == solr.SWC_SAMPLE_DTYPE and len(samples) == n > 1000
        assert np.array_equal(samples["id"], np.sort(samples["id"])) and (samples["parent"][samples["id"] == 1] == -1).all()
        nb = len(k.flat_scene().primitives)
        assert (samples["primitiveId"] >= 0).all() and (samples["primitiveId"] < nb).all()
        # the file's second sample, scaled by 40 as the scene loads it: " 2 1 2.14 14.34 -0.15 12.61 1"
        two = samples[samples["id"] == 2][0]
        assert (two["x"], two["y"], two["z"], two["radius"]) == (f32(40.0 * 2.14), f32(40.0 * 14.34), f32(40.0 * -0.15), f32(40.0 * 12.61))
        lamp = move_cases.lamp_indices(k)[0]
        light = k.get_primitive_material(lamp)
        _frame(k)
        state, marked = {}, []
        for step in range(8):
            marked.append(solr.scenes.swc_walk(k, samples, lamp, light, step, state))
            if engine == "host-replay":
                assert k.pending_moves() == 2 * (step + 1), "step %d took the host route" % step
            assert k.get_primitive_material(marked[-1]) == light
            _frame(k)
        assert len(set(marked)) > 2
        mine = k.flat_scene()
        assert (mine.primitives["materialId"] == light).sum() == 2          # the lamp and the sample marked last
    finally:
        k.finalize()
    h, _ = swc_scene(solr, "host-only")
    try:
        theirs = _walk_by_the_old_calls(h, h.swc_samples(), lamp, light, 8)
    finally:
        h.finalize()
    _assert_same_scene(mine, theirs, "eight frames of the walk")


def _declared(path):
    text = open(os.path.join(ROOT, path)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"^\s*(?:[A-Za-z_][\w \*]*?)\b(\w+)\s*\([^;{]*\)\s*;", text, flags=re.M))


def test_the_entry_points_are_declared_exported_and_taken_up(solr):
    assert set(ENGINE) <= _declared("include/solr_hip.h")
    assert {"SolRx_SetPrimitiveMaterials", "SolRx_GetMorphologies"} <= _declared("sol-r_amd/host/SolRStub.h")
    hip, host = solr.hip_lib(), solr.host_lib()
    for name in ENGINE:
        assert hasattr(hip, name), name
    assert hasattr(host, "SolRx_SetPrimitiveMaterials") and hasattr(host, "SolRx_GetMorphologies")
    # csrc/exports.map names what libsolr_hip.so exports, by pattern (tests/test_abi_track.py)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "sol-r_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", text, flags=re.S).group(1).split(";") if p.strip()]
    for name in ENGINE:
        assert any(re.fullmatch(p.replace("*", ".*"), name) for p in patterns), name
    for method in ("set_primitive_materials", "get_primitive_material", "swc_samples"):
        assert callable(getattr(solr.Kernel, method))
    assert callable(solr.scenes.swc_walk) and solr.SWC_SAMPLE_DTYPE.itemsize == 32


def test_the_model_of_the_tags_knows_the_cases(solr):
    """the numpy model the GPU tests hold the kernel to (material_set_cases): the kinds of the mix as its materials make
    them, and the three changes of kind the engine has to decline"""
    k = _kernel(solr, "mix")
    try:
        flat = k.flat_scene()
        p, m = flat.primitives, flat.materials
        kinds = [cases.kind_model(t, cases.facts_model(m[i])) for t, i in zip(p["type"], p["materialId"])]
        assert {cases.KIND_SPHERE, cases.KIND_TRIANGLE, cases.KIND_CYLINDER, cases.KIND_PLANE_XY, cases.KIND_PLANE_YZ,
                cases.KIND_GENERAL} <= set(kinds)
        yz = cases.first_of_type(flat, solr.ptYZPlane)
        sphere = cases.first_of_type(flat, solr.ptSphere)
        xy = cases.first_of_type(flat, solr.ptXYPlane)
        textured = int(np.flatnonzero(m["textureIds"][:, 0] >= 0)[0])
        assert cases.kind_changes(flat, yz, cases.emissive(flat)) and not cases.kind_changes(flat, xy, cases.emissive(flat))
        assert cases.kind_changes(flat, sphere, k.extra["procedural"]) and not cases.kind_changes(flat, sphere, k.extra["clear"])
        assert cases.kind_changes(flat, xy, textured) and not cases.kind_changes(flat, xy, k.extra["plain"])
        assert cases.key_model(m[k.extra["plain"]]) == f32(f32(f32(f32(0.15) + f32(0.8)) + f32(0.35)) / f32(3))
    finally:
        k.finalize()
