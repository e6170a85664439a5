"""Materials set on the resident scene: GPUKernel::setPrimitiveMaterials (SolRx_SetPrimitiveMaterials,
Kernel.set_primitive_materials) with the HIP engine runs on the device (solr_hip_set_primitive_materials:
sol-r_amd/csrc/solr_materials.hip) - one thread per record sets the tag, the material id and the colour key of its primitive,
the leaf records follow, nothing is uploaded or refitted - and the host scene store follows lazily, through the one journal
of the moves.

The bar: a kernel that takes the device route is compared with a kernel that takes the host route - the setter that was
there before, one record at a time, compactBoxes(false), a fresh upload - after every step, BIT FOR BIT: the primitive
records, the nodes and the leaf records of every list the engine holds, the light records, the rendered frame.  The three
words of a served primitive are also held to the numpy model of the tags (tests/material_set_cases.py);
solr_hip_device_material_sets advances exactly when a batch was served; and what the engine cannot serve it declines without
changing anything."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_cases  # noqa: E402
import engine_probes  # noqa: E402
import material_set_cases as cases  # noqa: E402
import move_cases  # noqa: E402
from helpers import copy_frame, gpu_frame, same_frames  # noqa: E402

pytestmark = pytest.mark.gpu

SIZE = (64, 48)
SWC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pyramidal.swc")
EVERY_LIST = (engine_probes.WALK_LIST, engine_probes.EXACT_LIST, engine_probes.FREE_LISTS)
EXACT_ONLY = (engine_probes.EXACT_LIST,)      # behind a refit the other lists are refitted, not built anew: not comparable
SETTLE = 3      # frames after an upload until the order-free lists are built and in the arena


def _kernel(solr, name):
    return cases.build(solr.Kernel(engine="hip", deterministic_seed=1), name, size=SIZE)


def _same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _same_records(a, b):
    """field by field: the structs carry padding that no one initialises"""
    return len(a) == len(b) and all(_same_bits(a[f], b[f]) for f in a.dtype.names)


def _snapshot(k, hip, lists=EVERY_LIST):
    """what the device holds now: primitive rows, light rows, per list its nodes and its leaf records"""
    out = {"primitives": k.device_primitives().copy(), "lights": k.device_lights().copy()}
    for which in lists:
        out["nodes of list %d" % which] = engine_probes.list_copy(hip, which, engine_probes.NODE_ROWS)
        out["leaf records of list %d" % which] = engine_probes.list_copy(hip, which, engine_probes.LEAF_RECORDS)
    return out


def _assert_same_snapshot(a, b, what):
    assert a.keys() == b.keys()
    for part in a:
        assert _same_bits(a[part], b[part]), "%s: the %s differ" % (what, part)


def _settle(k):
    for _ in range(SETTLE - 1):
        gpu_frame(k)
    return copy_frame(gpu_frame(k))


def _touch(k, lamps):
    """the store accessed: every move takes the host route until the next upload"""
    k.L.SolR_SetPrimitiveMaterial(lamps[0], k.L.SolR_GetPrimitiveMaterial(lamps[0]))


def _device_route(solr, build, make_steps, lists=EVERY_LIST, flights=1):
    """the steps on the resident scene, a frame and a snapshot after each; every step has to be served over there"""
    hip = solr.hip_lib()
    k = build()
    try:
        hip.solr_hip_set_frames_in_flight(flights)
        lamps = move_cases.lamp_indices(k)
        flat = k.flat_scene()
        steps = make_steps(k, flat)
        _settle(k)
        has_free_lists = engine_probes.list_copy(hip, engine_probes.FREE_LISTS, engine_probes.NODE_ROWS) is not None
        served = hip.solr_hip_device_material_sets()
        after = []
        for n, step in enumerate(steps):
            if step[0] == "walk":
                step[1](k)
            else:
                cases.apply(k, step, lamps)
            assert k.pending_moves() == (2 if step[0] == "walk" else 1) * (n + 1), "step %d, %s, took the host route" % (n, step[0])
            served += step[0] in ("materials", "walk")
            assert hip.solr_hip_device_material_sets() == served, "step %d, %s" % (n, step[0])
            if step[0] == "materials" and len(set(step[1][0])) == len(step[1][0]):
                rows = k.device_primitives()
                for slot, tag, material, key in cases.three_words_model(flat, *step[1]):
                    got = rows[slot, :, 3].view(np.int32)
                    assert (got[0], got[1]) == (tag, material), "step %d, slot %d: tag %#x, material %d" % (n, slot, got[0], got[1])
                    assert got[3] == np.float32(key).view(np.int32), "step %d, slot %d: the colour key" % (n, slot)
            frame = copy_frame(gpu_frame(k))
            after.append((frame, _snapshot(k, hip, lists)))
        assert k.pending_moves() >= len(steps)         # reading the device does not wake the host store
        k.sync_host()
        assert k.pending_moves() == 0
        caught_up = k.flat_scene()
        k.check(0, "the sequence")
    finally:
        hip.solr_hip_set_frames_in_flight(1)
        k.finalize()
    return steps, after, caught_up, has_free_lists


def _host_route(solr, build, steps, lists=EVERY_LIST, flights=1):
    """the same steps by the calls that were there before, the store touched before each, a fresh upload behind each"""
    hip = solr.hip_lib()
    k = build()
    try:
        hip.solr_hip_set_frames_in_flight(flights)
        lamps = move_cases.lamp_indices(k)
        _settle(k)
        served = hip.solr_hip_device_material_sets()
        after = []
        for n, step in enumerate(steps):
            _touch(k, lamps)
            if step[0] == "walk":
                step[2](k)
            else:
                cases.by_setter(k, step, lamps)
            assert k.pending_moves() == 0, "step %d, %s, ran on the device" % (n, step[0])
            frame = _settle(k)
            after.append((frame, _snapshot(k, hip, lists)))
        assert hip.solr_hip_device_material_sets() == served
        flat = k.flat_scene()
        k.check(0, "the sequence by the host route")
    finally:
        hip.solr_hip_set_frames_in_flight(1)
        k.finalize()
    return after, flat


def _device_route_equals_host_route(solr, build, make_steps, lists=EVERY_LIST, flights=1):
    steps, mine, caught_up, has_free_lists = _device_route(solr, build, make_steps, lists, flights)
    theirs, flat = _host_route(solr, build, steps, lists, flights)
    for n, ((frame, snapshot), (their_frame, their_snapshot)) in enumerate(zip(mine, theirs)):
        _assert_same_snapshot(snapshot, their_snapshot, "after step %d, %s" % (n, steps[n][0]))
        assert same_frames(frame, their_frame), "after step %d, %s: the frames differ" % (n, steps[n][0])
    if len(steps) > 1:
        assert not same_frames(mine[0][0], mine[-1][0]), "the steps changed nothing in the picture"
    # the host store after its lazy replay == the host route
    assert _same_records(caught_up.primitives, flat.primitives)
    assert _same_records(caught_up.boxes, flat.boxes)
    assert _same_records(caught_up.lights, flat.lights)
    return has_free_lists


def _plain_to_plain(k, flat):
    """a sphere, a cylinder, a triangle and an axis plane of the mix, each to another plain material; then all four at
    once to the plain material nobody had"""
    # (walls 1, 3, 5 and 0 of morph_cases' mix: plain materials, as the ones they get)
    four = [cases.first_of_type(flat, t, material=m) for t, m in ((solr_types.ptSphere, 1), (solr_types.ptCylinder, 3),
                                                                   (solr_types.ptTriangle, 5), (solr_types.ptXYPlane, 0))]
    steps = [("materials", ([i], [cases.other_wall(flat, i)])) for i in four]
    return steps + [("materials", (four, [k.extra["plain"]] * 4))]


def _emissive_and_back(k, flat):
    sphere = cases.first_of_type(flat, solr_types.ptSphere, material=1)
    slot = int(cases.slots_of(flat, [sphere])[0])
    return [("materials", ([sphere], [cases.emissive(flat)])), ("materials", ([sphere], [int(flat.primitives["materialId"][slot])]))]


def _first_of_a_leaf_and_another(k, flat):
    first, other = cases.leaf_first_and_other(flat)
    starts = set(int(s) for s, n in zip(flat.boxes["startIndex"], flat.boxes["nbPrimitives"]) if n > 0)
    slots = cases.slots_of(flat, [first, other])
    assert int(slots[0]) in starts and int(slots[1]) not in starts
    return [("materials", ([other, first], [k.extra["plain"], k.extra["clear"]]))]


def _one_record(k, flat):
    return [("materials", ([cases.first_of_type(flat, solr_types.ptCylinder, 3)], [k.extra["plain"]]))]


def _more_than_a_block(k, flat):
    indices, materials = cases.recolour_all(flat)
    assert len(indices) == 289          # 256 + 33: a second block of k_setPrimitiveMaterials, not full
    return [("materials", (indices, materials))]


def _twice_in_a_batch(k, flat):
    a, b = cases.first_of_type(flat, solr_types.ptSphere, 1), cases.first_of_type(flat, solr_types.ptSphere, 4)
    return [("materials", ([a, b, a], [k.extra["clear"], k.extra["plain"], k.extra["plain"]]))]


solr_types = cases.solr
SERVED = {"plain_to_plain": ("mix", _plain_to_plain), "emissive_and_back": ("mix", _emissive_and_back),
          "first_of_a_leaf_and_another": ("sticks", _first_of_a_leaf_and_another), "one_record": ("sticks", _one_record),
          "more_than_a_block": ("mesh", _more_than_a_block), "twice_in_a_batch": ("sticks", _twice_in_a_batch)}


@pytest.mark.parametrize("case", sorted(SERVED))
def test_device_material_sets_equal_the_setter_and_a_fresh_upload(solr, case):
    name, make_steps = SERVED[case]
    has_free_lists = _device_route_equals_host_route(solr, lambda: _kernel(solr, name), make_steps)
    # (the sticks and the mix hold cones and ellipsoids, which keeps a scene from having order-free lists: the mesh has them)
    assert has_free_lists == (name == "mesh"), "the leaf records of the order-free lists were not compared where there are some"


def test_the_first_transparent_primitive_of_an_opaque_scene(solr):
    """by either route: the sticks are opaque to shadows, which a frame is told (SceneArgs::opaqueShadows); a sphere turned
    transparent takes that back.  The engine serves the batch with the fact updated in place - nothing that is derived at
    upload depends on it -, and the frames are those of the host route"""
    def steps(k, flat):
        assert not (flat.materials["transparency"][np.unique(flat.primitives["materialId"])] != 0).any()
        sphere = cases.first_of_type(flat, solr_types.ptSphere, 5)
        return [("materials", ([sphere], [k.extra["clear"]])), ("materials", ([sphere], [cases.other_wall(flat, sphere)]))]
    _device_route_equals_host_route(solr, lambda: _kernel(solr, "sticks"), steps)


@pytest.mark.parametrize("flights", [1, 3], ids=["one_frame", "three_in_flight"])
def test_a_material_set_a_rotation_and_an_edit_that_names_the_new_material(solr, flights):
    """one journal, in order: pending_moves() == 3 (the device route asserts it step by step), and sync_host leaves the eager
    store"""
    def steps(k, flat):
        slot = flat.nb_lamps + 3
        index = int(flat.primitives["index"][slot])
        new = cases.other_wall(flat, index)
        record = edit_cases.record(flat.primitives[slot], seed=5, to=edit_cases.stage("sticks", 1))
        record["materialId"] = new
        rod = next(r for r in (cases.first_of_type(flat, solr_types.ptCylinder, n) for n in (2, 3)) if r != index)
        return [("materials", ([index, rod], [new, k.extra["plain"]])),
                ("rotate", edit_cases.TURNS[1]), ("edit", edit_cases.records([record]))]
    _device_route_equals_host_route(solr, lambda: _kernel(solr, "sticks"), steps, lists=EXACT_ONLY, flights=flights)


def _swc_kernel(solr):
    k = solr.Kernel(engine="hip", deterministic_seed=1)
    solr.scenes.swc_morphology(k, SWC, width=SIZE[0], height=SIZE[1], iterations=2)
    return k


def test_eight_steps_of_the_walk_along_a_morphology(solr):
    """scenes.swc_walk, SwcScene::doAnimate restated: per frame two materials set and the lamp dragged, all on the device"""
    f32 = np.float32

    def steps(k, flat):
        samples = k.swc_samples()
        lamp = move_cases.lamp_indices(k)[0]
        light = k.get_primitive_material(lamp)
        by_id = {int(s["id"]): s for s in samples}
        state, old = {}, {"marked": None}

        def old_calls(step):
            """the frame through the calls that were there before"""
            def run(h):
                s = by_id.get(step % len(samples))
                primitive = int(s["primitiveId"]) if s is not None else 0
                x, y, z = ((f32(s["x"]), f32(s["y"]), f32(s["z"])) if s is not None else (f32(0), f32(0), f32(0)))
                if old["marked"] is not None:
                    h.L.SolR_SetPrimitiveMaterial(*old["marked"])
                old["marked"] = (primitive, h.L.SolR_GetPrimitiveMaterial(primitive))
                h.L.SolR_SetPrimitiveMaterial(primitive, light)
                h.set_primitive_center(lamp, (float(x), float(y), float(f32(z - f32(50.0)))))
            return run
        return [("walk", (lambda step: lambda k: solr.scenes.swc_walk(k, samples, lamp, light, step, state))(step), old_calls(step))
                for step in range(8)]
    assert _device_route_equals_host_route(solr, lambda: _swc_kernel(solr), steps), "the morphology has order-free lists"


DECLINED = ("lamp", "yz_plane_emissive", "sphere_procedural", "plane_textured", "not_uploaded", "touched", "other_frame")


@pytest.mark.parametrize("case", DECLINED)
def test_requests_the_engine_cannot_serve_change_nothing(solr, case):
    """a lamp's slot (its light record carries the material), a YZ plane turned emissive, a plain sphere turned procedural and
    a plane turned textured (the primitive's kind would change: the thin copies and the order-free hierarchy were made from
    the kinds), a material that was not uploaded, a touched store, a frame that is not the resident one: rows, lists and
    lights are what they were, the counter too, and the host route serves the request with the frame of the setter"""
    hip = solr.hip_lib()

    def prepare(kernel, lamps):
        if case == "touched":
            _touch(kernel, lamps)
        elif case == "other_frame":
            kernel.set_frame(0)

    k = _kernel(solr, "mix")
    try:
        lamps = move_cases.lamp_indices(k)
        flat = k.flat_scene()
        sphere = cases.first_of_type(flat, solr_types.ptSphere, material=1)
        batch = {"lamp": ([sphere, lamps[0]], [k.extra["plain"], cases.emissive(flat)]),
                 "yz_plane_emissive": ([cases.first_of_type(flat, solr_types.ptYZPlane), sphere], [cases.emissive(flat), k.extra["plain"]]),
                 "sphere_procedural": ([sphere], [k.extra["procedural"]]),
                 "plane_textured": ([cases.first_of_type(flat, solr_types.ptXYPlane)], [int(np.flatnonzero(flat.materials["textureIds"][:, 0] >= 0)[0])]),
                 "not_uploaded": ([sphere], [k.extra["plain"] + 1])}.get(case, ([sphere], [k.extra["plain"]]))
        if case in ("yz_plane_emissive", "sphere_procedural", "plane_textured"):
            assert any(cases.kind_changes(flat, i, m) for i, m in zip(*batch))
        _settle(k)
        before = _snapshot(k, hip)
        counter = hip.solr_hip_device_material_sets()

        def unchanged(what):
            _assert_same_snapshot(_snapshot(k, hip), before, what)
            assert hip.solr_hip_device_material_sets() == counter, what
            k.check(0, what + ": a refusal is not an error")

        slots, materials = cases.slots_of(flat, batch[0]), np.array(batch[1], np.int32)
        if case not in ("touched", "other_frame"):
            assert hip.solr_hip_set_primitive_materials(slots.ctypes.data, materials.ctypes.data, len(slots)) == 0
            unchanged("the engine's own answer")
        if case == "lamp":
            # (the engine's own boundary: the host side never sends these)
            for what, bad_slots, bad_materials in (("a slot twice", np.r_[slots[:1], slots[:1]], materials),
                                                   ("a slot out of range", np.array([slots[0], len(flat.primitives)], np.int32), materials),
                                                   ("slot -1", np.array([slots[0], -1], np.int32), materials),
                                                   ("a negative material", slots[:1], np.array([-1], np.int32))):
                bad_slots, bad_materials = np.ascontiguousarray(bad_slots, np.int32), np.ascontiguousarray(bad_materials, np.int32)
                assert hip.solr_hip_set_primitive_materials(bad_slots.ctypes.data, bad_materials.ctypes.data, len(bad_slots)) == 0, what
                unchanged(what)
            assert hip.solr_hip_set_primitive_materials(None, None, 0) == 0
            assert hip.solr_hip_set_primitive_materials(slots.ctypes.data, materials.ctypes.data, 0) == 0
            unchanged("no records")
        prepare(k, lamps)
        # the Kernel-level call takes the host route then
        assert k.set_primitive_materials(*batch) == 0
        assert k.pending_moves() == 0, "the batch was served on the device"
        assert hip.solr_hip_device_material_sets() == counter
        frame = _settle(k)
        mine = _snapshot(k, hip)
        # ... after which the scene is resident again and a batch the engine can serve is served over there
        rod = cases.first_of_type(flat, solr_types.ptCylinder)
        assert k.set_primitive_materials([rod], [cases.other_wall(flat, rod)]) == 0
        assert k.pending_moves() == 1 and hip.solr_hip_device_material_sets() == counter + 1
        k.check(0, "the host route")
    finally:
        k.finalize()
    h = _kernel(solr, "mix")
    try:
        _settle(h)
        prepare(h, lamps)
        cases.by_setter(h, ("materials", batch), lamps)
        assert h.pending_moves() == 0
        their_frame = _settle(h)
        _assert_same_snapshot(mine, _snapshot(h, hip), "the host route against the setter")
        assert same_frames(frame, their_frame)
    finally:
        h.finalize()


def test_no_resident_scene_declines(solr):
    hip = solr.hip_lib()
    k = _kernel(solr, "sticks")
    try:
        one = np.array([3], np.int32)
        counter = hip.solr_hip_device_material_sets()
        assert hip.solr_hip_set_primitive_materials(one.ctypes.data, one.ctypes.data, 1) == 0      # nothing uploaded yet
        assert hip.solr_hip_device_material_sets() == counter
        k.check(0, "a refusal is not an error")
    finally:
        k.finalize()


def test_a_morph_behind_a_served_batch_takes_the_host_route(solr):
    """k_morphPrimitives would keep the materials it finds, where morphPrimitives' loop takes the first key's: the engine
    declines - its own rule, with the keys in its hands -, the host serves the morph, and the result is the host route's"""
    hip = solr.hip_lib()
    k = _kernel(solr, "mix")
    try:
        lamps = move_cases.lamp_indices(k)
        flat = k.flat_scene()
        indices = [cases.first_of_type(flat, solr_types.ptSphere, material=1), cases.first_of_type(flat, solr_types.ptCylinder)]
        _settle(k)
        assert k.morph_frame(0.25) == 0 and k.pending_morph()           # served over there: the engine holds the keys now
        gpu_frame(k)
        morphs, sets = hip.solr_hip_device_morphs(), hip.solr_hip_device_material_sets()
        assert k.set_primitive_materials(indices, [k.extra["plain"]] * 2) == 0
        assert k.pending_moves() == 1 and hip.solr_hip_device_material_sets() == sets + 1
        gpu_frame(k)
        assert hip.solr_hip_morph_primitives(0.5, k.info["viewDistance"]) == 0
        assert k.morph_frame(0.5) == 0
        assert k.pending_moves() == 0 and not k.pending_morph(), "the morph was served behind a material set"
        assert hip.solr_hip_device_morphs() == morphs
        frame = _settle(k)
        mine = _snapshot(k, hip, EXACT_ONLY)
        k.check(0, "a morph behind a material set is not an error")
        store = k.flat_scene()
    finally:
        k.finalize()
    h = _kernel(solr, "mix")
    try:
        _settle(h)
        for step in (lambda: h.morph_frame(0.25), lambda: cases.by_setter(h, ("materials", (indices, [h.extra["plain"]] * 2)), lamps),
                     lambda: h.morph_frame(0.5)):
            _touch(h, lamps)
            step()
            assert h.pending_moves() == 0 and not h.pending_morph()
        their_frame = _settle(h)
        _assert_same_snapshot(mine, _snapshot(h, hip, EXACT_ONLY), "a morph behind a material set")
        assert same_frames(frame, their_frame)
        flat = h.flat_scene()
    finally:
        h.finalize()
    assert _same_records(store.primitives, flat.primitives) and _same_records(store.boxes, flat.boxes)
