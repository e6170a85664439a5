"""What solr_arena.hip derives from a node list on the device - the thin copy (k_tightenLeaves, k_tightenInner), the copy
with sorted bounds (k_sortNodeBounds), the leaf records (k_buildLeafRecords), and all of them again after a rotation on
the device - read back through solr_hip_probe_list_copy and compared with the numpy model of tests/list_copies_model.py
BIT FOR BIT, for every list the engine holds (the walk-order list, the reference's, the eight order-free ones), on
hand-made lists uploaded through the C ABI alone: leaves of one, two and three plain planes, planes that are not plain
(textured, wireframe, an emissive YZ plane), sizes that are negative, zero or infinite, a NaN coordinate, inner nodes with
nothing below them; 255, 256 and 257 nodes (the edge of a 256-thread block); leaf boxes of another host's that do not hold
their planes.  The model takes the node rows and start indices as the engine holds them (its list builders have tests of
their own) and the primitive records as read back; which primitive is a plain plane, the scene's extent and the margin
are the model's own, from the arrays that were uploaded.

And what the engine holds of a scene - what its walks are offered, every copy of every list, the primitive records, a
small frame - does not depend on what was resident before: after an upload over another scene, rotations on the device, a
finalize_scene or other materials in between, it is what the same uploads leave in a freshly initialised engine, bit for
bit (the cases at the end; no expected value is written down)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_probes as E  # noqa: E402
import list_copies_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
f4, i4 = np.float32, np.int32


def resident(solr, scene, **si_changes):
    """the hand-made list made resident (tests/engine_probes.py Resident), one lamp at its lamp primitive"""
    from oracle import probes
    si = probes._scene_info(**si_changes)
    lights = np.zeros(1, solr.LIGHT_DTYPE)
    lights["primitiveId"], lights["materialId"] = scene.lamp, M.LAMP
    lights["location"], lights["color"] = scene.prims["p0"][scene.lamp], (1.0, 1.0, 1.0, 2.0)
    materials = M.hand_made_materials(solr.MATERIAL_DTYPE)
    return si, E.Resident(solr, si, scene.boxes, scene.prims, materials, M.texture_atlas(), lights, nb_lamps=1)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(i4), np.ascontiguousarray(b).view(i4))


def _differing(a, b):
    return np.flatnonzero((np.ascontiguousarray(a).view(i4) != np.ascontiguousarray(b).view(i4)).reshape(len(a), -1).any(axis=1))


def _leaves(rows, start):
    leaf = M.counts(rows) > 0
    return sorted(zip(start[leaf].tolist(), M.counts(rows)[leaf].tolist()))


def compare_copies(solr, scene, label, margin, uploaded=True, want_free=None):
    """every copy of every list against the model; returns how many thin boxes differ from their rows, per list"""
    hip = solr.hip_lib()
    materials = M.hand_made_materials(solr.MATERIAL_DTYPE)
    kinds = M.plain_kinds(scene.prims, materials)
    records = E.primitive_records(hip)
    assert len(records) == len(scene.prims)
    assert np.array_equal(M.kinds_of_records(records) * np.isin(M.kinds_of_records(records), (2, 3, 4)), kinds), label
    thinner = {}
    exact_leaves = None
    for which, name in ((E.EXACT_LIST, "the reference's list"), (E.WALK_LIST, "the walk-order list"),
                        (E.FREE_LISTS, "the order-free lists")):
        what = "%s, %s" % (label, name)
        rows = E.list_copy(hip, which, E.NODE_ROWS)
        if which == E.FREE_LISTS and want_free is not None:
            assert (rows is not None) == want_free, what
        if rows is None:
            assert which == E.FREE_LISTS, what
            for copy in (E.THIN_COPY, E.SORTED_COPY, E.LEAF_RECORDS, E.START_INDICES):
                assert E.list_copy(hip, which, copy) is None, what
            continue
        start = E.list_copy(hip, which, E.START_INDICES)
        lists = 8 if which == E.FREE_LISTS else 1
        nb = len(rows) // lists
        assert len(start) == len(rows) == lists * nb
        if which == E.EXACT_LIST:
            assert len(rows) == len(scene.boxes) and np.array_equal(start, scene.boxes["startIndex"]), what
            if uploaded:
                assert _same(rows, M.rows_of(scene.boxes)), what
            exact_leaves = _leaves(rows, start)
        else:       # the same leaves under another hierarchy (per list)
            for l in range(lists):
                assert _leaves(rows[l * nb:(l + 1) * nb], start[l * nb:(l + 1) * nb]) == exact_leaves, (what, l)
        leaf = E.list_copy(hip, which, E.LEAF_RECORDS)
        want = M.leaf_records(rows, start, records)
        assert _same(leaf, want), (what, "leaf records", _differing(leaf, want)[:8])
        thin = E.list_copy(hip, which, E.THIN_COPY)
        if which == E.EXACT_LIST:
            assert thin is None, what             # (one copy of it: nothing walks it but VARIANT_EXACT_LIST and the census)
        else:
            assert thin is not None, what
            want = M.thin_copy(rows, start, records, kinds, margin, list_length=nb)
            assert _same(thin, want), (what, "thin copy", _differing(thin, want)[:8])
            thinner[which] = len(_differing(thin, rows))
        ordered = E.list_copy(hip, which, E.SORTED_COPY)
        if which == E.FREE_LISTS:
            assert ordered is not None, what
            want = M.sorted_copy(rows, nb)
            assert _same(ordered, want), (what, "sorted copy", _differing(ordered, want)[:8])
            assert not ordered[-1].view(i4).any()
        else:
            assert ordered is None, what
    return thinner


@pytest.mark.parametrize("nodes, odd", [(None, False), (None, True), (255, False), (256, False), (257, False), (257, True)],
                         ids=["panels", "panels-odd-bounds", "255", "256", "257", "257-odd-bounds"])
def test_every_copy_of_every_list_is_the_model_s(solr, oracle, nodes, odd):
    hip = solr.hip_lib()
    scene = M.panels(solr, nodes=nodes, odd=odd)
    si, res = resident(solr, scene)
    with res:
        offer = E.walk_offer(hip, si)
        extent = M.extent(scene.prims)
        assert f4(offer["extent"]).view(i4) == extent.view(i4) and f4(offer["margin"]).view(i4) == M.margin_of(extent).view(i4)
        # bounds that are no ordinary numbers: the engine builds no lists of its own from such a list (the walk-order list
        # is the reference's, chains collapsed) - the honest list gets all of them
        thinner = compare_copies(solr, scene, "panels", M.margin_of(extent), want_free=not odd)
        print("panels (%s nodes%s): walk-order list %d nodes, order-free lists 8 x %d; thin boxes that differ from their rows: %s"
              % (nodes or len(scene.boxes), ", odd bounds" if odd else "", offer["nbBoxes"], offer["nbBoxesFree"], thinner))
        assert thinner[E.WALK_LIST] >= 20
        if not odd:
            assert offer["nbBoxesFree"] > 0 and offer["tightLists"] == 1 and thinner[E.FREE_LISTS] >= 8 * 20
            assert hip.solr_hip_order_free_nodes() == offer["nbBoxesFree"] and hip.solr_hip_shadow_lamp_cutoff() == 1


def test_boxes_that_do_not_hold_their_planes(solr, oracle):
    """`foreign`: the enclosing check fails - no order-free lists, no lamp cut-off; the thin copy of the walk-order list is
    made all the same (cut with the boxes as uploaded), and is the model's"""
    hip = solr.hip_lib()
    scene = M.foreign(solr)
    si, res = resident(solr, scene)
    with res:
        offer = E.walk_offer(hip, si)
        assert hip.solr_hip_order_free_nodes() == 0 and hip.solr_hip_shadow_lamp_cutoff() == 0
        assert offer["nbBoxesFree"] == 0 and offer["sortedLists"] == 0 and (offer["opaqueShadows"] & 2) == 0
        thinner = compare_copies(solr, scene, "foreign", M.margin_of(M.extent(scene.prims)), want_free=False)
        assert thinner[E.WALK_LIST] >= 20
        # a walk is not offered a thin copy that was cut with boxes which do not hold their planes
        assert offer["tightLists"] == 0


def test_the_copies_follow_a_rotation_on_the_device(solr, oracle):
    hip = solr.hip_lib()
    scene = M.panels(solr)
    si, res = resident(solr, scene)
    with res:
        offer = E.walk_offer(hip, si)
        margin = M.margin_of(M.extent(scene.prims))
        compare_copies(solr, scene, "before", margin, want_free=True)
        movable = np.ones(len(scene.prims), np.uint8)
        hip.solr_hip_set_movable(C.c_void_p(movable.ctypes.data), len(movable))
        centre = np.array([100.0, -50.0, 25.0], f4)
        angles = np.array([0.02, 0.1, -0.03])
        cos, sin = np.cos(angles).astype(f4), np.sin(angles).astype(f4)
        before = E.primitive_records(hip)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        for n in range(3):
            assert hip.solr_hip_rotate_primitives(fp(centre), fp(cos), fp(sin), si.viewDistance) == 1, "the rotation was refused"
            after = E.walk_offer(hip, si)
            # the margin is the one of the upload (the extent is not worked out again on the device)
            assert f4(after["margin"]).view(i4) == margin.view(i4)
            moved = E.primitive_records(hip)
            assert not _same(moved[:, 0, :3], before[:, 0, :3])
            before = moved
            # the order-free lists are refitted with the walk-order list (they have a refit plan), not left stale: their
            # copies are compared after every rotation too, and the walks are still offered the thin copies
            assert after["nbBoxesFree"] == offer["nbBoxesFree"] > 0 and after["tightLists"] == 1 and after["sortedLists"] == 1
            thinner = compare_copies(solr, scene, "after rotation %d" % (n + 1), margin, uploaded=False, want_free=True)
            assert thinner[E.WALK_LIST] >= 20 and thinner[E.FREE_LISTS] >= 8 * 20
        assert hip.solr_hip_device_rotations() >= 3


# ---- a scene's state does not depend on what was resident before ---------------------------------------------------------
FRAME = (32, 24)
EYE, LOOK, ANGLES = (0.0, 0.0, -15000.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 6400.0)    # the viewer's default camera


def wire_materials(solr):
    """hand_made_materials with the material of every plane made wireframe (mode 2: no plane is a plain one then)"""
    m = M.hand_made_materials(solr.MATERIAL_DTYPE)
    for material in (M.PLAIN, M.TEXTURED, M.EMISSIVE, M.WIRE):
        m["attributes"][material, 2], m["attributes"][material, 3] = 2, 5
    return m


def _lights(solr, scene):
    lights = np.zeros(1, solr.LIGHT_DTYPE)
    lights["primitiveId"], lights["materialId"] = scene.lamp, M.LAMP
    lights["location"], lights["color"] = scene.prims["p0"][scene.lamp], (1.0, 1.0, 1.0, 2.0)
    return lights


def _frame_info():
    from oracle import probes
    return probes._scene_info(size_x=FRAME[0], size_y=FRAME[1])


def fresh(solr, scene, materials=None):
    """the scene uploaded into a freshly initialised engine (engine_probes.Resident finalizes it afterwards)"""
    materials = M.hand_made_materials(solr.MATERIAL_DTYPE) if materials is None else materials
    return E.Resident(solr, _frame_info(), scene.boxes, scene.prims, materials, M.texture_atlas(), _lights(solr, scene), nb_lamps=1)


def upload_scene(solr, scene, keep):
    """h2d_scene and the scene's lights, over whatever is resident"""
    hip = solr.hip_lib()
    arrays = [np.ascontiguousarray(scene.boxes), np.ascontiguousarray(scene.prims), np.zeros(1, i4), _lights(solr, scene)]
    keep += arrays
    hip.h2d_scene(0, E._p(arrays[0]), len(arrays[0]), E._p(arrays[1]), len(arrays[1]), E._p(arrays[2]), 1)
    hip.h2d_lightInformation(0, E._p(arrays[3]), 1)
    E._check(hip, 0, "upload")


def upload_materials(solr, materials, keep):
    hip = solr.hip_lib()
    keep.append(np.ascontiguousarray(materials))
    hip.h2d_materials(0, E._p(keep[-1]), len(materials))
    E._check(hip, 0, "h2d_materials")


def rotate(solr, si, times):
    """that many rotations on the device; returns what each call returned"""
    hip = solr.hip_lib()
    centre = np.array([100.0, -50.0, 25.0], f4)
    angles = np.array([0.02, 0.1, -0.03])
    cos, sin = np.cos(angles).astype(f4), np.sin(angles).astype(f4)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    return [hip.solr_hip_rotate_primitives(fp(centre), fp(cos), fp(sin), si.viewDistance) for _ in range(times)]


def snapshot(solr, scene):
    """the engine's state of the resident scene, always taken in this order (the first call builds the order-free lists when
    they are due): the eight words of the walk's offer, the three counts, every copy of every list, the primitive records,
    one frame"""
    hip = solr.hip_lib()
    E.declare(hip)
    si = _frame_info()
    state = {}
    offer = np.zeros(8, i4)
    E._check(hip, hip.solr_hip_probe_walk_offer(C.byref(si), 0, E._p(offer)), "probe_walk_offer")
    state["offer"] = offer.tobytes()
    state["order-free nodes, lamp cut-off"] = (hip.solr_hip_order_free_nodes(), hip.solr_hip_shadow_lamp_cutoff())
    state["rotations"] = hip.solr_hip_device_rotations()
    for which in (E.WALK_LIST, E.EXACT_LIST, E.FREE_LISTS):
        for what in (E.NODE_ROWS, E.THIN_COPY, E.SORTED_COPY, E.LEAF_RECORDS, E.START_INDICES):
            copy = E.list_copy(hip, which, what)
            state["list %d, copy %d" % (which, what)] = None if copy is None else copy.tobytes()
    state["primitives"] = E.primitive_records(hip).tobytes()
    w, h = FRAME
    objects = solr.Vec4i(len(scene.boxes), len(scene.prims), 1, 1)
    ppi = solr.PostProcessingInfo()
    fp = lambda a: np.array(a, f4).ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    hip.solr_hip_render(C.byref(si), C.byref(objects), C.byref(ppi), fp(EYE), fp(LOOK), fp(ANGLES))
    E._check(hip, 0, "render")
    pp, ids, rgb = np.zeros((h, w, 8), f4), np.zeros((h, w, 4), i4), np.zeros((h, w, 3), np.uint8)
    hip.solr_hip_d2h_postprocessing(C.c_void_p(pp.ctypes.data))
    hip.solr_hip_d2h(C.byref(si), C.c_void_p(rgb.ctypes.data), C.c_void_p(ids.ctypes.data))
    E._check(hip, 0, "read-back")
    assert len(np.unique(rgb.reshape(-1, 3), axis=0)) > 1, "the frame is one colour"
    state["frame: float buffer"], state["frame: ids"], state["frame: RGB8"] = pp.tobytes(), ids.tobytes(), rgb.tobytes()
    return state


def assert_same_state(mine, theirs, label, rotations=None):
    """mine == theirs, key by key; rotations: the count `mine` is to show instead of theirs"""
    assert mine.keys() == theirs.keys()
    for key in mine:
        if key == "rotations" and rotations is not None:
            assert mine[key] == rotations, (label, key, mine[key])
        else:
            assert mine[key] == theirs[key], (label, key)


_FRESH = {}


def fresh_state(solr, name):
    """the snapshot of a scene uploaded into a freshly initialised engine, taken once per scene for all the cases"""
    if name not in _FRESH:
        scene = {"panels": M.panels, "foreign": M.foreign, "panels, wireframe": M.panels}[name](solr)
        with fresh(solr, scene, wire_materials(solr) if name.endswith("wireframe") else None):
            _FRESH[name] = snapshot(solr, scene)
        assert _FRESH[name]["rotations"] == 0
    return _FRESH[name]


def test_upload_over_upload_without_a_finalize(solr, oracle):
    hip = solr.hip_lib()
    panels, foreign = M.panels(solr), M.foreign(solr)
    fresh_panels, fresh_foreign = fresh_state(solr, "panels"), fresh_state(solr, "foreign")
    keep = []
    with fresh(solr, panels):
        si = _frame_info()
        p1 = snapshot(solr, panels)
        assert_same_state(p1, fresh_panels, "P1 against panels uploaded fresh")
        movable = np.ones(len(panels.prims), np.uint8)
        hip.solr_hip_set_movable(C.c_void_p(movable.ctypes.data), len(movable))
        assert rotate(solr, si, 2) == [1, 1], "a rotation was refused"
        assert hip.solr_hip_device_rotations() == 2
        upload_scene(solr, foreign, keep)
        f1 = snapshot(solr, foreign)
        assert_same_state(f1, fresh_foreign, "F1 against foreign uploaded fresh", rotations=2)
        upload_scene(solr, panels, keep)
        p2 = snapshot(solr, panels)
        assert_same_state(p2, p1, "P2 against P1", rotations=2)
        # the movable flags went with the scene they were for: nothing rotates before they are set again
        assert rotate(solr, si, 1) == [0]
        assert_same_state(snapshot(solr, panels), p2, "after a rotation that was refused")


def test_finalize_between_scenes(solr, oracle):
    hip = solr.hip_lib()
    panels, foreign = M.panels(solr), M.foreign(solr)
    fresh_panels, fresh_foreign = fresh_state(solr, "panels"), fresh_state(solr, "foreign")
    with fresh(solr, panels):
        si = _frame_info()
        assert_same_state(snapshot(solr, panels), fresh_panels, "panels, first")
        movable = np.ones(len(panels.prims), np.uint8)
        hip.solr_hip_set_movable(C.c_void_p(movable.ctypes.data), len(movable))
        assert rotate(solr, si, 1) == [1], "the rotation was refused"
    with fresh(solr, foreign):
        assert_same_state(snapshot(solr, foreign), fresh_foreign, "foreign, after panels rotated and finalized")
    with fresh(solr, panels):
        assert_same_state(snapshot(solr, panels), fresh_panels, "panels, after foreign finalized")


def test_materials_uploaded_again(solr, oracle):
    panels = M.panels(solr)
    fresh_panels, fresh_wire = fresh_state(solr, "panels"), fresh_state(solr, "panels, wireframe")
    assert fresh_wire["offer"] != fresh_panels["offer"] and fresh_wire["primitives"] != fresh_panels["primitives"]
    keep = []
    with fresh(solr, panels):
        p1 = snapshot(solr, panels)
        assert_same_state(p1, fresh_panels, "P1 against panels uploaded fresh")
        upload_materials(solr, wire_materials(solr), keep)
        assert_same_state(snapshot(solr, panels), fresh_wire, "every plane wireframe, against a fresh upload with those materials")
        upload_materials(solr, M.hand_made_materials(solr.MATERIAL_DTYPE), keep)
        assert_same_state(snapshot(solr, panels), p1, "the first materials again, against P1")
