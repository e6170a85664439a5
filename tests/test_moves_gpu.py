"""Translations and lamp moves on the resident scene: GPUKernel::translatePrimitives and a lamp's setPrimitiveCenter with
the HIP engine run on the device (solr_hip_translate_primitives, solr_hip_move_lamp: sol-r_amd/csrc/solr_moves.hip) - the
translation refits the node lists like a rotation, the lamp move sets one primitive's centre and one light record - and the
host scene store follows lazily, through one journal with the rotations.

The bar: after any sequence of rotations, translations and lamp moves the device holds, bit for bit, the primitive
records, the node list and the light records the host route - the loops on the host, flatten, upload:
tests/test_moves_host.py - produces; the frames rendered on the way match the oracle on the host-route scene; the host
store, once it catches up, equals the host route's; and what the engine cannot serve it refuses without changing
anything."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import morph_cases  # noqa: E402
import move_cases  # noqa: E402
from helpers import assert_parity, compare_frames, copy_frame, gpu_frame, oracle_frame  # noqa: E402

pytestmark = pytest.mark.gpu

TRANSLATIONS = [(300.0, 0.0, -250.5), (-450.0, 120.0, 80.25), (0.0, -200.0, 0.125)]
TURNS = [((0.0, 0.0, 0.0), (0.0, 0.02, 0.0)), ((10.0, -20.0, 30.0), (0.11, -0.07, 0.05)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.3))]
LAMP_1_THERE = (2500.0, 7000.0, -11000.0)
LAMP_0_THERE = (-3000.0, 6000.0, -12000.5)
MIXED = [("rotate", TURNS[0]), ("translate", TRANSLATIONS[0]), ("lamp", (1, LAMP_1_THERE)), ("rotate", TURNS[1]),
         ("lamp", (0, LAMP_0_THERE)), ("translate", TRANSLATIONS[1])]
MAX_RECORDED_ROTATIONS = 100000      # GPUKernel.h ResidentScene::MAX_RECORDED_MOVES: past it moves are counted, not recorded


def _kernel(solr, name, engine):
    return move_cases.build(solr.Kernel(engine=engine, deterministic_seed=1), name)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _same_records(a, b):
    """field by field: the structs carry padding that no one initialises"""
    return len(a) == len(b) and all(_same_bits(a[f], b[f]) for f in a.dtype.names)


def _node_rows(flat):
    """the reference's flattened boxes in the engine's node-record layout (scene_layout.h)"""
    b = flat.boxes
    rows = np.zeros((len(b), 2, 4), np.float32)
    rows[:, 0, :3] = b["min"]
    rows[:, 0, 3] = b["max"][:, 2]
    rows[:, 1, :2] = b["max"][:, :2]
    rows[:, 1, 2] = b["nbPrimitives"].view(np.float32)
    rows[:, 1, 3] = b["indexForNextBox"][:, 0].copy().view(np.float32)
    return rows


def _primitive_rows(flat, uploaded):
    """the eight rows a fresh upload of the flattened primitives leaves in the arena (scene_layout.h); the tag and the
    plane colour key are the engine's own join of the materials: those two words as `uploaded` has them"""
    p = flat.primitives
    rows = np.zeros((len(p), 8, 4), np.float32)
    for row, field in ((0, "p0"), (1, "size"), (2, "p1"), (3, "p2"), (4, "n0"), (5, "n1"), (6, "n2")):
        rows[:, row, :3] = p[field]
    rows[:, 0, 3] = uploaded[:, 0, 3]
    rows[:, 1, 3] = p["materialId"].view(np.float32)
    rows[:, 2, 3] = p["index"].view(np.float32)
    rows[:, 3, 3] = uploaded[:, 3, 3]
    rows[:, 4, 3], rows[:, 5, 3], rows[:, 6, 3] = p["vt0"][:, 0], p["vt0"][:, 1], p["vt1"][:, 0]
    rows[:, 7, 0], rows[:, 7, 1], rows[:, 7, 2] = p["vt1"][:, 1], p["vt2"][:, 0], p["vt2"][:, 1]
    return rows


def _light_rows(flat):
    """the three rows a light record is uploaded as (solr_uploads.hip h2dLightInformationOne)"""
    l = flat.lights
    rows = np.zeros((len(l), 3, 4), np.float32)
    rows[:, 0, :3] = l["location"][:, :3]
    rows[:, 0, 3] = l["primitiveId"].view(np.float32)
    rows[:, 1, :] = l["color"]
    rows[:, 2, 0] = l["materialId"].view(np.float32)
    return rows


def _apply(k, step, lamps):
    what, arg = step
    if what == "rotate":
        k.rotate_primitives(*arg)
    elif what == "translate":
        k.translate_primitives(arg)
    elif what == "lamp":
        k.set_primitive_center(lamps[arg[0]], arg[1])
    else:
        assert k.morph_frame(arg) == 0


def _oracle_on(h, oracle, frame, randoms):
    """the engine's frame against the oracle on the scene the host-only kernel h holds"""
    flat = h.flat_scene()
    flat.randoms = randoms               # a store that never rendered has not drawn its random buffer
    si, ppi, eye, direction, angles = h.frame_parameters()
    opp, oids, orgb, _, status = oracle.render(flat, si, ppi, eye, direction, angles)
    assert status == 0
    assert_parity(compare_frames(*frame, opp, oids, orgb))


def _counters(hip):
    return hip.solr_hip_device_rotations(), hip.solr_hip_device_translations(), hip.solr_hip_device_lamp_moves()


def _device_route_equals_host_route(solr, oracle, name, steps, checked, flights=1):
    """the steps on the HIP engine, a frame after each; the same on the host-only engine; `checked`: the steps whose
    frames are held to the oracle"""
    hip = solr.hip_lib()
    k = _kernel(solr, name, "hip")
    frames = []
    try:
        hip.solr_hip_set_frames_in_flight(flights)
        lamps = move_cases.lamp_indices(k)
        gpu_frame(k)                                   # uploads the scene
        uploaded = k.device_primitives().copy()
        order_free = hip.solr_hip_order_free_nodes()
        before = _counters(hip)
        for n, step in enumerate(steps):
            _apply(k, step, lamps)
            assert k.pending_moves() == n + 1, "%s took the host route" % step[0]
            frames.append(copy_frame(gpu_frame(k)))
        served = tuple(b - a for a, b in zip(before, _counters(hip)))
        assert served == tuple(sum(1 for s in steps if s[0] == what) for what in ("rotate", "translate", "lamp"))
        assert k.pending_rotations() == served[0]
        assert hip.solr_hip_order_free_nodes() == order_free, "the order-free lists did not follow"
        nodes = k.device_nodes(exact=True)
        prims = k.device_primitives()
        lights = k.device_lights()
        assert k.pending_moves() == len(steps)         # reading the device does not wake the host store
        caught_up = k.flat_scene()                     # this does
        assert k.pending_moves() == 0 and k.pending_rotations() == 0
        k.compact_boxes(False)                         # flattened again: the next frame uploads the replayed scene
        fresh = copy_frame(gpu_frame(k))
        fresh_prims, fresh_lights = k.device_primitives(), k.device_lights()
    finally:
        hip.solr_hip_set_frames_in_flight(1)
        k.finalize()

    h = _kernel(solr, name, "host-only")
    try:
        assert move_cases.lamp_indices(h) == lamps
        for n, step in enumerate(steps):
            _apply(h, step, lamps)
            assert h.pending_moves() == 0
            if n in checked:
                _oracle_on(h, oracle, frames[n], caught_up.randoms)
        flat = h.flat_scene()
    finally:
        h.finalize()
    # the host store after its lazy replay == the host route
    assert _same_records(caught_up.boxes, flat.boxes)
    assert _same_records(caught_up.primitives, flat.primitives)
    assert _same_records(caught_up.lights, flat.lights)
    # the resident scene == what the host route would upload: all eight rows of every primitive, every node, every light
    assert _same_bits(prims, _primitive_rows(flat, uploaded))
    assert _same_bits(fresh_prims, prims)
    assert _same_bits(nodes, _node_rows(flat))
    assert len(flat.lights) >= flat.nb_lamps > 0
    assert _same_bits(lights, _light_rows(flat))
    assert _same_bits(fresh_lights, lights)
    # ... and renders the frame a fresh upload renders
    res = compare_frames(*frames[-1], *fresh)
    assert res["ids_all_equal"] and res["max_ulp"] == 0 and res["rgb_max_diff"] == 0, res
    return order_free


@pytest.mark.parametrize("grouping", [True, False], ids=["grouped", "ungrouped"])
@pytest.mark.parametrize("name", ["mesh", "sticks", "mix"])
def test_device_translation_equals_host_translation(solr, oracle, name, grouping):
    hip = solr.hip_lib()
    hip.solr_hip_set_variant(0 if grouping else 5)      # 5: no grouping nodes, from the next upload on
    try:
        steps = [("translate", t) for t in TRANSLATIONS]
        _device_route_equals_host_route(solr, oracle, name, steps, checked=(0, len(steps) - 1))
    finally:
        hip.solr_hip_set_variant(0)


def test_order_free_lists_follow_a_translation(solr, oracle):
    """on a scene whose long rays walk the order-free lists: they are refitted in place - as many nodes as before,
    the leaves those of the reference's list bit for bit - and the frames are right"""
    hip = solr.hip_lib()
    k = _kernel(solr, "mesh", "hip")
    try:
        gpu_frame(k)
        order_free = hip.solr_hip_order_free_nodes()
        assert order_free > 0
        for n, t in enumerate(TRANSLATIONS[:2]):
            k.translate_primitives(t)
            assert k.pending_moves() == n + 1
            frame = copy_frame(gpu_frame(k))
            assert hip.solr_hip_order_free_nodes() == order_free
            exact = k.device_nodes(exact=True)
            leaves = exact[exact[:, 1, 2].view(np.int32) > 0].copy()
            leaves[:, 1, 3] = np.int32(1).view(np.float32)
            want = np.sort(np.ascontiguousarray(leaves).view(np.uint32).reshape(len(leaves), -1), axis=0)
            for octant in range(8):
                nodes = k.device_nodes(order_free=octant)
                mine = nodes[nodes[:, 1, 2].view(np.int32) > 0]
                got = np.sort(np.ascontiguousarray(mine).view(np.uint32).reshape(len(mine), -1), axis=0)
                assert got.shape == want.shape and np.array_equal(got, want), "octant %d holds other leaves" % octant
        assert k.pending_moves() == 2
        opp, oids, orgb, _, status = oracle_frame(k, oracle)     # the host store catches up here
        assert status == 0 and k.pending_moves() == 0
        assert_parity(compare_frames(*frame, opp, oids, orgb))
    finally:
        k.finalize()


@pytest.mark.parametrize("flights", [1, 3], ids=["one_frame", "three_in_flight"])
def test_rotations_translations_and_lamp_moves_mixed(solr, oracle, flights):
    """one journal, in order; every frame behind a lamp move is held to the oracle - only the light record makes the
    shading follow the lamp"""
    checked = tuple(n for n in range(len(MIXED)) if any(s[0] == "lamp" for s in MIXED[:n + 1]))
    assert checked == (2, 3, 4, 5)
    _device_route_equals_host_route(solr, oracle, "two_lamps", MIXED, checked=checked, flights=flights)


def test_a_morph_behind_a_lamp_move(solr, oracle):
    """k_morphPrimitives would put the dragged lamp back at its keys' place and leave its light record where the drag put
    it: the engine declines, the host serves the morph and makes the record from the primitive again"""
    hip = solr.hip_lib()
    k = morph_cases.build(solr.Kernel(engine="hip", deterministic_seed=1), "sticks")
    try:
        lamp = move_cases.lamp_indices(k)[0]
        gpu_frame(k)
        uploaded = k.device_primitives().copy()
        morphs = hip.solr_hip_device_morphs()
        k.set_primitive_center(lamp, LAMP_0_THERE)
        assert k.pending_moves() == 1
        gpu_frame(k)
        assert np.array_equal(k.device_lights()[0, 0, :3], np.asarray(LAMP_0_THERE, np.float32))
        assert k.morph_frame(0.5) == 0
        assert k.pending_moves() == 0
        frame = copy_frame(gpu_frame(k))
        lights, prims = k.device_lights(), k.device_primitives()
        # served over there only by an engine whose light rows follow the morph
        assert hip.solr_hip_device_morphs() == morphs + (1 if k.pending_morph() else 0)
        k.check(0, "a morph behind a lamp move is not an error")
        randoms = k.flat_scene().randoms
    finally:
        k.finalize()
    h = morph_cases.build(solr.Kernel(engine="host-only", deterministic_seed=1), "sticks")
    try:
        h.set_primitive_center(lamp, LAMP_0_THERE)
        assert h.morph_frame(0.5) == 0
        _oracle_on(h, oracle, frame, randoms)
        flat = h.flat_scene()
    finally:
        h.finalize()
    assert _same_bits(lights, _light_rows(flat))
    assert _same_bits(prims, _primitive_rows(flat, uploaded))
    assert not np.array_equal(lights[0, 0, :3], np.asarray(LAMP_0_THERE, np.float32))


def _long_sequence(k, lamps, total):
    for i in range(total):
        tail = i - MAX_RECORDED_ROTATIONS
        if i % 20000 == 0 or tail == 4:
            k.rotate_primitives(*TURNS[(i // 20000) % 3])
        elif i % 20000 == 10000 or tail in (1, 5):
            k.translate_primitives(TRANSLATIONS[(i // 20000) % 3])
        else:
            slot = i % 2
            k.set_primitive_center(lamps[slot], (1000.0 * slot - 3000.0 + (i % 977), 6000.0 + (i % 13), -12000.0 + 0.5 * (i % 7)))


def test_long_sequence_is_fetched_not_replayed(solr):
    """more moves than the journal records, of all three kinds, the last ones of each kind unrecorded: the host store
    takes the primitives - the lamps' among them - from the device, and equals the host route's"""
    total = MAX_RECORDED_ROTATIONS + 6
    k = _kernel(solr, "two_lamps", "hip")
    try:
        lamps = move_cases.lamp_indices(k)
        gpu_frame(k)
        _long_sequence(k, lamps, total)
        assert k.pending_moves() == total
        assert k.pending_rotations() == 7            # one per 20 000 moves, and the one past the journal's end
        fetched = k.flat_scene()
        assert k.pending_moves() == 0
        k.check(0, "the long sequence")
    finally:
        k.finalize()
    h = _kernel(solr, "two_lamps", "host-only")
    try:
        _long_sequence(h, lamps, total)
        eager = h.flat_scene()
    finally:
        h.finalize()
    assert _same_records(fetched.boxes, eager.boxes) and _same_records(fetched.primitives, eager.primitives)
    assert _same_records(fetched.lights, eager.lights)


def test_requests_the_engine_cannot_serve_change_nothing(solr, oracle):
    hip = solr.hip_lib()
    k = _kernel(solr, "two_lamps", "hip")
    f3 = C.c_float * 3
    try:
        lamps = move_cases.lamp_indices(k)
        gpu_frame(k)
        view_distance = k.info["viewDistance"]
        prims, lights, counters = k.device_primitives().copy(), k.device_lights().copy(), _counters(hip)

        def unchanged(what):
            assert _same_bits(k.device_primitives(), prims) and _same_bits(k.device_lights(), lights), what
            assert _counters(hip) == counters, what
            k.check(0, what + ": a refusal is not an error")

        t = f3(10.0, 20.0, 30.0)
        for what, refused in (("a NaN component", hip.solr_hip_translate_primitives(f3(1.0, float("nan"), 0.0), view_distance)),
                              ("an infinite component", hip.solr_hip_translate_primitives(f3(float("inf"), 0.0, 0.0), view_distance)),
                              ("no translation", hip.solr_hip_translate_primitives(None, view_distance)),
                              ("seeds would not commute", hip.solr_hip_translate_primitives(t, 2.0e6)),
                              ("viewDistance -1", hip.solr_hip_translate_primitives(t, -1.0))):
            assert refused == 0, what
            unchanged(what)
        there = f3(*LAMP_0_THERE)
        beyond = (0.0, view_distance, 0.0)       # the lamp's sphere would reach beyond its cell
        for what, refused in (("slot -1", hip.solr_hip_move_lamp(-1, there)), ("slot nbLamps", hip.solr_hip_move_lamp(len(lamps), there)),
                              ("a NaN centre", hip.solr_hip_move_lamp(0, f3(0.0, 0.0, float("nan")))),
                              ("no centre", hip.solr_hip_move_lamp(0, None)),
                              ("beyond viewDistance", hip.solr_hip_move_lamp(1, f3(*beyond)))):
            assert refused == 0, what
            unchanged(what)
        small = np.zeros((1, 4), np.float32)
        assert hip.solr_hip_read_lights(small.ctypes.data, 1) == -1
        assert hip.solr_hip_read_lights(None, 0) == 3 * lights.shape[0]
        # the Kernel-level call takes the host route then, and its frame is right
        k.set_primitive_center(lamps[1], beyond)
        assert k.pending_moves() == 0 and _counters(hip) == counters
        frame = copy_frame(gpu_frame(k))
        opp, oids, orgb, _, status = oracle_frame(k, oracle)
        assert status == 0
        assert_parity(compare_frames(*frame, opp, oids, orgb))
        assert np.array_equal(k.device_lights()[1, 0, :3], np.asarray(beyond, np.float32))
        # the next valid requests are served
        assert hip.solr_hip_translate_primitives(t, view_distance) == 1
        assert hip.solr_hip_move_lamp(0, there) == 1
        assert _counters(hip) == (counters[0], counters[1] + 1, counters[2] + 1)
        assert np.array_equal(k.device_lights()[0, 0, :3], np.asarray(LAMP_0_THERE, np.float32))
        assert np.array_equal(k.device_primitives()[0, 0, :3], np.asarray(LAMP_0_THERE, np.float32))
        k.check(0, "served requests")
    finally:
        k.finalize()


def test_a_lamp_that_is_a_plane_takes_the_host_route(solr, oracle):
    """an emissive XZ plane is a plain axis plane to the engine: the thin copy of its leaf (tightenList) is its rectangle, made
    from its p0, and k_moveLamp does not make thin copies again - the engine declines, the host moves the lamp and uploads,
    and a ray finds the lamp where it now is"""
    hip = solr.hip_lib()
    k = _kernel(solr, "plane_lamp", "hip")
    try:
        lamps = move_cases.lamp_indices(k)
        assert len(lamps) == 1
        assert k.flat_scene().primitives["type"][0] == solr.ptXZPlane
        gpu_frame(k)
        prims, lights, counters = k.device_primitives().copy(), k.device_lights().copy(), _counters(hip)
        there = (-3500.0, 6000.0, 1000.0)
        assert hip.solr_hip_move_lamp(0, (C.c_float * 3)(*there)) == 0
        assert _same_bits(k.device_primitives(), prims) and _same_bits(k.device_lights(), lights)
        assert _counters(hip) == counters
        k.check(0, "a refusal is not an error")
        k.set_primitive_center(lamps[0], there)
        assert k.pending_moves() == 0 and _counters(hip) == counters
        frame = copy_frame(gpu_frame(k))
        assert np.array_equal(k.device_lights()[0, 0, :3], np.asarray(there, np.float32))
        opp, oids, orgb, _, status = oracle_frame(k, oracle)
        assert status == 0
        assert_parity(compare_frames(*frame, opp, oids, orgb))
        # the translation of the model under it is still served, and its frame is right
        k.translate_primitives(TRANSLATIONS[0])
        assert k.pending_moves() == 1
        frame = copy_frame(gpu_frame(k))
        opp, oids, orgb, _, status = oracle_frame(k, oracle)
        assert status == 0
        assert_parity(compare_frames(*frame, opp, oids, orgb))
    finally:
        k.finalize()


def test_touching_the_scene_store_ends_the_fast_path(solr, oracle):
    k = _kernel(solr, "two_lamps", "hip")
    try:
        lamps = move_cases.lamp_indices(k)
        gpu_frame(k)
        k.translate_primitives(TRANSLATIONS[0])
        k.set_primitive_center(lamps[0], LAMP_0_THERE)
        assert k.pending_moves() == 2
        gpu_frame(k)
        # a change of the scene store: the next moves have to see it, so they run on the host and are uploaded
        k.L.SolR_SetPrimitiveMaterial(3, k.L.SolR_GetPrimitiveMaterial(3))
        assert k.pending_moves() == 0
        k.translate_primitives(TRANSLATIONS[1])
        k.set_primitive_center(lamps[1], LAMP_1_THERE)
        assert k.pending_moves() == 0
        frame = copy_frame(gpu_frame(k))
        opp, oids, orgb, _, status = oracle_frame(k, oracle)
        assert_parity(compare_frames(*frame, opp, oids, orgb))
        # ... after which the scene is resident and unchanged again (reading the flattened arrays is no change)
        k.translate_primitives(TRANSLATIONS[2])
        k.set_primitive_center(lamps[1], LAMP_0_THERE)
        assert k.pending_moves() == 2
        frame = copy_frame(gpu_frame(k))
        opp, oids, orgb, _, status = oracle_frame(k, oracle)      # catches the host store up
        assert k.pending_moves() == 0
        assert_parity(compare_frames(*frame, opp, oids, orgb))
    finally:
        k.finalize()


@pytest.mark.parametrize("what", ["rotate", "translate"])
def test_moves_on_a_frame_that_is_not_the_resident_one_take_the_host_route(solr, oracle, what):
    """tests/test_moves_host.py's test of the same name on the engine itself: after a frame switch the device still holds
    frame 1, so a rotation or a translation of frame 0 is the host's (one offer rule, GPUKernel.h ResidentScene::offers) and
    the frame that follows shows frame 0 moved, uploaded anew - not frame 1 moved in place"""
    hip = solr.hip_lib()
    k = morph_cases.build(solr.Kernel(engine="hip", deterministic_seed=1), "sticks")
    move = ("rotate", TURNS[1]) if what == "rotate" else ("translate", TRANSLATIONS[0])
    try:
        gpu_frame(k)                                   # uploads frame 1
        served = _counters(hip)
        k.set_frame(0)
        _apply(k, move, None)
        assert k.pending_moves() == 0, "a move of frame 0 was offered to an engine whose resident scene is frame 1"
        assert _counters(hip) == served
        frame = copy_frame(gpu_frame(k))               # uploads frame 0, moved on the host
        opp, oids, orgb, _, status = oracle_frame(k, oracle)
        assert status == 0
        assert_parity(compare_frames(*frame, opp, oids, orgb))
        # ... after which frame 0 is the resident one, and the next rotation is served over there
        k.rotate_primitives(*TURNS[2])
        assert k.pending_moves() == 1 and k.pending_rotations() == 1
        assert _counters(hip) == (served[0] + 1, served[1], served[2])
        frame = copy_frame(gpu_frame(k))
        opp, oids, orgb, _, status = oracle_frame(k, oracle)      # catches the host store up
        assert status == 0 and k.pending_moves() == 0
        assert_parity(compare_frames(*frame, opp, oids, orgb))
    finally:
        k.finalize()


def test_a_touch_without_an_upload_keeps_the_fast_path_closed(solr, oracle):
    """tests/test_moves_host.py test_the_double_uploads_when_the_engine_would, on the engine the double stands in for: the
    same calls, the same counts at the same points"""
    k = _kernel(solr, "two_lamps", "hip")
    try:
        gpu_frame(k)
        k.L.SolR_SetPrimitiveMaterial(3, k.L.SolR_GetPrimitiveMaterial(3))
        gpu_frame(k)                                   # touched, no upload due: nothing is uploaded
        k.translate_primitives(TRANSLATIONS[0])
        assert k.pending_moves() == 0, "the fast path was open again without an upload"
        gpu_frame(k)                                   # the translation on the host made one due
        k.translate_primitives(TRANSLATIONS[1])
        assert k.pending_moves() == 1
        frame = copy_frame(gpu_frame(k))
        opp, oids, orgb, _, status = oracle_frame(k, oracle)      # catches the host store up
        assert status == 0 and k.pending_moves() == 0
        assert_parity(compare_frames(*frame, opp, oids, orgb))
    finally:
        k.finalize()
