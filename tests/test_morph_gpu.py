"""Key-frame morphing on the resident scene: GPUKernel::morphFrame (SolRx_MorphFrame, Kernel.morph_frame) with the HIP
engine blends the resident primitives on the device (solr_hip_set_morph_keys, solr_hip_morph_primitives:
sol-r_amd/csrc/solr_morph.hip) and refits the node lists like after a rotation; the host scene store follows lazily.

The bar: after any number of morphs (and rotations between them) the device holds, bit for bit, the primitive records
and the node list the host route - the loop on the host, flatten, upload: tests/test_morph_host.py - produces; the frames
rendered on the way match the oracle on the host-route scene; the host store, once it catches up, equals the host
route's; and what the engine cannot serve it refuses without changing anything."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import morph_cases  # noqa: E402
from helpers import assert_parity, compare_frames, copy_frame, gpu_frame, oracle_frame  # noqa: E402

pytestmark = pytest.mark.gpu

THIRD = float(np.float32(1) / np.float32(3))
WEIGHTS = [0.5, 0.0, 1.5, THIRD, 0.8125]
TURNS = [((0.0, 0.0, 0.0), (0.0, 0.02, 0.0)), ((10.0, -20.0, 30.0), (0.11, -0.07, 0.05)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.3))]
MIXED = [("morph", 0.5), ("rotate", TURNS[0]), ("rotate", TURNS[1]), ("morph", 0.8125), ("rotate", TURNS[2])]


def _kernel(solr, name, engine):
    return morph_cases.build(solr.Kernel(engine=engine, deterministic_seed=1), name)


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


def _apply(k, step):
    what, arg = step
    if what == "morph":
        assert k.morph_frame(arg) == 0
    else:
        k.rotate_primitives(*arg)


def _oracle_on(h, oracle, frame, randoms):
    """the engine's frame against the oracle on the scene the host-only kernel h holds"""
    flat = h.flat_scene()
    flat.randoms = randoms               # a store that never rendered has not drawn its random buffer
    si, ppi, eye, direction, angles = h.frame_parameters()
    opp, oids, orgb, _, status = oracle.render(flat, si, ppi, eye, direction, angles)
    assert status == 0
    assert_parity(compare_frames(*frame, opp, oids, orgb))


def _device_route_equals_host_route(solr, oracle, name, steps, checked, flights=1):
    """the steps on the HIP engine, a frame after each; the same on the host-only engine; `checked`: the steps whose
    frames are held to the oracle"""
    hip = solr.hip_lib()
    k = _kernel(solr, name, "hip")
    frames = []
    try:
        hip.solr_hip_set_frames_in_flight(flights)
        gpu_frame(k)                                   # uploads frame 1
        uploaded = k.device_primitives().copy()
        assert (uploaded[:, 0, 3].view(np.int32) & 0xFF == k.flat_scene().primitives["type"]).all()
        order_free = hip.solr_hip_order_free_nodes()
        morphs, rotations = hip.solr_hip_device_morphs(), hip.solr_hip_device_rotations()
        pending = 0
        for step in steps:
            _apply(k, step)
            pending = 0 if step[0] == "morph" else pending + 1
            assert k.pending_morph(), "the morph took the host route"
            assert k.pending_rotations() == pending
            frames.append(copy_frame(gpu_frame(k)))
        assert hip.solr_hip_device_morphs() - morphs == sum(1 for s in steps if s[0] == "morph")
        assert hip.solr_hip_device_rotations() - rotations == sum(1 for s in steps if s[0] == "rotate")
        assert hip.solr_hip_order_free_nodes() == order_free, "the order-free lists did not follow"
        nodes = k.device_nodes(exact=True)
        prims = k.device_primitives()
        assert k.pending_morph()                       # reading the device does not wake the host store
        caught_up = k.flat_scene()                     # this does
        assert not k.pending_morph() and k.pending_rotations() == 0
        k.compact_boxes(False)                         # flattened again: the next frame uploads the replayed scene
        fresh = copy_frame(gpu_frame(k))
        fresh_prims = k.device_primitives()
    finally:
        hip.solr_hip_set_frames_in_flight(1)
        k.finalize()

    h = _kernel(solr, name, "host-only")
    try:
        for n, step in enumerate(steps):
            _apply(h, step)
            assert not h.pending_morph() and h.pending_rotations() == 0
            if n in checked:
                _oracle_on(h, oracle, frames[n], caught_up.randoms)
        flat = h.flat_scene()
    finally:
        h.finalize()
    # the host store after its lazy replay == the host route
    assert _same_records(caught_up.boxes, flat.boxes)
    assert _same_records(caught_up.primitives, flat.primitives)
    assert _same_records(caught_up.lights, flat.lights)
    # the resident scene == what the host route would upload: all eight rows of every primitive, every node
    assert _same_bits(prims, _primitive_rows(flat, uploaded))
    assert _same_bits(fresh_prims, prims)
    assert _same_bits(nodes, _node_rows(flat))
    # ... and renders the frame a fresh upload renders
    res = compare_frames(*frames[-1], *fresh)
    assert res["ids_all_equal"] and res["max_ulp"] == 0 and res["rgb_max_diff"] == 0, res
    return order_free


@pytest.mark.parametrize("grouping", [True, False], ids=["grouped", "ungrouped"])
@pytest.mark.parametrize("name", ["mesh", "sticks", "mix"])
def test_device_morph_equals_host_morph(solr, oracle, name, grouping):
    hip = solr.hip_lib()
    hip.solr_hip_set_variant(0 if grouping else 5)      # 5: no grouping nodes, from the next upload on
    try:
        steps = [("morph", w) for w in WEIGHTS]
        _device_route_equals_host_route(solr, oracle, name, steps, checked=(0, len(steps) - 1))
    finally:
        hip.solr_hip_set_variant(0)


@pytest.mark.parametrize("flights", [1, 3], ids=["one_frame", "three_in_flight"])
def test_morphs_and_rotations_mixed(solr, oracle, flights):
    """a morph supersedes the rotations before it; the rotations after it queue behind it"""
    _device_route_equals_host_route(solr, oracle, "sticks", MIXED, checked=(len(MIXED) - 1,), flights=flights)


def test_order_free_lists_follow_a_morph(solr, oracle):
    """on a scene whose long rays walk the order-free lists: they are refitted in place - as many nodes as before,
    the leaves those of the reference's list bit for bit - and the frames are right"""
    hip = solr.hip_lib()
    k = _kernel(solr, "mesh", "hip")
    try:
        gpu_frame(k)
        order_free = hip.solr_hip_order_free_nodes()
        assert order_free > 0
        for weight in (0.8125, -0.25):
            assert k.morph_frame(weight) == 0 and k.pending_morph()
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
        assert k.pending_morph()
        opp, oids, orgb, _, status = oracle_frame(k, oracle)     # the host store catches up here
        assert status == 0 and not k.pending_morph()
        assert_parity(compare_frames(*frame, opp, oids, orgb))
    finally:
        k.finalize()


def test_a_lamp_that_moves_takes_the_host_route(solr, oracle):
    """the keys of a primitive that lights the scene differ: the light table would have to follow, the engine declines
    and the host route serves the request"""
    hip = solr.hip_lib()
    k = _kernel(solr, "lamp_moves", "hip")
    try:
        gpu_frame(k)
        morphs = hip.solr_hip_device_morphs()
        view_distance = k.info["viewDistance"]
        assert k.morph_frame(0.5) == 0                 # hands the keys over, is declined, runs on the host
        assert not k.pending_morph()
        assert hip.solr_hip_device_morphs() == morphs
        before = k.device_primitives().copy()          # (the arena is still the uploaded frame's, the keys are in place)
        assert hip.solr_hip_morph_primitives(0.5, view_distance) == 0
        assert hip.solr_hip_device_morphs() == morphs
        assert _same_bits(k.device_primitives(), before)
        k.check(0, "a refused morph is not an error")
        frame = copy_frame(gpu_frame(k))               # uploads the morphed host scene
        after = k.device_primitives()
        assert not _same_bits(after[:, :7, :3], before[:, :7, :3])
        opp, oids, orgb, _, status = oracle_frame(k, oracle)
        assert status == 0
        assert_parity(compare_frames(*frame, opp, oids, orgb))
        flat = k.flat_scene()
    finally:
        k.finalize()
    h = _kernel(solr, "lamp_moves", "host-only")
    try:
        assert h.morph_frame(0.5) == 0
        want = h.flat_scene()
    finally:
        h.finalize()
    assert _same_records(flat.primitives, want.primitives) and _same_records(flat.boxes, want.boxes)
    assert _same_records(flat.lights, want.lights)
    assert _same_bits(after, _primitive_rows(want, after))


def test_morph_requests_the_engine_cannot_serve_change_nothing(solr):
    hip = solr.hip_lib()
    k = _kernel(solr, "sticks", "hip")
    try:
        gpu_frame(k)
        view_distance = k.info["viewDistance"]
        served = hip.solr_hip_device_morphs()
        before = k.device_primitives().copy()
        n = before.shape[0]
        assert hip.solr_hip_morph_primitives(0.5, view_distance) == 0               # no keys
        records = np.zeros(n, solr.PRIMITIVE_DTYPE)
        assert hip.solr_hip_set_morph_keys(records.ctypes.data, records.ctypes.data, n - 1) == 1
        assert hip.solr_hip_morph_primitives(0.5, view_distance) == 0               # keys for another number of primitives
        assert hip.solr_hip_set_morph_keys(None, None, n) == 0                      # no keys again
        assert hip.solr_hip_morph_primitives(0.5, view_distance) == 0
        assert _same_bits(k.device_primitives(), before)
        assert k.morph_frame(0.5) == 0 and k.pending_morph()                        # the host hands its keys over
        assert hip.solr_hip_device_morphs() == served + 1
        morphed = k.device_primitives().copy()
        assert not _same_bits(morphed, before)
        assert hip.solr_hip_morph_primitives(float("nan"), view_distance) == 0
        assert hip.solr_hip_morph_primitives(float("inf"), view_distance) == 0
        assert hip.solr_hip_morph_primitives(0.25, 2.0e6) == 0                      # seeds would not commute
        assert hip.solr_hip_morph_primitives(0.25, -1.0) == 0
        assert hip.solr_hip_device_morphs() == served + 1
        assert _same_bits(k.device_primitives(), morphed)
        k.check(0, "refused morphs are not errors")
        assert hip.solr_hip_morph_primitives(0.25, view_distance) == 1              # ... and the keys are still good
        assert not _same_bits(k.device_primitives(), morphed)
    finally:
        k.finalize()


def test_touching_the_scene_store_ends_the_fast_path(solr, oracle):
    k = _kernel(solr, "sticks", "hip")
    try:
        gpu_frame(k)
        assert k.morph_frame(0.5) == 0 and k.pending_morph()
        gpu_frame(k)
        # a change of the scene store: the next morph has to see it, so it runs on the host and is uploaded
        k.L.SolR_SetPrimitiveMaterial(3, k.L.SolR_GetPrimitiveMaterial(3))
        assert not k.pending_morph()
        assert k.morph_frame(0.8125) == 0
        assert not k.pending_morph()
        frame = copy_frame(gpu_frame(k))
        opp, oids, orgb, _, status = oracle_frame(k, oracle)
        assert_parity(compare_frames(*frame, opp, oids, orgb))
        # ... after which the scene is resident and unchanged again (reading the flattened arrays is no change)
        assert k.morph_frame(0.25) == 0 and k.pending_morph()
        frame = copy_frame(gpu_frame(k))
        opp, oids, orgb, _, status = oracle_frame(k, oracle)      # catches the host store up
        assert not k.pending_morph()
        assert_parity(compare_frames(*frame, opp, oids, orgb))
    finally:
        k.finalize()
