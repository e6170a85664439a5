"""Key-frame tracks on the resident scene: GPUKernel::morphBetween (SolRx_MorphBetween, Kernel.morph_between) with the HIP
engine hands each key frame over once (solr_hip_set_morph_track_key: k_packMorphKeys packs it into planes on the device),
blends any two of them into the resident primitives (solr_hip_morph_between: k_morphPrimitives, sol-r_amd/csrc/solr_morph.hip)
and refits the node lists like after a rotation; the host scene store follows lazily.

The bar is the one of tests/test_morph_gpu.py, whose method this file uses: after every request the device holds, bit for bit,
the primitive records and the node list the host route - the loop on the host, flatten, upload: tests/test_track_host.py -
produces; the frames rendered on the way match the oracle on the host-route scene; the host store, once it catches up, equals
the host route's; and what the engine cannot serve it refuses without changing anything."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import morph_cases  # noqa: E402
import track_cases  # noqa: E402
from helpers import assert_parity, compare_frames, copy_frame, gpu_frame, oracle_frame  # noqa: E402
from test_morph_gpu import _node_rows, _oracle_on, _primitive_rows, _same_bits, _same_records  # noqa: E402

pytestmark = pytest.mark.gpu

TURN = ((10.0, -20.0, 30.0), (0.11, -0.07, 0.05))
STEPS = track_cases.STEPS[:3] + [TURN] + track_cases.STEPS[3:]      # a rotation after the third request
ORACLE_STEPS = (track_cases.STEPS[0], track_cases.STEPS[3])         # the frames after requests 1 and 4
STAGE = track_cases.NB_KEYS


def _kernel(solr, name, engine):
    return track_cases.build(solr.Kernel(engine=engine, deterministic_seed=1), name)


def _apply(k, step):
    if len(step) == 3:
        assert k.morph_between(*step) == 0
    else:
        k.rotate_primitives(*step)


# ---- k_packMorphKeys alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_pack_kernel_gathers_every_record_into_its_planes(solr, n):
    """one lane per resident primitive, 256 lanes a workgroup: one lane, a wave less one, a wave, a wave and one, a workgroup
    less one, a workgroup, a workgroup and one.  Every float of the records distinct, so a word from the wrong record, the
    wrong field or the wrong plane shows; compared as integers"""
    hip = solr.hip_lib()
    hip.solr_hip_probe_pack_morph_key.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    hip.solr_hip_probe_pack_morph_key.restype = C.c_int
    key = np.zeros(n, solr.PRIMITIVE_DTYPE)
    words = key.view(np.float32).reshape(n, -1)
    assert words.shape[1] == 32
    words[:] = (np.arange(n * 32, dtype=np.float32).reshape(n, 32) + 1.0) * np.float32(0.25)
    words[:, 24:] = np.float32(-7.0)                  # beyond type, index and materialId: never read
    rs = np.random.RandomState(n)
    for rank_of in (rs.permutation(n), np.arange(n), np.arange(n)[::-1]):
        rank_of = np.ascontiguousarray(rank_of, np.int32)
        planes = np.zeros((7, n, 4), np.float32)
        assert hip.solr_hip_probe_pack_morph_key(key.ctypes.data, rank_of.ctypes.data, n, planes.ctypes.data) == 0
        want = np.zeros((7, n, 4), np.float32)
        for plane, field in enumerate(("p0", "p1", "p2", "n0", "n1", "n2", "size")):
            want[plane, :, :3] = key[field][rank_of]
        assert np.array_equal(planes.view(np.uint32), want.view(np.uint32))
        assert not planes.view(np.uint32)[:, :, 3].any(), "the fourth word of a row is +0"
    # ranks outside the records are refused before anything is launched
    for bad in (n, -1):
        rank_of = np.arange(n, dtype=np.int32)
        rank_of[n // 2] = bad
        assert hip.solr_hip_probe_pack_morph_key(key.ctypes.data, rank_of.ctypes.data, n, planes.ctypes.data) == -1
        hip.solr_hip_clear_error()


# ---- the device route against the host route -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mesh", "sticks", "mix"])
def test_device_route_equals_host_route(solr, oracle, name):
    hip = solr.hip_lib()
    k = _kernel(solr, name, "hip")
    frames, arenas = {}, []
    try:
        gpu_frame(k)                                   # uploads the stage
        uploaded = k.device_primitives().copy()
        assert (uploaded[:, 0, 3].view(np.int32) & 0xFF == k.flat_scene().primitives["type"]).all()
        order_free = hip.solr_hip_order_free_nodes()
        served, two_key, rotations = hip.solr_hip_device_track_morphs(), hip.solr_hip_device_morphs(), hip.solr_hip_device_rotations()
        assert hip.solr_hip_morph_track_keys() == 0
        named, pending = set(), 0
        for step in STEPS:
            _apply(k, step)
            if len(step) == 3:
                served, pending = served + 1, 0
                named |= {step[0], step[1]}
            else:
                rotations, pending = rotations + 1, pending + 1
            assert k.pending_morph(), "the request took the host route"
            assert k.pending_rotations() == pending
            assert hip.solr_hip_device_track_morphs() == served and hip.solr_hip_device_rotations() == rotations
            assert hip.solr_hip_morph_track_keys() == len(named)
            frame = copy_frame(gpu_frame(k))
            if step in ORACLE_STEPS:
                frames[step] = frame
            arenas.append((k.device_primitives().copy(), k.device_nodes(exact=True).copy()))
            assert hip.solr_hip_order_free_nodes() == order_free, "the order-free lists did not follow"
        assert hip.solr_hip_device_morphs() == two_key
        assert k.pending_morph()                       # reading the device does not wake the host store
        k.sync_host()                                  # this does
        assert not k.pending_morph() and k.pending_rotations() == 0
        caught_up = k.flat_scene()
        k.compact_boxes(False)                         # flattened again: the next frame uploads the replayed scene
        fresh = copy_frame(gpu_frame(k))
        fresh_prims = k.device_primitives().copy()
        assert hip.solr_hip_morph_track_keys() == 0    # ... and the keys go with the upload
    finally:
        k.finalize()

    h = _kernel(solr, name, "host-only")
    try:
        for step, (prims, nodes) in zip(STEPS, arenas):
            _apply(h, step)
            assert not h.pending_morph() and h.pending_rotations() == 0
            flat = h.flat_scene()
            # the resident scene == what the host route would upload: all eight rows of every primitive, every node
            assert _same_bits(prims, _primitive_rows(flat, uploaded)), step
            assert _same_bits(nodes, _node_rows(flat)), step
            if step in frames:
                _oracle_on(h, oracle, frames[step], caught_up.randoms)
    finally:
        h.finalize()
    assert len(frames) == 2
    # the host store after its lazy replay == the host route
    assert _same_records(caught_up.boxes, flat.boxes)
    assert _same_records(caught_up.primitives, flat.primitives)
    assert _same_records(caught_up.lights, flat.lights)
    assert _same_bits(fresh_prims, arenas[-1][0])
    # ... and the last frame is the one a fresh upload renders
    res = compare_frames(*frame, *fresh)
    assert res["ids_all_equal"] and res["max_ulp"] == 0 and res["rgb_max_diff"] == 0, res


def test_an_upload_drops_the_keys(solr):
    hip = solr.hip_lib()
    rows = []
    k = _kernel(solr, "sticks", "hip")
    try:
        gpu_frame(k)
        uploaded = k.device_primitives().copy()
        assert k.morph_between(1, 2, 0.5) == 0 and k.pending_morph()
        assert hip.solr_hip_morph_track_keys() == 2
        served = hip.solr_hip_device_track_morphs()
        k.compact_boxes(True)                          # a tree of its own for the morphed stage: an upload is due
        assert not k.pending_morph()
        gpu_frame(k)
        assert hip.solr_hip_morph_track_keys() == 0
        again = k.device_primitives().copy()
        assert k.morph_between(1, 2, 0.5) == 0 and k.pending_morph()     # hands both keys over again
        assert hip.solr_hip_morph_track_keys() == 2 and hip.solr_hip_device_track_morphs() == served + 1
        rows = [k.device_primitives().copy(), k.device_nodes(exact=True).copy()]
    finally:
        k.finalize()
    h = _kernel(solr, "sticks", "host-only")
    try:
        assert h.morph_between(1, 2, 0.5) == 0
        h.compact_boxes(True)
        assert h.morph_between(1, 2, 0.5) == 0
        want = h.flat_scene()
    finally:
        h.finalize()
    assert uploaded.shape == again.shape
    assert _same_bits(rows[0], _primitive_rows(want, again))
    assert _same_bits(rows[1], _node_rows(want))


def test_a_lamp_that_moves_between_two_keys_takes_the_host_route(solr, oracle):
    """the lamp is elsewhere in key 2 only: keys 0 and 1 blend on the device, keys 1 and 2 on the host - the light record
    would have to follow -, and the light is where the blend puts it"""
    hip = solr.hip_lib()
    k = _kernel(solr, "lamp_moves", "hip")
    try:
        gpu_frame(k)
        served = hip.solr_hip_device_track_morphs()
        assert k.morph_between(0, 1, 0.5) == 0 and k.pending_morph()
        assert hip.solr_hip_device_track_morphs() == served + 1
        gpu_frame(k)
        before = k.device_primitives().copy()
        assert k.morph_between(1, 2, 0.5) == 0         # hands key 2 over, is declined, runs on the host
        assert not k.pending_morph()
        assert hip.solr_hip_device_track_morphs() == served + 1 and hip.solr_hip_morph_track_keys() == 3
        assert hip.solr_hip_morph_between(1, 2, 0.5, k.info["viewDistance"]) == 0
        assert hip.solr_hip_morph_between(2, 1, 0.5, k.info["viewDistance"]) == 0
        assert _same_bits(k.device_primitives(), before)
        k.check(0, "a declined request is not an error")
        frame = copy_frame(gpu_frame(k))               # uploads the morphed host scene
        after = k.device_primitives().copy()
        opp, oids, orgb, _, status = oracle_frame(k, oracle)
        assert status == 0
        assert_parity(compare_frames(*frame, opp, oids, orgb))
        lights = k.device_lights().copy()
        flat = k.flat_scene()
    finally:
        k.finalize()
    # (-5000, 5000, -15000) + 0.5 * ((-1000, 6500, -12000) - (-5000, 5000, -15000)), exact in binary32
    assert lights.shape[0] == 1 and np.array_equal(lights[0, 0, :3], np.array([-3000.0, 5750.0, -13500.0], np.float32))
    h = _kernel(solr, "lamp_moves", "host-only")
    try:
        assert h.morph_between(0, 1, 0.5) == 0 and h.morph_between(1, 2, 0.5) == 0
        want = h.flat_scene()
    finally:
        h.finalize()
    assert _same_records(flat.primitives, want.primitives) and _same_records(flat.boxes, want.boxes)
    assert _same_records(flat.lights, want.lights)
    assert _same_bits(after, _primitive_rows(want, after))


def test_a_key_with_other_texture_coordinates_takes_the_host_route(solr):
    hip = solr.hip_lib()
    k = _kernel(solr, "other_uv", "hip")
    try:
        gpu_frame(k)
        served = hip.solr_hip_device_track_morphs()
        assert k.morph_between(0, 1, 0.5) == 0 and k.pending_morph()
        assert k.morph_between(2, 3, 0.5) == 0 and not k.pending_morph()
        assert hip.solr_hip_device_track_morphs() == served + 1
        assert hip.solr_hip_morph_track_keys() == 3    # 0, 1 and 2: key 3 never left the host
        gpu_frame(k)
        assert k.morph_between(3, 0, 0.25) == 0 and not k.pending_morph()
        gpu_frame(k)
        after = k.device_primitives().copy()
        flat = k.flat_scene()
    finally:
        k.finalize()
    h = _kernel(solr, "other_uv", "host-only")
    try:
        for step in ((0, 1, 0.5), (2, 3, 0.5), (3, 0, 0.25)):
            assert h.morph_between(*step) == 0
        want = h.flat_scene()
    finally:
        h.finalize()
    assert _same_records(flat.primitives, want.primitives) and _same_records(flat.boxes, want.boxes)
    assert _same_bits(after, _primitive_rows(want, after))


def test_key_requests_the_engine_cannot_serve_change_nothing(solr):
    hip = solr.hip_lib()
    k = _kernel(solr, "sticks", "hip")
    try:
        gpu_frame(k)
        view_distance = k.info["viewDistance"]
        assert k.morph_between(0, 1, 0.5) == 0 and k.pending_morph()
        served = hip.solr_hip_device_track_morphs()
        morphed = k.device_primitives().copy()
        n = morphed.shape[0]
        records = np.zeros(n + 1, solr.PRIMITIVE_DTYPE)
        ranks = np.arange(n + 1, dtype=np.int32) % n
        low, high = ranks.copy(), ranks.copy()
        low[n // 2], high[3] = -1, n
        refused = [(-1, records, ranks, n), (256, records, ranks, n), (0, None, ranks, n), (0, records, None, n),
                   (0, records, ranks, n - 1), (0, records, ranks, n + 1), (0, records, ranks, 0), (1, records, low, n),
                   (1, records, high, n)]
        for slot, key, rank_of, count in refused:
            assert hip.solr_hip_set_morph_track_key(slot, None if key is None else key.ctypes.data,
                                                    None if rank_of is None else rank_of.ctypes.data, count) == 0
            assert hip.solr_hip_morph_track_keys() == 2
        for a, b, weight, distance in ((-1, 1, 0.5, view_distance), (0, 256, 0.5, view_distance), (0, 7, 0.5, view_distance),
                                       (7, 7, 0.5, view_distance), (0, 1, float("nan"), view_distance),
                                       (0, 1, float("inf"), view_distance), (0, 1, 0.25, 2.0e6), (0, 1, 0.25, -1.0)):
            assert hip.solr_hip_morph_between(a, b, weight, distance) == 0, (a, b, weight, distance)
        assert hip.solr_hip_device_track_morphs() == served
        assert _same_bits(k.device_primitives(), morphed)
        k.check(0, "refused requests are not errors")
        # the resident slots are what they were: the same request again gives the same bits
        assert hip.solr_hip_morph_between(0, 1, 0.25, view_distance) == 1
        assert not _same_bits(k.device_primitives(), morphed)
        assert hip.solr_hip_morph_between(0, 1, 0.5, view_distance) == 1
        assert _same_bits(k.device_primitives(), morphed)
        assert hip.solr_hip_device_track_morphs() == served + 2
        # a key handed over directly takes a slot of its own
        assert hip.solr_hip_set_morph_track_key(9, records.ctypes.data, ranks.ctypes.data, n) == 1
        assert hip.solr_hip_morph_track_keys() == 3
        k.check(0, "a key is no error")
    finally:
        k.finalize()


def test_two_keys_two_routes(solr):
    """morph_frame and morph_between of the first and the last frame: two entry points of the engine, one kernel, the same
    arena; each counts its own"""
    hip = solr.hip_lib()
    k = morph_cases.build(solr.Kernel(engine="hip", deterministic_seed=1), "sticks")
    try:
        gpu_frame(k)
        two_key, track = hip.solr_hip_device_morphs(), hip.solr_hip_device_track_morphs()
        assert k.morph_frame(0.3) == 0 and k.pending_morph()
        assert (hip.solr_hip_device_morphs(), hip.solr_hip_device_track_morphs()) == (two_key + 1, track)
        assert hip.solr_hip_morph_track_keys() == 0
        by_frame = (k.device_primitives().copy(), k.device_nodes(exact=True).copy())
        assert k.morph_frame(0.8125) == 0
        assert not _same_bits(k.device_primitives(), by_frame[0])
        assert k.morph_between(0, 2, 0.3) == 0 and k.pending_morph()
        assert (hip.solr_hip_device_morphs(), hip.solr_hip_device_track_morphs()) == (two_key + 2, track + 1)
        assert hip.solr_hip_morph_track_keys() == 2
        assert _same_bits(k.device_primitives(), by_frame[0])
        assert _same_bits(k.device_nodes(exact=True), by_frame[1])
    finally:
        k.finalize()
