"""The product path of a host that renders one frame at a time (render_begin / render_end, SolR_RunKernel): an
F_STREAM instantiation of k_standardRenderer whose epilogue counts tiles into rows and bands while the image leaves
in bands, launched - with the cost order on - in the band order of k_orderTiles.  Every frame here is held to
something independent of that path: the same view rendered unstreamed (solr_hip_render with no stream request) bit
for bit, and the CPU oracle as pinned (helpers.assert_frame_pinned / assert_pass_parity).  solr_hip_probe_last_frame
says which instantiation ran, so a scene that stops selecting the kernel it is here for fails.

The frames are ragged: 203 x 131 is 26 x 17 tiles, the last tile column 3 pixels wide and the last tile row 3 pixels
tall; callers' arrays are guarded by canary bytes on both sides."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import engine_probes as E
import scenes_extra as X
import tile_order_model as M
from helpers import assert_frame_pinned, assert_pass_parity, device_frame

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# rt_device.h enum Feature
F_SPHERE, F_CYL, F_TRI, F_PLANE = 1, 4, 16, 32
F_DEEP, F_STACK, F_STREAM = 256, 512, 1024
W, H = 203, 131
CANARY = 64


def last_frame(solr):
    hip = solr.hip_lib()
    E.declare(hip)
    out = (C.c_int * 6)()
    hip.solr_hip_probe_last_frame(out)
    return {"row": out[0], "mask": out[1], "streamed": out[2], "bands": out[3], "ordered": out[4], "order_bands": out[5]}


class Guarded:
    """a caller's array of rows x width RGB pixels with CANARY bytes of a pattern before and after it"""

    def __init__(self, width, rows, channels=3, dtype=np.uint8):
        self.shape = (rows, width, channels)
        self.item = np.dtype(dtype).itemsize
        body = rows * width * channels * self.item
        self.raw = np.empty(body + 2 * CANARY, np.uint8)
        self.raw[:] = (np.arange(len(self.raw)) * 7 + 0x5B) & 0xFF
        self.pattern = self.raw.copy()
        self.array = self.raw[CANARY:CANARY + body].view(dtype).reshape(self.shape)

    @property
    def address(self):
        return self.array.ctypes.data

    def untouched_rows(self, first):
        return np.array_equal(self.raw[CANARY:].reshape(-1)[first * self.shape[1] * self.shape[2] * self.item:],
                              self.pattern[CANARY:].reshape(-1)[first * self.shape[1] * self.shape[2] * self.item:])

    def canaries_intact(self):
        return (np.array_equal(self.raw[:CANARY], self.pattern[:CANARY]) and
                np.array_equal(self.raw[-CANARY:], self.pattern[-CANARY:]))


def objects_of(solr, k):
    flat = k.flat_scene()
    return solr.Vec4i(len(flat.boxes), len(flat.primitives), flat.nb_lamps, len(flat.lights))


def render_unstreamed(solr, k):
    """the next frame's view through solr_hip_render with no stream request: (pp, ids, rgb) from the device"""
    hip = solr.hip_lib()
    si, ppi, eye, direction, angles = k.frame_parameters()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    hip.solr_hip_render(C.byref(si), C.byref(objects_of(solr, k)), C.byref(ppi), fp(eye), fp(direction), fp(angles))
    k.check(0, "solr_hip_render")
    assert last_frame(solr)["streamed"] == 0
    return device_frame(solr, si)


def run_kernel(k, rows=None):
    """SolR_RunKernel into a guarded array (rows: an array taller than the frame)"""
    si = k.frame_parameters()[0]
    out = Guarded(si.size_x, rows or si.size_y)
    assert k.L.SolR_RunKernel(0.0, out.address) == 0
    k.check(0, "SolR_RunKernel")
    assert out.canaries_intact()
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def streamed_against_twin(solr, k, expect_mask=None, rows=None):
    """one frame through SolR_RunKernel, streamed; then its twin unstreamed: delivered RGB, device pp and ids bit for bit"""
    out = run_kernel(k, rows)
    probe = last_frame(solr)
    assert probe["streamed"] == 1 and probe["bands"] == 5, probe
    if expect_mask is not None:
        assert probe["mask"] == expect_mask, (probe, expect_mask)
    si = k.frame_parameters()[0]
    h = si.size_y
    delivered = out.array[:h].copy()
    pp, ids, rgb = device_frame(solr, si)
    assert np.array_equal(delivered, rgb), "delivered bytes are not the device's image"
    tpp, tids, trgb = render_unstreamed(solr, k)
    assert np.array_equal(delivered, trgb), ("streamed frame differs from its unstreamed twin",
                                             np.argwhere((delivered != trgb).any(axis=-1))[:8].tolist())
    assert np.array_equal(bits(pp), bits(tpp)) and np.array_equal(ids, tids)
    return (pp, ids, delivered), out, probe


# ---- the instantiation matrix ----------------------------------------------------------------------------------------
SCENES = {
    # name: (build, keyword arguments, expected features of the streamed instantiation)
    "cornell": ("cornell", dict(iterations=3), F_SPHERE | F_PLANE | F_STREAM),
    "cornell, ten bounces": ("cornell", dict(iterations=10), F_SPHERE | F_PLANE | F_STACK | F_STREAM),
    "cornell, deep list": ("cornell", dict(iterations=3, extra_spheres=1500), F_SPHERE | F_PLANE | F_DEEP | F_STREAM),
    "cornell, deep list, ten bounces": ("cornell", dict(iterations=10, extra_spheres=1500),
                                        F_SPHERE | F_PLANE | F_DEEP | F_STACK | F_STREAM),
    "triangles": ("triangles_only", dict(iterations=3, backdrop=True), F_SPHERE | F_TRI | F_STREAM),
    "triangles, ten bounces": ("triangles_only", dict(iterations=10, backdrop=True), F_SPHERE | F_TRI | F_STACK | F_STREAM),
    "height field": ("height_field", dict(iterations=3, n=40), F_SPHERE | F_TRI | F_DEEP | F_STREAM),
    "height field, ten bounces": ("height_field", dict(iterations=10, n=40), F_SPHERE | F_TRI | F_DEEP | F_STACK | F_STREAM),
    "sticks": ("sticks", dict(iterations=3, backdrop=True), F_SPHERE | F_CYL | F_STREAM),
    "sticks, ten bounces": ("sticks", dict(iterations=10, backdrop=True), F_SPHERE | F_CYL | F_STACK | F_STREAM),
    "molecule": ("molecule", dict(iterations=3, atoms=2500), F_SPHERE | F_CYL | F_DEEP | F_STREAM),
    "molecule, ten bounces": ("molecule", dict(iterations=10, atoms=2500), F_SPHERE | F_CYL | F_DEEP | F_STACK | F_STREAM),
}
# row 3 (spheres, planes, triangles, cylinders: the three-bank loop only) - the Cornell box as if it had all four
ROW3 = {"row 3": dict(iterations=3), "row 3, ten bounces": dict(iterations=10)}
ROW3_MASK = F_SPHERE | F_PLANE | F_TRI | F_CYL | F_DEEP | F_STREAM


def build_scene(solr, k, name, kw, width=W, height=H):
    build, args, _ = SCENES[name] if name in SCENES else ("cornell", kw, None)
    args = dict(args, width=width, height=height)
    if build in ("triangles_only", "sticks"):
        getattr(X, build)(k, **args)
    else:
        getattr(solr.scenes, build)(k, **args)


def second_camera(k):
    eye = k.frame_parameters()[2]
    k.set_camera((float(eye[0]) + 300.0, float(eye[1]) + 120.0, float(eye[2])))


def matrix_case(solr, oracle, name, kw=None, expect=None):
    """the scene's second frame streamed at 203 x 131: against its unstreamed twin and the oracle"""
    hip = solr.hip_lib()
    k = solr.Kernel(engine="hip", deterministic_seed=1)
    build_scene(solr, k, name, kw)
    try:
        if hip.solr_hip_stream_next_image(0) != 1:
            pytest.skip("SOLR_HIP_NO_IMAGE_STREAMING=1")
        hip.solr_hip_set_tile_scheduling(0)
        assert k.L.SolRx_Render(0.0) == 0
        second_camera(k)
        frame, _, probe = streamed_against_twin(solr, k, expect)
        res = assert_frame_pinned(k, oracle, frame, 2, "%s, streamed" % name)
        k.check(0, name)
        return probe, res
    finally:
        hip.solr_hip_set_tile_scheduling(1)
        k.finalize()


@pytest.mark.parametrize("name", list(SCENES))
def test_every_streamed_instantiation_against_its_twin_and_the_oracle(solr, oracle, name):
    probe, _ = matrix_case(solr, oracle, name, expect=SCENES[name][2])
    print(name, probe)
    assert probe["row"] == {F_PLANE: 0, F_TRI: 1, F_CYL: 2}[SCENES[name][2] & (F_PLANE | F_TRI | F_CYL)]


CHILD = r"""
import importlib, json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
solr = importlib.import_module("sol-r_amd")
from oracle import loader
import test_streamed_frames_gpu as T
out = {}
for name, kw in T.ROW3.items():
    probe, res = T.matrix_case(solr, loader, name, kw)
    out[name] = probe
print(json.dumps(out))
"""


def test_row_3_streamed_in_a_child_that_forces_its_features(solr):
    """SOLR_HIP_FORCE_FEATURES=53 (read once per process): the Cornell box takes row 3, whose F_STREAM forms are the
    three-bank loop with and without F_STACK"""
    env = dict(os.environ, SOLR_HIP_FORCE_FEATURES=str(F_SPHERE | F_PLANE | F_TRI | F_CYL))
    code = CHILD % {"root": os.path.dirname(HERE), "here": HERE}
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    print(got)
    assert got["row 3"]["row"] == 3 and got["row 3"]["mask"] == ROW3_MASK, got
    assert got["row 3, ten bounces"]["row"] == 3 and got["row 3, ten bounces"]["mask"] == ROW3_MASK | F_STACK, got


# ---- entry points, the threshold, reshapes ------------------------------------------------------------------------
def test_both_entry_points_and_the_ids_route(solr, oracle):
    """SolRx_Render + GetBitmap, and solr_hip_stream_next_image(2) + solr_hip_d2h_streamed (three bands, the ids too)
    into guarded arrays"""
    hip = solr.hip_lib()
    k = solr.Kernel(engine="hip", deterministic_seed=1)
    solr.scenes.cornell(k, width=W, height=H, iterations=3)
    try:
        hip.solr_hip_set_tile_scheduling(0)
        assert k.L.SolRx_Render(0.0) == 0
        second_camera(k)
        assert k.L.SolRx_Render(0.0) == 0
        assert last_frame(solr)["streamed"] == 1
        ptr = k.L.SolRx_GetBitmap()
        got = np.frombuffer((C.c_ubyte * (W * H * 3)).from_address(ptr), np.uint8).reshape(H, W, 3).copy()
        pp, ids, rgb = device_frame(solr, k.frame_parameters()[0])
        assert np.array_equal(got, rgb)
        tpp, tids, trgb = render_unstreamed(solr, k)
        assert np.array_equal(got, trgb) and np.array_equal(bits(pp), bits(tpp)) and np.array_equal(ids, tids)
        assert_frame_pinned(k, oracle, (pp, ids, got), 2, "SolRx_Render, streamed")
        # the ids route of the C ABI
        si, ppi, eye, direction, angles = k.frame_parameters()
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        assert hip.solr_hip_stream_next_image(2) == 1
        hip.solr_hip_render(C.byref(si), C.byref(objects_of(solr, k)), C.byref(ppi), fp(eye), fp(direction), fp(angles))
        probe = last_frame(solr)
        assert probe["streamed"] == 1 and probe["bands"] == 3, probe
        image, idbuf = Guarded(W, H), Guarded(W, H, 4, np.int32)
        assert hip.solr_hip_d2h_streamed(C.c_void_p(image.address), C.c_void_p(idbuf.address)) == 1
        assert image.canaries_intact() and idbuf.canaries_intact()
        assert np.array_equal(image.array, trgb) and np.array_equal(idbuf.array, tids)
        misround = np.zeros((H, W), np.uint8)
        opp, oids, orgb, _, status = oracle.render(k.flat_scene(), si, ppi, eye, direction, angles, misround=misround)
        assert status == 0 and np.array_equal(idbuf.array, oids)
        k.check(0, "entry points")
    finally:
        hip.solr_hip_set_tile_scheduling(1)
        k.finalize()


def test_sixteen_tile_rows_stream_fifteen_do_not_and_a_reshape_keeps_its_rows(solr, oracle):
    """height 121: 16 tile rows, the last one pixel row tall - streamed; 120: 15 rows - not.  203 x 131 -> 203 x 129 keeps
    17 tile rows and the stream key (armImageStreaming leaves the height out): in an array of 131 rows the two below 129
    stay as they were"""
    hip = solr.hip_lib()
    k = solr.Kernel(engine="hip", deterministic_seed=1)
    solr.scenes.cornell(k, width=W, height=121, iterations=3)
    try:
        hip.solr_hip_set_tile_scheduling(0)
        assert k.L.SolRx_Render(0.0) == 0
        second_camera(k)
        frame, _, _ = streamed_against_twin(solr, k)
        assert_frame_pinned(k, oracle, frame, 2, "16 tile rows, the last one pixel tall")
        k.set_scene_info(height=120)
        out = run_kernel(k)
        assert last_frame(solr)["streamed"] == 0
        assert np.array_equal(out.array, device_frame(solr, k.frame_parameters()[0])[2])
        k.set_scene_info(height=131)
        run_kernel(k)
        streamed_against_twin(solr, k)
        k.set_scene_info(height=129)
        before = hip.solr_hip_stream_next_image(-2)
        frame, out, _ = streamed_against_twin(solr, k, rows=131)
        assert hip.solr_hip_stream_next_image(-2) == before + 1
        assert out.untouched_rows(129), "rows below the frame were written"
        assert_frame_pinned(k, oracle, frame, 2, "203 x 129 after 203 x 131")
        k.check(0, "threshold and reshapes")
    finally:
        hip.solr_hip_set_tile_scheduling(1)
        k.finalize()


def test_a_ragged_full_size_frame_streamed(solr, oracle):
    """1917 x 1077: 240 x 135 tiles, the last column 5 pixels wide, the last row 5 pixels tall"""
    hip = solr.hip_lib()
    k = solr.Kernel(engine="hip", deterministic_seed=1)
    solr.scenes.cornell(k, width=1917, height=1077, iterations=3)
    try:
        hip.solr_hip_set_tile_scheduling(0)
        assert k.L.SolRx_Render(0.0) == 0
        second_camera(k)
        frame, _, _ = streamed_against_twin(solr, k)
        assert_frame_pinned(k, oracle, frame, 4, "1917 x 1077, streamed")
        k.check(0, "1917 x 1077")
    finally:
        hip.solr_hip_set_tile_scheduling(1)
        k.finalize()


# ---- passes ---------------------------------------------------------------------------------------------------------
def test_refinement_and_accumulation_passes_streamed(solr, oracle):
    """passes 0 ... 13 at 203 x 131: each streamed pass is its unstreamed twin of the same sequence bit for bit and the
    oracle's pass over the engine's previous buffers; a pixel a refinement pass leaves alone keeps the previous pass's
    RGB.  Then
    frames in flight on and off: the next frame streams again, right"""
    hip = solr.hip_lib()
    k = solr.Kernel(engine="hip", deterministic_seed=1)
    solr.scenes.cornell(k, width=W, height=H, iterations=2, maxPathTracingIterations=20)
    L = k.L
    try:
        hip.solr_hip_set_tile_scheduling(0)
        assert L.SolRx_Render(0.0) == 0
        second_camera(k)
        twins = []
        for i in range(14):                                   # the sequence unstreamed
            k.set_scene_info(pathTracingIteration=i)
            twins.append(render_unstreamed(solr, k))
        previous = None
        left_alone = 0
        for i in range(14):                                   # ... and streamed
            k.set_scene_info(pathTracingIteration=i)
            out = run_kernel(k)
            probe = last_frame(solr)
            assert probe["streamed"] == 1, (i, probe)
            pp, ids, rgb = device_frame(solr, k.frame_parameters()[0])
            assert np.array_equal(out.array, rgb), i
            tpp, tids, trgb = twins[i]
            assert np.array_equal(out.array, trgb) and np.array_equal(bits(pp), bits(tpp)) and np.array_equal(ids, tids), i
            assert_pass_parity(k, oracle, (pp, ids, out.array), previous and previous[:2], what="streamed pass %d" % i)
            if previous is not None and i <= 10:
                # (refinement passes 1 ... 10 skip the pixels that are done; an accumulation pass divides by its count)
                same = (bits(pp) == bits(previous[0])).all(axis=-1)
                left_alone += int(same.sum())
                assert np.array_equal(out.array[same], previous[2][same]), i
            previous = (pp.copy(), ids.copy(), out.array.copy())
        assert left_alone > 0
        # frames in flight on, off
        k.set_scene_info(pathTracingIteration=0)
        L.SolRx_SetFramesInFlight(2)
        for _ in range(3):
            assert L.SolRx_Render(0.0) == 0
        L.SolRx_SetFramesInFlight(1)
        frame, _, _ = streamed_against_twin(solr, k)
        assert np.array_equal(frame[2], twins[0][2])
        k.check(0, "passes")
    finally:
        hip.solr_hip_set_tile_scheduling(1)
        L.SolRx_SetFramesInFlight(1)
        k.finalize()


# ---- the banded cost order, end to end ----------------------------------------------------------------------------
def camera_path(i):
    return (float(2000.0 * np.sin(0.045 * i)), float(800.0 * np.cos(0.07 * i)), -15000.0 + 40.0 * i)


def test_frames_launched_in_band_order_are_the_frames_of_no_order(solr):
    """517 x 283 (65 x 36 tiles, ragged both ways), 140 views: rendered unstreamed with tile scheduling off, then again one
    at a time through SolR_RunKernel under scheduling 2 (always ordered: band-ordered when streamed) and 1 (automatic).
    Every delivered frame is the expected one; band-ordered frames come before and after the re-sort at frame 64."""
    hip = solr.hip_lib()
    w, h, n = 517, 283, 140
    k = solr.Kernel(engine="hip", deterministic_seed=1)
    # (one bounce, a short list: tiles of nearly the same cost, so that the automatic mode keeps the band order)
    solr.scenes.cornell(k, width=w, height=h, iterations=1, glass=0, extra_spheres=4)
    try:
        hip.solr_hip_set_tile_scheduling(0)
        assert k.L.SolRx_Render(0.0) == 0
        expected = []
        for i in range(n):
            k.set_camera(camera_path(i))
            expected.append(render_unstreamed(solr, k)[2])
        assert not np.array_equal(expected[0], expected[-1])
        summary = {}
        for mode in (2, 1):
            hip.solr_hip_set_tile_scheduling(mode)
            banded = []
            for i in range(n):
                k.set_camera(camera_path(i))
                out = run_kernel(k)
                assert np.array_equal(out.array, expected[i]), (mode, i, np.argwhere((out.array != expected[i]).any(-1))[:8].tolist())
                probe = last_frame(solr)
                if probe["streamed"] and probe["ordered"]:
                    assert probe["order_bands"] == probe["bands"] == 5, probe
                    banded.append(i)
            summary[mode] = banded
        assert any(i < 64 for i in summary[2]) and any(i > 65 for i in summary[2]), summary
        k.check(0, "band order")
    finally:
        hip.solr_hip_set_tile_scheduling(1)
        k.finalize()


def test_a_frame_of_sky_in_band_order(solr):
    """uniform costs, no heavy tile: every tile waits for its band"""
    hip = solr.hip_lib()
    k = solr.Kernel(engine="hip", deterministic_seed=1)
    X.lone_light(k, width=W, height=H)
    k.set_camera((0.0, 0.0, -1.5e7))
    try:
        hip.solr_hip_set_tile_scheduling(2)
        assert k.L.SolRx_Render(0.0) == 0
        banded = 0
        for i in range(6):
            k.set_camera((float(i), 0.0, -1.5e7))
            expected = render_unstreamed(solr, k)[2]
            out = run_kernel(k)
            probe = last_frame(solr)
            banded += probe["streamed"] and probe["ordered"] and probe["order_bands"] == 5
            assert np.array_equal(out.array, expected), i
        assert banded >= 3
        k.check(0, "sky")
    finally:
        hip.solr_hip_set_tile_scheduling(1)
        k.finalize()


def test_the_full_size_mesh_keeps_its_split_order_unstreamed(solr):
    """the 100k-triangle mesh at 1920 x 1080: its horizon tiles are split into quadrant waves, so the frame keeps that
    order and is not streamed; the bytes are still the unstreamed frame's"""
    hip = solr.hip_lib()
    k = solr.Kernel(engine="hip", deterministic_seed=1)
    solr.scenes.height_field(k, width=1920, height=1080)
    try:
        assert k.L.SolRx_Render(0.0) == 0
        probes = []
        for i in range(8):
            out = run_kernel(k)
            probes.append(last_frame(solr))
            assert np.array_equal(out.array, device_frame(solr, k.frame_parameters()[0])[2]), i
        assert probes[-1]["streamed"] == 0 and probes[-1]["ordered"] == 1 and probes[-1]["order_bands"] == 0, probes
        assert np.array_equal(out.array, render_unstreamed(solr, k)[2])
        k.check(0, "1080p mesh")
    finally:
        k.finalize()


def test_the_cuts_the_frames_here_use():
    """(the streamed frames above: 17, 16 and 36 tile rows in five bands)"""
    assert M.image_streaming_cuts((H + 7) // 8) == [0, 3, 6, 10, 13, 17]
    assert M.image_streaming_cuts((121 + 7) // 8) == [0, 3, 6, 9, 12, 16]
    assert M.image_streaming_cuts((120 + 7) // 8) is None
