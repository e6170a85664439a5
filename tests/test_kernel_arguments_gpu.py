"""k_standardRenderer reads its arguments where they lie, phase by phase (sol-r_amd/csrc/rt_device.h again(), renderer.h
RendererArgs): the primary ray from the parameters as they arrive, every trip of the trace, each walk, the shader, the
bounce bookkeeping and the epilogue from the kernel-argument segment once more.  A field read at the wrong offset, a
phase that kept the value of the frame before, an epilogue that addressed another frame's buffers would all show in a
small frame; these are the smallest ones in which each kind of argument decides pixels, every one held bit for bit to
the oracle as pinned (helpers.assert_frame_pinned / assert_pass_parity: ids and depth exact, RGB8 exact, float colour
<= 1 ULP but for the counted pixels behind a mis-rounded libm result - at most two, as everywhere else)."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_frame_pinned, assert_pass_parity, device_frame, gpu_frame

pytestmark = pytest.mark.gpu

W, H = 76, 44            # 10 x 6 tiles, the last column 4 pixels wide, the last row 4 pixels high
NB_MAX_ITERATIONS = 10   # include/solr_types.h


def _render_arguments(solr, k):
    flat = k.flat_scene()
    si, ppi, eye, direction, angles = k.frame_parameters()
    objects = solr.Vec4i(len(flat.boxes), len(flat.primitives), flat.nb_lamps, len(flat.lights))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    return si, (C.byref(si), C.byref(objects), C.byref(ppi), fp(eye), fp(direction), fp(angles)), (eye, direction, angles)


def test_partial_tiles_on_both_axes(solr, oracle):
    k = solr.Kernel(engine="hip")
    solr.scenes.cornell(k, width=W, height=H, iterations=3)
    try:
        print(assert_frame_pinned(k, oracle, gpu_frame(k), 2, "Cornell %d x %d, pass 0" % (W, H)))
    finally:
        k.finalize()


def test_the_same_frame_as_a_strip(solr, oracle):
    """rows 16 ... 35: firstRow and nbRows decide the primary rays, the random-buffer index and the epilogue's addresses"""
    first, rows = 16, 20
    hip = solr.hip_lib()
    k = solr.Kernel(engine="hip")
    solr.scenes.cornell(k, width=W, height=H, iterations=3)
    try:
        whole = gpu_frame(k)
        si, arguments, _ = _render_arguments(solr, k)
        si.pathTracingIteration = 0
        hip.solr_hip_set_strip(first, rows)
        hip.solr_hip_render(*arguments)
        k.check(0, "strip frame")
        pp = np.zeros((rows, W, 8), np.float32)
        hip.solr_hip_d2h_postprocessing(C.c_void_p(pp.ctypes.data))
        rgb = np.zeros((H, W, 3), np.uint8)
        ids = np.zeros((H, W, 4), np.int32)
        hip.solr_hip_d2h(C.byref(si), C.c_void_p(rgb.ctypes.data), C.c_void_p(ids.ctypes.data))
        k.check(0, "strip read-back")
        strip = (pp, ids[first:first + rows], rgb[first:first + rows])
        print(assert_pass_parity(k, oracle, strip, None, what="rows %d ... %d" % (first, first + rows - 1),
                                 first_row=first, nb_rows=rows))
        # ... and they are the rows of the whole frame
        assert np.array_equal(pp.view(np.uint32), whole[0][first:first + rows].view(np.uint32))
        assert np.array_equal(strip[1], whole[1][first:first + rows]) and np.array_equal(strip[2], whole[2][first:first + rows])
        assert not rgb[:first].any() and not rgb[first + rows:].any()
    finally:
        hip.solr_hip_set_strip(0, -1)
        k.finalize()


def test_refinement_passes_and_the_first_accumulation_passes(solr, oracle):
    """passes 1 - 3 read the ids of the pass before and deepen the bounce limit; from NB_MAX_ITERATIONS on the primary ray
    is jittered with the depth of the pass before (pp, ppi, timestamp) and the epilogue accumulates and divides"""
    k = solr.Kernel(engine="hip")
    solr.scenes.cornell(k, width=W, height=H, iterations=1, maxPathTracingIterations=40)
    try:
        previous = None
        images = []
        for it in (0, 1, 2, 3, NB_MAX_ITERATIONS, NB_MAX_ITERATIONS + 1, NB_MAX_ITERATIONS + 2):
            k.set_scene_info(pathTracingIteration=it)
            pp, ids, rgb = gpu_frame(k)
            assert_pass_parity(k, oracle, (pp, ids, rgb), previous, what="pass %d" % it)
            previous = (pp.copy(), ids.copy())
            images.append(rgb.copy())
        assert not np.array_equal(images[0], images[3]) and not np.array_equal(images[4], images[6])
    finally:
        k.finalize()


def test_two_frames_back_to_back_with_other_arguments(solr, oracle):
    """one engine, one resident scene, two frames whose arguments differ in every phase's fields: the walks' view
    distance, the shader's shadow intensity and background, the bounce's ray epsilon and limit (1, then 5: the second
    frame bounces deeper than the colour stack in LDS), the camera of the primary ray"""
    k = solr.Kernel(engine="hip")
    solr.scenes.cornell(k, width=W, height=H, iterations=1)
    try:
        first = gpu_frame(k)
        print(assert_frame_pinned(k, oracle, first, 2, "first frame"))
        k.set_scene_info(viewDistance=42000.0, shadowIntensity=0.35, rayEpsilon=0.01, bgColor=(0.3, 0.1, 0.5, 0.2),
                         nbRayIterations=5)
        k.set_camera((1800.0, 900.0, -13000.0))
        second = gpu_frame(k)
        print(assert_frame_pinned(k, oracle, second, 2, "second frame"))
        assert not np.array_equal(first[2], second[2])
        # ... and back: nothing of the second frame stays behind
        k.set_scene_info(viewDistance=solr.SCENE_DEFAULTS["viewDistance"], shadowIntensity=solr.SCENE_DEFAULTS["shadowIntensity"],
                         rayEpsilon=solr.SCENE_DEFAULTS["rayEpsilon"], bgColor=solr.SCENE_DEFAULTS["bgColor"], nbRayIterations=1)
        k.set_camera((0.0, 0.0, -15000.0))
        third = gpu_frame(k)
        assert np.array_equal(third[0].view(np.uint32), first[0].view(np.uint32))
        assert np.array_equal(third[1], first[1]) and np.array_equal(third[2], first[2])
    finally:
        k.finalize()


# 64 x 136 frames, from the likeliest to split downwards: a tile is rendered by four quadrant waves when it costs more than
# twice the mean tile (k_orderTiles), so most tiles see the background and a few see mirrors facing each other
SPLIT_CANDIDATES = [dict(room=False, iterations=10), dict(room=False, iterations=10, eye=(0.0, 0.0, -30000.0)),
                    dict(room=False, iterations=3), dict(room=True, iterations=10)]


def test_split_tiles_and_a_streamed_frame(solr, oracle):
    """64 x 136: seventeen tile rows, the fewest a frame is streamed with.  In cost order the heaviest tiles are rendered
    by four quadrant waves (the epilogue's tile, part and lane arithmetic from tileMagic / tileShift / tilesX as read
    again); streamed, the epilogue counts tiles into rows and bands (rowDone, streamPlan, streamSerial).  Every frame of
    every candidate is held to the oracle; the test wants at least one of them to have had split tiles."""
    w, h = 64, 136
    hip = solr.hip_lib()
    seen = []
    for candidate in SPLIT_CANDIDATES:
        info = dict(candidate)
        eye = info.pop("eye", (0.0, 0.0, -15000.0))
        k = solr.Kernel(engine="hip", deterministic_seed=1)
        solr.scenes.cornell(k, width=w, height=h, **info)
        k.set_camera(eye)
        try:
            hip.solr_hip_set_tile_scheduling(0)
            frame = gpu_frame(k)
            assert_frame_pinned(k, oracle, frame, 2, "raster order, %s" % candidate)
            si, arguments, _ = _render_arguments(solr, k)
            si.pathTracingIteration = 0
            hip.solr_hip_set_tile_scheduling(2)
            split = 0
            for i in range(4):
                hip.solr_hip_render(*arguments)
                hip.solr_hip_synchronize()
                k.check(0, "cost-ordered frame %d" % i)
                split = max(split, hip.solr_hip_split_tiles() if hip.solr_hip_tile_scheduling_active() == 1 else 0)
                pp, ids, rgb = device_frame(solr, si)
                assert np.array_equal(pp.view(np.uint32), frame[0].view(np.uint32)), (candidate, i)
                assert np.array_equal(ids, frame[1]) and np.array_equal(rgb, frame[2]), (candidate, i)
            seen.append(split)
            hip.solr_hip_set_tile_scheduling(0)
            if hip.solr_hip_stream_next_image(0) == 1:
                before = hip.solr_hip_stream_next_image(-2)
                assert hip.solr_hip_stream_next_image(1) == 1
                hip.solr_hip_render(*arguments)
                image = np.zeros((h, w, 3), np.uint8)
                assert hip.solr_hip_d2h_streamed_image(C.c_void_p(image.ctypes.data)) == 1
                k.check(0, "streamed frame")
                assert hip.solr_hip_stream_next_image(-2) == before + 1
                assert np.array_equal(image, frame[2])
                pp, ids, rgb = device_frame(solr, si)
                assert np.array_equal(pp.view(np.uint32), frame[0].view(np.uint32)) and np.array_equal(ids, frame[1])
        finally:
            hip.solr_hip_set_tile_scheduling(1)
            k.finalize()
        if split:
            break
    print("tiles rendered by quadrant waves, per candidate:", seen)
    assert seen[-1] > 0, "no tile was rendered by quadrant waves: the case would prove nothing"


@pytest.mark.parametrize("scene", ["molecule", "mesh"])
def test_long_node_lists(solr, oracle, scene):
    """the smallest molecule and mesh whose node lists are long enough for the three-bank node loop (F_DEEP rows: spheres
    + cylinders, spheres + triangles), two frames: the second walks the order-free lists and their sorted copies"""
    k = solr.Kernel(engine="hip")
    if scene == "molecule":
        solr.scenes.molecule(k, atoms=2500, width=W, height=H, iterations=2)
    else:
        solr.scenes.height_field(k, n=40, width=W, height=H)
    try:
        for frame in range(2):
            print(assert_frame_pinned(k, oracle, gpu_frame(k), 2, "%s, frame %d" % (scene, frame)))
        assert len(k.flat_scene().boxes) > 1024, "the node list is too short for the F_DEEP instantiation"
    finally:
        k.finalize()
