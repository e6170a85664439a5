"""The per-pixel buffer sets of frames in flight (solr_hip_set_frames_in_flight), seen from outside the library.

Every frame in flight has a set of its own: the float frame buffer, the primitive ids and the RGB image - and a second
RGB image once a read-back still holds the first.  Two things about them that no other test looks at:

* solr_hip_memory_usage counts every set: its float frame buffer, its ids and its FIRST image - not the second;
* every set's three buffers are its own, the sets are taken in turn, and each holds the frame rendered into it: with
  four frames in flight a moving camera gives, frame by frame, what it gives one frame at a time, bit for bit.

A Cornell box at 64 x 48, one iteration.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 64, 48
FRAMES = 8


def _sizes(solr):
    """bytes per pixel of the float frame buffer, the primitive ids and the RGB image, from the declarations"""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "solr_types.h")).read()
    depth = int(re.search(r"#define\s+SOLR_COLOR_DEPTH\s+(\d+)", header).group(1))
    return solr.PP_DTYPE.itemsize, C.sizeof(solr.Vec4i), depth


def _usage(hip):
    out = (C.c_ulonglong * 4)()
    hip.solr_hip_memory_usage(out)
    return list(out)


def _renderer(solr, hip, k):
    """render(i): frame i of a camera that moves sideways, through the boundary"""
    flat = k.flat_scene()
    si, ppi, eye, direction, angles = k.frame_parameters()
    si.pathTracingIteration = 0
    objects = solr.Vec4i(len(flat.boxes), len(flat.primitives), flat.nb_lamps, len(flat.lights))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731

    def render(i):
        e = eye.copy()
        e[0] += 150.0 * i
        hip.solr_hip_render(C.byref(si), C.byref(objects), C.byref(ppi), fp(e), fp(direction), fp(angles))

    return si, render


def test_memory_usage_counts_every_buffer_set_and_not_its_second_image(solr):
    hip = solr.hip_lib()
    pp_bytes, ids_bytes, depth = _sizes(solr)
    per_set = W * H * (pp_bytes + ids_bytes + depth)
    k = solr.Kernel(engine="hip")
    solr.scenes.cornell(k, width=W, height=H, iterations=1)
    try:
        hip.solr_hip_set_frames_in_flight(1)     # (the setting outlives finalize_scene)
        k.render()
        si, render = _renderer(solr, hip, k)
        one = _usage(hip)
        for sets in (2, 4):
            hip.solr_hip_set_frames_in_flight(sets)
            now = _usage(hip)
            print("sets", sets, "bytes", now, "one set", one, "per set", per_set)
            assert now[3] - one[3] == (sets - 1) * per_set
            assert now[:3] == one[:3]
        four = _usage(hip)
        # a read-back that still holds a set's image when the next frame is rendered into that set: the set's second image
        # (which set a frame takes goes by a count the process keeps: the fourth frame from here is on this one again)
        render(0)
        assert _usage(hip) == four
        set_before = hip.solr_hip_device_postprocessing()
        image_before = hip.solr_hip_device_bitmap()
        ticket = hip.solr_hip_d2h_image_async()
        assert ticket >= 0
        for i in range(1, 5):
            render(i)
        assert hip.solr_hip_device_postprocessing() == set_before      # the same set ...
        assert hip.solr_hip_device_bitmap() != image_before            # ... on its other image
        after = _usage(hip)
        print("with a second image", after)
        assert after == four
        assert hip.solr_hip_image_wait(ticket)
        k.check(0, "memory usage")
    finally:
        hip.solr_hip_set_frames_in_flight(1)
        k.finalize()


def test_every_buffer_set_is_its_own_and_holds_its_frame(solr):
    hip = solr.hip_lib()
    k = solr.Kernel(engine="hip")
    solr.scenes.cornell(k, width=W, height=H, iterations=1)
    try:
        hip.solr_hip_set_frames_in_flight(1)     # (the setting outlives finalize_scene)
        k.render()
        si, render = _renderer(solr, hip, k)

        def host_copies():
            pp = np.zeros((H, W, 8), np.float32)
            rgb = np.zeros((H, W, 3), np.uint8)
            ids = np.zeros((H, W, 4), np.int32)
            hip.solr_hip_d2h_postprocessing(C.c_void_p(pp.ctypes.data))
            hip.solr_hip_d2h(C.byref(si), C.c_void_p(rgb.ctypes.data), C.c_void_p(ids.ctypes.data))
            return pp.view(np.uint32), rgb, ids

        expected = []
        for i in range(FRAMES):
            render(i)
            expected.append(host_copies())
        assert not np.array_equal(expected[0][1], expected[FRAMES - 1][1])   # the camera does move

        hip.solr_hip_set_frames_in_flight(4)
        pointers, seen = [], []
        for i in range(FRAMES):
            render(i)
            pointers.append((hip.solr_hip_device_bitmap(), hip.solr_hip_device_primitive_ids(),
                             hip.solr_hip_device_postprocessing()))
            seen.append(host_copies())
        k.check(0, "four frames in flight")
        for b in range(3):
            column = [p[b] for p in pointers]
            assert all(column)
            assert len(set(column[:4])) == 4, (b, column)
            assert column[4:] == column[:4], (b, column)            # no read-back outstanding: no set changes sides
        everything = [p for row in pointers[:4] for p in row]
        assert len(set(everything)) == 12
        for i in range(FRAMES):
            for b, what in enumerate(("float frame buffer", "image", "primitive ids")):
                assert np.array_equal(seen[i][b], expected[i][b]), (i, what)
    finally:
        hip.solr_hip_set_frames_in_flight(1)
        k.finalize()
