"""Key-frame morphing on the host, no GPU: GPUKernel::morphFrame (SolRx_MorphFrame, Kernel.morph_frame) blends the current
frame anew from the first and the last key frame at any weight, by the reference's own statements
(GPUKernel::morphPrimitives, GPUKernel.cpp:1513-1572) with r = weight, keeps the frame's tree in shape and refits it.

Held to: the frame GPUKernel::morphPrimitives itself made (the same bits at weight frame / nbFrames), a binary32 model
of the loop written here in numpy (tests/morph_cases.py morph_model), and the rules for what is refused.  The "host-replay"
engine is the test double that claims every morph and rotation for a device it does not have (sol-r_amd/host/HipKernel.h
ReplayKernel): its lazy replay against the eager host route.  The real engine's kernel is held to the same host route in
tests/test_morph_gpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import morph_cases  # noqa: E402

WEIGHTS = [0.0, 1.0, 0.5, 0.8125, -0.25, 1.5]
THIRD = float(np.float32(1) / np.float32(3))   # morphPrimitives' weight of frame 1 of 3


def _same(a, b):
    """field by field: the structs carry padding that no one initialises"""
    return len(a) == len(b) and all(
        np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8))
        for f in a.dtype.names)


def _same_scene(a, b):
    return _same(a.boxes, b.boxes) and _same(a.primitives, b.primitives) and _same(a.lights, b.lights) and a.nb_lamps == b.nb_lamps


def _differing(a, b):
    return [f for f in a.dtype.names
            if not np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8))]


def _kernel(solr, name, engine="host-only", **kw):
    return morph_cases.build(solr.Kernel(engine=engine, deterministic_seed=1), name, **kw)


def _frame(k):
    """one frame of the frame protocol; without a device it renders nothing and says so"""
    k.L.SolRx_Render(0.0)


@pytest.mark.parametrize("name", morph_cases.NAMES)
def test_morph_frame_at_the_frames_own_weight_is_the_frame_morph_primitives_made(solr, name):
    k = _kernel(solr, name)
    try:
        before = k.flat_scene()
        assert len(before.primitives) > 0 and before.nb_lamps == 1
        assert k.morph_frame(THIRD) == 0
        assert not k.pending_morph()
        after = k.flat_scene()
        assert _same_scene(before, after), (_differing(before.boxes, after.boxes), _differing(before.primitives, after.primitives))
    finally:
        k.finalize()


@pytest.mark.parametrize("name", morph_cases.NAMES)
def test_morph_frame_equals_the_binary32_model_of_the_loop(solr, name):
    k = _kernel(solr, name)
    try:
        first, last = morph_cases.key_frames(k)
        for weight in WEIGHTS:
            current = k.flat_scene().primitives
            assert k.morph_frame(weight) == 0
            got = k.flat_scene().primitives
            want = morph_cases.morph_model(first, last, current, weight)
            assert _same(got, want), (weight, _differing(got, want))
        # weight 0: the first key frame's points and sizes themselves (first + 0 * (last - first))
        assert k.morph_frame(0.0) == 0
        got = k.flat_scene().primitives
        ids = np.sort(got["index"])
        rank = np.searchsorted(ids, got["index"])
        for field in ("p0", "p1", "size"):
            assert np.array_equal(got[field], first[rank][field]), field
    finally:
        k.finalize()


def test_the_model_sees_every_derivation(solr):
    """the scenes reach what setPrimitive derives per type: sizes of spheres, cylinders and cones differ between the keys
    (the model's (w, w, w)), cylinders and cones have mid-points that move, a sphere's zero normals stay zero"""
    k = _kernel(solr, "mix")
    try:
        first, last = morph_cases.key_frames(k)
        kinds = set(first["type"].tolist())
        assert {solr.ptSphere, solr.ptCylinder, solr.ptCone, solr.ptEllipsoid, solr.ptTriangle, solr.ptXYPlane, solr.ptYZPlane,
                solr.ptXZPlane, solr.ptCheckboard} <= kinds
        for kind in (solr.ptSphere, solr.ptCylinder, solr.ptCone):
            sel = first["type"] == kind
            assert (first["size"][sel, 0] != last["size"][sel, 0]).any()
            assert (first["size"][sel, 1] == first["size"][sel, 0]).all()
        balls = first["type"] == solr.ptSphere
        assert balls.any() and not first["n0"][balls].any()   # normalizeVector leaves their zero normals alone
        assert k.morph_frame(0.5) == 0
        got = k.flat_scene().primitives
        assert np.isfinite(got["n0"]).all() and np.isfinite(got["p2"]).all()
        assert not got["n0"][got["type"] == solr.ptSphere].any()
    finally:
        k.finalize()


def test_requests_that_cannot_be_served_change_nothing(solr):
    # two frames only: the current frame is a key frame whichever it is
    k = _kernel(solr, "sticks", nb_frames=2, morph=False)
    try:
        k.set_frame(1)
        k.compact_boxes(False)
        before = k.flat_scene()
        assert k.morph_frame(0.5) == -1
        assert _same_scene(before, k.flat_scene())
    finally:
        k.finalize()
    # the current frame is the first or the last frame; a weight that is not finite
    k = _kernel(solr, "sticks")
    try:
        for frame in (0, 2):
            k.set_frame(frame)
            k.compact_boxes(False)
            before = k.flat_scene()
            assert k.morph_frame(0.5) == -1
            assert _same_scene(before, k.flat_scene())
        k.set_frame(1)
        k.compact_boxes(False)
        before = k.flat_scene()
        for weight in (float("inf"), float("-inf"), float("nan"), 1e300):   # (1e300 is infinite in binary32)
            assert k.morph_frame(weight) == -1
            assert _same_scene(before, k.flat_scene())
        assert k.morph_frame(0.25) == 0
        assert not _same(before.primitives, k.flat_scene().primitives)
    finally:
        k.finalize()
    # one primitive more in the last key frame; a type swapped
    for flaw in ("one_more", "swap_type"):
        k = _kernel(solr, "sticks", **{flaw: True})
        try:
            before = k.flat_scene()
            assert k.morph_frame(0.5) == -1, flaw
            assert _same_scene(before, k.flat_scene()), flaw
        finally:
            k.finalize()


@pytest.mark.parametrize("name", ["sticks", "mix"])
def test_lazy_replay_equals_the_eager_host_route(solr, name):
    """an engine that morphs and rotates its resident scene leaves the store behind by one morph and the rotations after it
    (every rotation before the morph is superseded); the store, once it looks, holds what the host route holds"""
    steps = [("morph", 0.5), ("rotate", ((0.0, 0.0, 0.0), (0.0, 0.02, 0.0))), ("rotate", ((10.0, -20.0, 30.0), (0.11, -0.07, 0.05))),
             ("morph", 0.8125), ("rotate", ((0.0, 0.0, 0.0), (0.0, 0.0, 0.3)))]
    k = _kernel(solr, name, engine="host-replay")
    try:
        _frame(k)                                    # the upload a real engine does here
        expected_rotations = 0
        for what, arg in steps:
            if what == "morph":
                assert k.morph_frame(arg) == 0
                expected_rotations = 0
            else:
                k.rotate_primitives(*arg)
                expected_rotations += 1
            assert k.pending_morph()
            assert k.pending_rotations() == expected_rotations
            assert k.compact_boxes(False) > 0        # returns as with rotations pending: nothing to flatten here
            assert k.pending_morph()
            _frame(k)
        lazy = k.flat_scene()                        # reading the flattened arrays wakes the store ...
        assert not k.pending_morph() and k.pending_rotations() == 0
        assert k.morph_frame(0.25) == 0              # ... without ending the fast path
        assert k.pending_morph()
        lazy2 = k.flat_scene()
        # touching the store does end it
        k.L.SolR_SetPrimitiveMaterial(3, k.L.SolR_GetPrimitiveMaterial(3))
        assert k.morph_frame(0.75) == 0
        assert not k.pending_morph()
        _frame(k)
        assert k.morph_frame(0.75) == 0
        assert k.pending_morph()
    finally:
        k.finalize()
    h = _kernel(solr, name)
    try:
        for what, arg in steps:
            if what == "morph":
                assert h.morph_frame(arg) == 0
            else:
                h.rotate_primitives(*arg)
            assert not h.pending_morph() and h.pending_rotations() == 0
        eager = h.flat_scene()
        assert h.morph_frame(0.25) == 0
        eager2 = h.flat_scene()
    finally:
        h.finalize()
    assert _same_scene(lazy, eager), (_differing(lazy.boxes, eager.boxes), _differing(lazy.primitives, eager.primitives))
    assert _same_scene(lazy2, eager2)
