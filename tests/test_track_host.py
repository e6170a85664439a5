"""Key-frame tracks on the host, no GPU: GPUKernel::morphBetween (SolRx_MorphBetween, Kernel.morph_between) sets the current
frame - the stage - anew from any two other frames at any weight, by the statements GPUKernel::morphFrame runs for the first
and the last frame, keeps the stage's tree in shape and refits it.

Held to: a binary32 model of the loop written in numpy (tests/morph_cases.py morph_model) on the key frames of
tests/track_cases.py, GPUKernel::morphFrame on the scenes that has (the same loop: the same bits), and the rules for what is
refused.  The "host-replay" engine is the test double that claims every move it is offered for a device it does not have
(sol-r_amd/host/HipKernel.h ReplayKernel): what is offered and what is not, and its lazy replay against the eager host route.
The real engine's kernels are held to the same host route in tests/test_track_gpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_cases  # noqa: E402
import morph_cases  # noqa: E402
import move_cases  # noqa: E402
import track_cases  # noqa: E402

STEPS = track_cases.STEPS
TURN = ((10.0, -20.0, 30.0), (0.11, -0.07, 0.05))
STAGE = track_cases.NB_KEYS


def _same(a, b):
    """field by field, as integers: the structs carry padding that no one initialises"""
    return len(a) == len(b) and all(
        np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8))
        for f in a.dtype.names)


def _same_scene(a, b):
    return _same(a.boxes, b.boxes) and _same(a.primitives, b.primitives) and _same(a.lights, b.lights) and a.nb_lamps == b.nb_lamps


def _differing(a, b):
    return [f for f in a.dtype.names
            if not np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8))]


def _kernel(solr, name, engine="host-only", **kw):
    return track_cases.build(solr.Kernel(engine=engine, deterministic_seed=1), name, **kw)


def _frame(k):
    """one frame of the frame protocol; without a device it renders nothing and says so"""
    k.L.SolRx_Render(0.0)


@pytest.mark.parametrize("name", track_cases.NAMES)
def test_morph_between_equals_the_binary32_model_of_the_loop(solr, name):
    k = _kernel(solr, name)
    try:
        assert k.L.SolRx_GetNbFrames() == STAGE + 1 and k.set_frame(STAGE) == STAGE
        keys = track_cases.key_frames(k)
        assert len(keys[0]) == {"mesh": 290, "sticks": 85}.get(track_cases._kind(name), len(keys[0]))
        for a, b, weight in STEPS:
            current = k.flat_scene().primitives
            assert k.morph_between(a, b, weight) == 0
            assert not k.pending_morph()
            got = k.flat_scene().primitives          # flattened by the call itself: no compact_boxes here
            want = morph_cases.morph_model(keys[a], keys[b], current, weight)
            assert _same(got, want), ((a, b, weight), _differing(got, want))
        # the keys themselves are as they were
        again = track_cases.key_frames(k)
        assert all(_same(x, y) for x, y in zip(keys, again))
    finally:
        k.finalize()


def test_the_keys_of_a_track_differ_from_each_other(solr):
    """four keys that are four different frames, in every scene: a step between two of them shows which two were taken"""
    for name in ("mesh", "sticks", "mix"):
        k = _kernel(solr, name)
        try:
            keys = track_cases.key_frames(k)
            for a in range(4):
                for b in range(a + 1, 4):
                    assert not np.array_equal(keys[a]["p0"], keys[b]["p0"]), (name, a, b)
            assert all(np.array_equal(keys[0]["type"], key["type"]) for key in keys)
            if name == "sticks":
                assert len(set(keys[0]["type"].tolist())) == 4
        finally:
            k.finalize()


@pytest.mark.parametrize("name", ["mesh", "sticks", "mix"])
def test_morph_between_the_first_and_the_last_frame_is_morph_frame(solr, name):
    """on the three-frame scenes of tests/morph_cases.py: one loop, two ways in"""
    flats = []
    for between in (False, True):
        k = morph_cases.build(solr.Kernel(engine="host-only", deterministic_seed=1), name)
        try:
            for weight in (0.5, -0.25, track_cases.THIRD):
                assert (k.morph_between(0, 2, weight) if between else k.morph_frame(weight)) == 0
            flats.append(k.flat_scene())
        finally:
            k.finalize()
    assert _same_scene(flats[0], flats[1]), (_differing(flats[0].boxes, flats[1].boxes),
                                             _differing(flats[0].primitives, flats[1].primitives))


def test_requests_that_cannot_be_served_change_nothing(solr):
    k = _kernel(solr, "sticks")
    try:
        before = k.flat_scene()
        refused = [(5, 1, 0.5), (1, 5, 0.5), (-1, 1, 0.5), (1, -1, 0.5), (1000, 1, 0.5),      # no such frame
                   (STAGE, 1, 0.5), (1, STAGE, 0.5), (STAGE, STAGE, 0.5),                       # the stage is no key
                   (0, 1, float("inf")), (0, 1, float("-inf")), (0, 1, float("nan")), (0, 1, 1e300)]   # (1e300: inf in binary32)
        for a, b, weight in refused:
            assert k.morph_between(a, b, weight) == -1, (a, b, weight)
            assert _same_scene(before, k.flat_scene()), (a, b, weight)
        assert k.L.SolRx_GetNbFrames() == STAGE + 1
        assert k.morph_between(0, 1, 0.25) == 0
        assert not _same(before.primitives, k.flat_scene().primitives)
        # a key is the current frame after a frame switch, too
        k.set_frame(1)
        k.compact_boxes(False)
        before = k.flat_scene()
        assert k.morph_between(1, 2, 0.5) == -1 and k.morph_between(0, 1, 0.5) == -1
        assert _same_scene(before, k.flat_scene())
        assert k.morph_between(0, 2, 0.5) == 0       # ... and any other frame can be the stage
    finally:
        k.finalize()
    # a primitive more, or one of another type, in one of the three frames: in a key, whichever place it has, or in the stage
    for flaw in ("one_more", "swap_type"):
        for flawed, requests, fine in ((2, [(1, 2), (2, 3), (2, 2)], (0, 1)), ("stage", [(0, 1), (3, 3)], None)):
            k = _kernel(solr, "sticks", flaw=flaw, flawed=flawed)
            try:
                before = k.flat_scene()
                for a, b in requests:
                    assert k.morph_between(a, b, 0.5) == -1, (flaw, flawed, a, b)
                    assert _same_scene(before, k.flat_scene()), (flaw, flawed, a, b)
                if fine:
                    assert k.morph_between(*fine, 0.5) == 0
            finally:
                k.finalize()


def test_what_the_engine_is_offered(solr):
    """the one offer rule (ResidentScene::offers): a stage that is uploaded and untouched"""
    k = _kernel(solr, "sticks", engine="host-replay")
    try:
        assert k.morph_between(0, 1, 0.5) == 0 and not k.pending_morph()        # nothing uploaded yet
        _frame(k)                                                                # the upload a real engine does here
        assert k.morph_between(0, 1, 0.5) == 0 and k.pending_morph()
        assert k.morph_between(1, 2, 0.25) == 0 and k.pending_morph()
        assert k.compact_boxes(False) > 0 and k.pending_morph()                 # nothing to flatten: the morph stays pending
        k.flat_scene()                                                           # a look wakes the store ...
        assert not k.pending_morph()
        assert k.morph_between(2, 3, 0.5) == 0 and k.pending_morph()            # ... without ending the fast path
        k.rotate_primitives(*TURN)
        assert k.pending_morph() and k.pending_rotations() == 1
        assert k.morph_between(3, 0, 1.5) == 0                                   # supersedes the rotation
        assert k.pending_morph() and k.pending_rotations() == 0
        # a touch ends it until the next upload
        k.L.SolR_SetPrimitiveMaterial(3, k.L.SolR_GetPrimitiveMaterial(3))
        assert not k.pending_morph()
        assert k.morph_between(0, 1, 0.5) == 0 and not k.pending_morph()
        _frame(k)
        assert k.morph_between(0, 1, 0.5) == 0 and k.pending_morph()
        # refused requests are refused here as well, and leave what is pending pending
        assert k.morph_between(STAGE, 1, 0.5) == -1 and k.morph_between(0, 1, float("nan")) == -1 and k.pending_morph()
    finally:
        k.finalize()


@pytest.mark.parametrize("what", ["lamp_move", "edit"])
def test_behind_a_lamp_move_or_an_edit_on_the_device_the_host_serves(solr, what):
    k = _kernel(solr, "sticks", engine="host-replay")
    try:
        _frame(k)
        flat = k.flat_scene()
        if what == "lamp_move":
            k.set_primitive_center(move_cases.lamp_indices(k)[0], (-4000.0, 5500.0, -14000.0))
        else:
            slot = flat.nb_lamps + 5
            assert k.set_primitives(edit_cases.records([edit_cases.record(flat.primitives[slot], seed=3)])) == 0
        assert k.pending_moves() == 1, "the double did not claim the move"
        assert k.morph_between(0, 1, 0.5) == 0
        assert not k.pending_morph() and k.pending_moves() == 0
        _frame(k)                                                                # uploaded again: offered again
        assert k.morph_between(0, 1, 0.5) == 0 and k.pending_morph()
    finally:
        k.finalize()


def test_a_key_with_other_texture_coordinates_is_not_handed_over(solr):
    k = _kernel(solr, "other_uv", engine="host-replay")
    try:
        _frame(k)
        assert k.morph_between(0, 1, 0.5) == 0 and k.pending_morph()
        assert k.morph_between(2, 3, 0.5) == 0 and not k.pending_morph()        # key 3 as the second key ...
        _frame(k)
        assert k.morph_between(1, 2, 0.5) == 0 and k.pending_morph()
        assert k.morph_between(3, 0, 0.5) == 0 and not k.pending_morph()        # ... and as the first
        got = k.flat_scene()
    finally:
        k.finalize()
    h = _kernel(solr, "other_uv")
    try:
        for a, b in ((0, 1), (2, 3), (1, 2), (3, 0)):
            assert h.morph_between(a, b, 0.5) == 0
        want = h.flat_scene()
    finally:
        h.finalize()
    assert _same_scene(got, want)
    assert not np.array_equal(got.primitives["vt0"], np.zeros_like(got.primitives["vt0"]))


def test_a_frame_the_engine_has_no_slot_for_is_not_handed_over(solr):
    """key frames 256 and 257 (SOLR_MORPH_TRACK_MAX_KEYS slots, the slot is the frame's number): served on the host"""
    frames = (0, 1, 256, 257)
    flats = {}
    for engine in ("host-replay", "host-only"):
        k = _kernel(solr, "sticks", engine=engine, frames=frames)
        try:
            _frame(k)
            assert k.morph_between(0, 1, 0.5) == 0 and k.pending_morph() == (engine == "host-replay")
            assert k.morph_between(1, 256, 0.5) == 0 and not k.pending_morph()
            _frame(k)
            assert k.morph_between(257, 0, 0.25) == 0 and not k.pending_morph()
            flats[engine] = k.flat_scene()
        finally:
            k.finalize()
    assert _same_scene(flats["host-replay"], flats["host-only"])


@pytest.mark.parametrize("name", ["sticks", "mix"])
def test_lazy_replay_equals_the_eager_host_route(solr, name):
    """an engine that serves the requests leaves the store behind by one morph - its two keys and its weight - and the
    rotations after it; the store, once it looks, holds what the host route holds"""
    steps = STEPS[:3] + [TURN] + STEPS[3:]
    flats = {}
    for engine in ("host-replay", "host-only"):
        k = _kernel(solr, name, engine=engine)
        try:
            _frame(k)
            looks = []
            for step in steps:
                if len(step) == 3:
                    assert k.morph_between(*step) == 0
                else:
                    k.rotate_primitives(*step)
                assert k.pending_morph() == (engine == "host-replay")
                _frame(k)
                if step is TURN or step is steps[-1]:
                    looks.append(k.flat_scene())
                    assert not k.pending_morph() and k.pending_rotations() == 0
            flats[engine] = looks
        finally:
            k.finalize()
    for lazy, eager in zip(flats["host-replay"], flats["host-only"]):
        assert _same_scene(lazy, eager), (_differing(lazy.boxes, eager.boxes), _differing(lazy.primitives, eager.primitives))


def test_play_blends_neighbouring_keys_and_clamps(solr):
    def after(call):
        k = _kernel(solr, "sticks")
        try:
            assert call(k) == 0
            return k.flat_scene()
        finally:
            k.finalize()

    for t, (a, b, weight) in ((0.0, (0, 1, 0.0)), (0.5, (0, 1, 0.5)), (1.25, (1, 2, 0.25)), (2.75, (2, 3, 0.75)),
                              (3.0, (2, 3, 1.0)), (7.5, (2, 3, 1.0)), (-2.0, (0, 1, 0.0))):
        assert _same_scene(after(lambda k: k.play(t)), after(lambda k: k.morph_between(a, b, weight))), t
    k = _kernel(solr, "sticks")
    try:
        assert k.play(float("nan")) == -1 and k.play(float("inf")) == -1
    finally:
        k.finalize()
