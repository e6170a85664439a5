"""Translations and lamp moves on the host, no GPU: GPUKernel::translatePrimitives (SolRx_TranslatePrimitives,
Kernel.translate_primitives) and GPUKernel::setPrimitiveCenter (SolRx_SetPrimitiveCenter, Kernel.set_primitive_center), each
followed by compactBoxes(false) as the reference's applications follow them.

Held to: a binary32 model of the translation and of the box updates behind it, written in numpy (tests/move_cases.py), and
the rules of the journal - the "host-replay" engine is the test double that claims every rotation, translation, lamp move
and morph for a device it does not have (sol-r_amd/host/HipKernel.h ReplayKernel): its lazy replay against the eager host
route.  The real engine's kernels are held to the same host route in tests/test_moves_gpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import morph_cases  # noqa: E402
import move_cases  # noqa: E402

# a zero component; a negative one and a fraction; far enough to carry coordinates past 1e6, the seed of updateBoundingBox
TRANSLATIONS = [(300.0, 0.0, -250.5), (-1200.0, 75.0, 0.125), (2.5e6, -3.0e6, 1.5e6)]
TURNS = [((0.0, 0.0, 0.0), (0.0, 0.02, 0.0)), ((10.0, -20.0, 30.0), (0.11, -0.07, 0.05))]
MIXED = [("rotate", TURNS[0]), ("translate", TRANSLATIONS[0]), ("lamp", (1, (2500.0, 7000.0, -11000.0))), ("rotate", TURNS[1]),
         ("translate", TRANSLATIONS[1])]


def _same(a, b):
    """field by field: the structs carry padding that no one initialises"""
    return len(a) == len(b) and all(
        np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8))
        for f in a.dtype.names)


def _differing(a, b):
    return [f for f in a.dtype.names
            if not np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8))]


def _same_scene(a, b):
    return _same(a.boxes, b.boxes) and _same(a.primitives, b.primitives) and _same(a.lights, b.lights) and a.nb_lamps == b.nb_lamps


def _kernel(solr, name, engine="host-only"):
    return move_cases.build(solr.Kernel(engine=engine, deterministic_seed=1), name)


def _frame(k):
    """one frame of the frame protocol; without a device it renders nothing and says so"""
    k.L.SolRx_Render(0.0)


def _apply(k, step, lamps):
    what, arg = step
    if what == "rotate":
        k.rotate_primitives(*arg)
    elif what == "translate":
        k.translate_primitives(arg)
    else:
        k.set_primitive_center(lamps[arg[0]], arg[1])


@pytest.mark.parametrize("name", ["mesh", "sticks", "mix"])
def test_host_translation_equals_the_binary32_model(solr, name):
    k = _kernel(solr, name)
    try:
        view_distance = k.info["viewDistance"]
        before = k.flat_scene()
        p = before.primitives
        unmovable = p["index"][(p["type"] == solr.ptSphere) & (p["size"][:, 0] == 1300.0)] if name == "mix" else []
        assert len(unmovable) == (1 if name == "mix" else 0)
        moved = move_cases.moved_by_a_translation(before, unmovable)
        assert moved.sum() == len(p) - before.nb_lamps - len(unmovable)
        for t in TRANSLATIONS:
            k.translate_primitives(t)
            assert k.pending_moves() == 0
            after = k.flat_scene()
            want = move_cases.translation_model(before.primitives, moved, t)
            assert _same(after.primitives, want), (t, _differing(after.primitives, want))
            # the lamps, the unmovable sphere of the mix and every word that is not p0, p1 or p2 stay
            assert _same(after.primitives[~moved], before.primitives[~moved])
            for field in after.primitives.dtype.names:
                if field not in ("p0", "p1", "p2"):
                    assert np.array_equal(after.primitives[field], before.primitives[field]), field
            assert not np.array_equal(after.primitives["p0"][moved], before.primitives["p0"][moved])
            assert _same(after.lights, before.lights)
            boxes = move_cases.refit_model(before.boxes, want, view_distance)
            assert _same(after.boxes, boxes), (t, _differing(after.boxes, boxes))
            before = after
        assert np.abs(before.primitives["p0"][moved]).max() > 1.0e6
    finally:
        k.finalize()


def test_lazy_replay_of_the_journal_equals_the_eager_host_route(solr):
    """an engine that rotates, translates and moves lamps on its resident scene leaves the store behind by those moves, in
    order; the store, once it looks, holds what the host route holds"""
    k = _kernel(solr, "two_lamps", engine="host-replay")
    try:
        lamps = move_cases.lamp_indices(k)
        assert len(lamps) == 2
        _frame(k)                                    # the upload a real engine does here
        rotations = 0
        for n, step in enumerate(MIXED):
            _apply(k, step, lamps)
            rotations += step[0] == "rotate"
            assert k.pending_moves() == n + 1, "the move took the host route"
            assert k.pending_rotations() == rotations
            assert k.compact_boxes(False) > 0        # returns as with rotations pending: nothing to flatten here
            assert k.pending_moves() == n + 1
            _frame(k)
        lazy = k.flat_scene()                        # reading the flattened arrays wakes the store ...
        assert k.pending_moves() == 0 and k.pending_rotations() == 0
        # ... and so does a look, neither ending the fast path
        centre = (-3000.0, 6000.0, -12000.5)
        k.set_primitive_center(lamps[0], centre)
        assert k.pending_moves() == 1
        assert k.get_primitive_center(lamps[0]) == centre
        assert k.pending_moves() == 0
        k.translate_primitives(TRANSLATIONS[0])
        assert k.pending_moves() == 1
        assert k.L.SolR_GetLight(1) == lamps[1]
        assert k.pending_moves() == 0
        k.set_primitive_center(lamps[1], centre)
        assert k.pending_moves() == 1 and k.pending_rotations() == 0
        lazy2 = k.flat_scene()
        # a change of the store does end it, until the next upload
        k.L.SolR_SetPrimitiveMaterial(3, k.L.SolR_GetPrimitiveMaterial(3))
        k.translate_primitives(TRANSLATIONS[1])
        k.set_primitive_center(lamps[0], SECOND_CENTRE)
        assert k.pending_moves() == 0
        _frame(k)
        k.translate_primitives(TRANSLATIONS[1])
        k.set_primitive_center(lamps[0], centre)
        assert k.pending_moves() == 2
        lazy3 = k.flat_scene()
    finally:
        k.finalize()
    h = _kernel(solr, "two_lamps")
    try:
        assert move_cases.lamp_indices(h) == lamps
        for step in MIXED:
            _apply(h, step, lamps)
            assert h.pending_moves() == 0 and h.pending_rotations() == 0
        eager = h.flat_scene()
        h.set_primitive_center(lamps[0], centre)
        h.translate_primitives(TRANSLATIONS[0])
        h.set_primitive_center(lamps[1], centre)
        eager2 = h.flat_scene()
        h.translate_primitives(TRANSLATIONS[1])
        h.set_primitive_center(lamps[0], SECOND_CENTRE)
        h.translate_primitives(TRANSLATIONS[1])
        h.set_primitive_center(lamps[0], centre)
        eager3 = h.flat_scene()
    finally:
        h.finalize()
    for lazy_scene, eager_scene in ((lazy, eager), (lazy2, eager2), (lazy3, eager3)):
        assert _same(lazy_scene.boxes, eager_scene.boxes), _differing(lazy_scene.boxes, eager_scene.boxes)
        assert _same(lazy_scene.primitives, eager_scene.primitives), _differing(lazy_scene.primitives, eager_scene.primitives)
        assert _same(lazy_scene.lights, eager_scene.lights), _differing(lazy_scene.lights, eager_scene.lights)
    # the lamp's light record follows its primitive
    slot = 1
    assert np.array_equal(eager.lights["location"][slot, :3], np.asarray(MIXED[2][1][1], np.float32))
    assert eager.lights["primitiveId"][slot] == lamps[slot]


SECOND_CENTRE = (100.0, 9000.0, -7000.0)


def test_which_centre_moves_take_the_journal(solr):
    """the centre of a lamp of a resident, untouched scene is journalled; any other primitive's is the host's (its boxes
    would have to follow), and so is a lamp's while the scene is not resident"""
    k = _kernel(solr, "two_lamps", engine="host-replay")
    try:
        lamps = move_cases.lamp_indices(k)
        other = next(i for i in range(10) if i not in lamps)
        k.set_primitive_center(lamps[1], SECOND_CENTRE)            # nothing uploaded yet
        assert k.pending_moves() == 0
        assert k.get_primitive_center(lamps[1]) == SECOND_CENTRE
        _frame(k)
        k.set_primitive_center(lamps[1], (0.0, 8000.0, -9000.0))
        assert k.pending_moves() == 1 and k.pending_rotations() == 0
        k.set_primitive_center(other, (1.0, 2.0, 3.0))             # replays what is pending, changes the store
        assert k.pending_moves() == 0
        assert k.get_primitive_center(other) == (1.0, 2.0, 3.0)
        assert k.get_primitive_center(lamps[1]) == (0.0, 8000.0, -9000.0)
        k.set_primitive_center(lamps[1], SECOND_CENTRE)            # the store was touched: the host's, until the next upload
        assert k.pending_moves() == 0
        _frame(k)
        k.set_primitive_center(lamps[1], SECOND_CENTRE)
        assert k.pending_moves() == 1
        lazy = k.flat_scene()
    finally:
        k.finalize()
    h = _kernel(solr, "two_lamps")
    try:
        h.set_primitive_center(lamps[1], (0.0, 8000.0, -9000.0))
        h.set_primitive_center(other, (1.0, 2.0, 3.0))
        h.set_primitive_center(lamps[1], SECOND_CENTRE)
        eager = h.flat_scene()
    finally:
        h.finalize()
    assert _same_scene(lazy, eager), (_differing(lazy.primitives, eager.primitives), _differing(lazy.lights, eager.lights))


@pytest.mark.parametrize("weight", [0.5, 0.8125])
def test_a_morph_behind_a_lamp_move_puts_the_lamp_and_its_light_back(solr, weight):
    """a morph sets every primitive anew from its keys - the dragged lamp too, and on the host route the light record is
    made from it again.  The engines decline a morph behind a lamp move of their own, so the host serves it"""
    k = morph_cases.build(solr.Kernel(engine="host-replay", deterministic_seed=1), "sticks")
    try:
        lamp = move_cases.lamp_indices(k)[0]
        _frame(k)
        assert k.morph_frame(0.25) == 0 and k.pending_morph()      # (a morph in front of the move is served over there)
        k.set_primitive_center(lamp, SECOND_CENTRE)
        assert k.pending_moves() == 1 and k.pending_morph()
        assert k.morph_frame(weight) == 0
        assert not k.pending_morph() and k.pending_moves() == 0, "the morph was served behind a lamp move"
        lazy = k.flat_scene()
        _frame(k)                                                  # uploaded again: morphs are served again
        assert k.morph_frame(0.25) == 0 and k.pending_morph()
    finally:
        k.finalize()
    h = morph_cases.build(solr.Kernel(engine="host-only", deterministic_seed=1), "sticks")
    try:
        at_the_keys = h.get_primitive_center(lamp)
        assert h.morph_frame(0.25) == 0
        h.set_primitive_center(lamp, SECOND_CENTRE)
        moved = h.flat_scene()
        assert h.morph_frame(weight) == 0
        eager = h.flat_scene()
    finally:
        h.finalize()
    assert np.array_equal(moved.lights["location"][0, :3], np.asarray(SECOND_CENTRE, np.float32))
    assert np.array_equal(eager.lights["location"][0, :3], np.asarray(at_the_keys, np.float32))
    assert _same(lazy.lights, eager.lights) and _same(lazy.primitives, eager.primitives) and _same(lazy.boxes, eager.boxes)


def _move(k, what, lamp):
    if what == "rotate":
        k.rotate_primitives(*TURNS[1])
    elif what == "translate":
        k.translate_primitives(TRANSLATIONS[0])
    else:
        k.set_primitive_center(lamp, SECOND_CENTRE)


@pytest.mark.parametrize("order", [("rotate", "translate", "lamp"), ("translate", "lamp", "rotate"), ("lamp", "rotate", "translate")],
                         ids=lambda order: order[0] + "_first")
def test_moves_on_a_frame_that_is_not_the_resident_one_take_the_host_route(solr, order):
    """one offer rule (GPUKernel.h ResidentScene::offers): uploaded, untouched since, and uploaded from the current frame.
    After a frame switch the engine's resident scene is another frame's, so a rotation, a translation and a lamp's centre
    are the host's until the next upload.  Only the first move after the switch meets a scene that is still transferred
    and untouched - the host route it takes ends that for the moves behind it - so each of the three goes first once.
    Before the rule was one, rotatePrimitives and translatePrimitives left the frame out of it: with either of them first the
    first assertion below failed with 1 - a move of frame 0 offered to an engine that holds frame 1."""
    scenes = {}
    for engine in ("host-replay", "host-only"):
        k = morph_cases.build(solr.Kernel(engine=engine, deterministic_seed=1), "sticks")
        try:
            lamp = move_cases.lamp_indices(k)[0]
            _frame(k)                                # uploads frame 1
            k.set_frame(0)
            for what in order:
                _move(k, what, lamp)
                assert k.pending_moves() == 0, "a %s of frame 0 was offered to an engine whose resident scene is frame 1" % what
            assert k.pending_rotations() == 0 and move_cases.lamp_indices(k)[0] == lamp
            switched = k.flat_scene()
            _frame(k)                                # uploads frame 0: resident again
            for what in order:
                _move(k, what, lamp)
            assert k.pending_moves() == (3 if engine == "host-replay" else 0)
            assert k.pending_rotations() == (1 if engine == "host-replay" else 0)
            scenes[engine] = (switched, k.flat_scene())
            assert k.pending_moves() == 0
        finally:
            k.finalize()
    for lazy, eager in zip(scenes["host-replay"], scenes["host-only"]):
        assert _same_scene(lazy, eager), (_differing(lazy.boxes, eager.boxes), _differing(lazy.primitives, eager.primitives),
                                          _differing(lazy.lights, eager.lights))


def test_the_double_uploads_when_the_engine_would(solr):
    """HipKernel::render_begin uploads the scene - and opens the fast path again - only when an upload is due; a touch that
    leaves the scene transferred (SolR_SetPrimitiveMaterial) keeps it closed over the frames that follow, until a change of
    the store makes an upload due.  The double follows the same rule through the same transition"""
    scenes = {}
    for engine in ("host-replay", "host-only"):
        k = _kernel(solr, "two_lamps", engine=engine)
        try:
            replay = engine == "host-replay"
            _frame(k)
            k.L.SolR_SetPrimitiveMaterial(3, k.L.SolR_GetPrimitiveMaterial(3))
            _frame(k)                                # touched, no upload due: nothing is uploaded
            k.translate_primitives(TRANSLATIONS[0])
            assert k.pending_moves() == 0, "the fast path was open again without an upload"
            _frame(k)                                # the translation on the host made one due
            k.translate_primitives(TRANSLATIONS[1])
            assert k.pending_moves() == (1 if replay else 0)
            scenes[engine] = k.flat_scene()
            assert k.pending_moves() == 0
        finally:
            k.finalize()
    lazy, eager = scenes["host-replay"], scenes["host-only"]
    assert _same_scene(lazy, eager), (_differing(lazy.boxes, eager.boxes), _differing(lazy.primitives, eager.primitives))


def test_the_journal_has_a_cap_and_counts_by_kind_beyond_it(solr, capfd):
    """past ResidentScene::MAX_RECORDED_MOVES (100 000) entries a move is counted by kind and not recorded.  An engine that
    hands back its primitives makes up for that; the double does not, and the store says that it lags - so the store after
    this is compared to nothing: only the counts and that line are held"""
    k = _kernel(solr, "two_lamps", engine="host-replay")
    try:
        lamps = move_cases.lamp_indices(k)
        _frame(k)
        k.rotate_primitives(*TURNS[0])
        set_center = k.L.SolRx_SetPrimitiveCenter
        for n in range(100000):
            set_center(lamps[n & 1], 100.0, 9000.0, -7000.0 + (n & 7))
        k.translate_primitives(TRANSLATIONS[0])
        k.rotate_primitives(*TURNS[1])
        assert k.pending_moves() == 100003
        assert k.pending_rotations() == 2
        capfd.readouterr()
        k.flat_scene()
        assert k.pending_moves() == 0 and k.pending_rotations() == 0
        assert " 3 of the moves it applied were not recorded" in capfd.readouterr().err
    finally:
        k.finalize()
