"""Primitives set anew on the host, no GPU: GPUKernel::setPrimitives (SolRx_SetPrimitives, Kernel.set_primitives) - a batch
of records, each the arguments of setPrimitive and, by flag, of setPrimitiveNormals and setPrimitiveTextureCoordinates, then
the box updates of a rotation, then compactBoxes(false).

Held to: a binary32 model of the three setters per type, written in numpy (tests/edit_cases.py edit_model), with the model
of the box updates behind them (tests/move_cases.py refit_model); the setters that were there before, called one record at a
time and followed by a translation by -0 (edit_cases.by_setters); and the rules of the journal - the "host-replay" engine
claims every batch the store's side of the engine's conditions allows (GPUKernel::editSlots) for a device it does not have:
its lazy replay against the eager host route.  The real engine's kernel is held to the same host route in
tests/test_edits_gpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_cases  # noqa: E402
import move_cases  # noqa: E402

f32 = np.float32
TRANSLATION = (300.0, 0.0, -250.5)
TURNS = [((0.0, 0.0, 0.0), (0.0, 0.02, 0.0)), ((10.0, -20.0, 30.0), (0.11, -0.07, 0.05))]
LAMP_THERE = (-3000.0, 6000.0, -12000.5)
MAX_RECORDED_MOVES = 100000          # GPUKernel.h ResidentScene::MAX_RECORDED_MOVES


def _same(a, b):
    """field by field: the structs carry padding that no one initialises"""
    return len(a) == len(b) and all(
        np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8))
        for f in a.dtype.names)


def _differing(a, b):
    return [f for f in a.dtype.names
            if not np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8))]


def _assert_same_scene(a, b, what=""):
    assert _same(a.primitives, b.primitives), (what, _differing(a.primitives, b.primitives))
    assert _same(a.boxes, b.boxes), (what, _differing(a.boxes, b.boxes))
    assert _same(a.lights, b.lights), (what, _differing(a.lights, b.lights))
    assert a.nb_lamps == b.nb_lamps


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
    elif what == "lamp":
        k.set_primitive_center(lamps[arg[0]], arg[1])
    elif what == "morph":
        assert k.morph_frame(arg) == 0
    else:
        assert k.set_primitives(arg) == 0


def _lazy_and_eager(solr, name, steps):
    """the steps on the double, a frame first and after each, every step claimed; the same on the host-only engine; the
    flattened scenes of both at the end"""
    k = _kernel(solr, name, engine="host-replay")
    try:
        lamps = move_cases.lamp_indices(k)
        _frame(k)
        for n, step in enumerate(steps):
            _apply(k, step, lamps)
            assert k.pending_moves() == n + 1, "%s took the host route" % step[0]
            assert k.compact_boxes(False) > 0        # returns as with rotations pending: nothing to flatten here
            assert k.pending_moves() == n + 1
            _frame(k)
        lazy = k.flat_scene()
        assert k.pending_moves() == 0
    finally:
        k.finalize()
    h = _kernel(solr, name)
    try:
        for step in steps:
            _apply(h, step, lamps)
            assert h.pending_moves() == 0
        eager = h.flat_scene()
    finally:
        h.finalize()
    return lazy, eager


def _scenes_by_setters(solr, name, batches):
    """the flattened scene after each of the batches by the setters one record at a time, on a kernel of its own (the
    engine is one per process: kernels follow one another, none stands beside another)"""
    s = _kernel(solr, name)
    try:
        scenes = []
        for batch in batches:
            edit_cases.by_setters(s, batch)
            scenes.append(s.flat_scene())
        return scenes
    finally:
        s.finalize()


@pytest.mark.parametrize("name", ["mesh", "sticks", "mix"])
def test_host_edits_equal_the_binary32_model_and_the_setters(solr, name):
    k = _kernel(solr, name)
    scenes = []
    try:
        view_distance = k.info["viewDistance"]
        before = k.flat_scene()
        batches = edit_cases.batches(before, name)
        assert len(batches) == 3
        for batch in batches:
            far, there = edit_cases.far_index(before, name, batch)
            assert edit_cases.outside_old_leaf(before, far, there)
            assert k.set_primitives(batch) == 0
            assert k.pending_moves() == 0
            after = k.flat_scene()
            want = edit_cases.edit_model(before.primitives, batch)
            assert _same(after.primitives, want), (len(batch), _differing(after.primitives, want))
            edited = np.isin(before.primitives["index"], batch["index"])
            assert edited.sum() == len(batch)
            assert _same(after.primitives[~edited], before.primitives[~edited])
            assert not np.array_equal(after.primitives["p0"][edited], before.primitives["p0"][edited])
            boxes = edit_cases.refit_model(before.boxes, want, view_distance)
            assert _same(after.boxes, boxes), (len(batch), _differing(after.boxes, boxes))
            assert not _same(after.boxes, before.boxes)
            assert _same(after.lights, before.lights)
            scenes.append(after)
            before = after
        if name == "mesh":
            assert np.abs(before.primitives["vt2"]).max() > 0 and np.abs(before.primitives["n1"]).max() > 0
    finally:
        k.finalize()
    for batch, mine, theirs in zip(batches, scenes, _scenes_by_setters(solr, name, batches)):
        _assert_same_scene(mine, theirs, "the setters one at a time, %d records" % len(batch))


def test_what_the_setters_derive_per_type(solr):
    """the mix has every type.  Without the normals flag: a sphere's, a cylinder's and a cone's size are size.x thrice, the
    rods' n1 is their axis and p2 their mid-point, the planes and the checkerboard have their axis for a normal, a triangle
    its face normal, an ellipsoid nothing.  A cylinder of zero length has no axis, a triangle with two equal vertices no face
    normal, and a zero normal given with the normals flag stays zero: normalizeVector leaves a zero vector alone"""
    solr_ = solr
    k = _kernel(solr, "mix")
    try:
        before = k.flat_scene()
        p = before.primitives
        kinds = (solr_.ptSphere, solr_.ptEllipsoid, solr_.ptCylinder, solr_.ptCone, solr_.ptTriangle, solr_.ptXYPlane,
                 solr_.ptYZPlane, solr_.ptXZPlane, solr_.ptCheckboard)
        first = {kind: int(np.flatnonzero((p["type"] == kind) & (np.arange(len(p)) >= before.nb_lamps))[0]) for kind in kinds}
        batch = edit_cases.records([edit_cases.record(p[first[kind]], seed=50 + n) for n, kind in enumerate(kinds)])
        assert not batch["flags"].any()
        assert k.set_primitives(batch) == 0
        after = k.flat_scene()
        want = edit_cases.edit_model(p, batch)
        assert _same(after.primitives, want), _differing(after.primitives, want)
        got = {kind: after.primitives[first[kind]] for kind in kinds}
        given = dict(zip(kinds, batch))
        for kind in (solr_.ptSphere, solr_.ptCylinder, solr_.ptCone):
            assert np.array_equal(got[kind]["size"], [given[kind]["size"][0]] * 3)
        assert np.array_equal(got[solr_.ptEllipsoid]["size"], given[solr_.ptEllipsoid]["size"])
        assert len(set(given[solr_.ptEllipsoid]["size"])) == 3
        for kind in (solr_.ptCylinder, solr_.ptCone):
            axis = (given[kind]["p1"] - given[kind]["p0"]).astype(np.float64)
            assert np.allclose(got[kind]["n1"], axis / np.linalg.norm(axis), atol=1e-6)
            assert np.allclose(got[kind]["p2"], (given[kind]["p0"] + given[kind]["p1"]) / 2, rtol=1e-6)
            assert not got[kind]["n0"].any() and not got[kind]["n2"].any()
        for kind, normal in ((solr_.ptXYPlane, (0, 0, 1)), (solr_.ptYZPlane, (1, 0, 0)), (solr_.ptXZPlane, (0, 1, 0)),
                             (solr_.ptCheckboard, (0, 1, 0))):
            for field in ("n0", "n1", "n2"):
                assert np.array_equal(got[kind][field], normal)
        t = given[solr_.ptTriangle]
        face = np.cross((t["p1"] - t["p0"]).astype(np.float64), (t["p2"] - t["p0"]).astype(np.float64))
        for field in ("n0", "n1", "n2"):
            assert np.allclose(got[solr_.ptTriangle][field], face / np.linalg.norm(face), atol=1e-5)
        for kind in kinds:
            assert not got[kind]["vt0"].any() and not got[kind]["vt1"].any() and not got[kind]["vt2"].any()

        # the degenerate ones
        rod, tri = batch[kinds.index(solr_.ptCylinder)].copy(), batch[kinds.index(solr_.ptTriangle)].copy()
        rod["p1"] = rod["p0"]
        tri["p1"] = tri["p0"]
        flat_normal = batch[kinds.index(solr_.ptTriangle)].copy()
        flat_normal["index"] = p["index"][np.flatnonzero(p["type"] == solr_.ptTriangle)[1]]
        flat_normal["materialId"] = p["materialId"][np.flatnonzero(p["type"] == solr_.ptTriangle)[1]]
        flat_normal["flags"] = solr_.EDIT_NORMALS
        flat_normal["n1"] = 0.0
        degenerate = edit_cases.records([rod, tri, flat_normal])
        assert k.set_primitives(degenerate) == 0
        last = k.flat_scene()
        want = edit_cases.edit_model(after.primitives, degenerate)
        assert _same(last.primitives, want), _differing(last.primitives, want)
        slot = {int(e["index"]): int(np.flatnonzero(p["index"] == e["index"])[0]) for e in degenerate}
        assert not last.primitives["n1"][slot[int(rod["index"])]].any()
        assert np.array_equal(last.primitives["p2"][slot[int(rod["index"])]], rod["p0"])
        for field in ("n0", "n1", "n2"):
            assert not last.primitives[field][slot[int(tri["index"])]].any()
        assert not last.primitives["n1"][slot[int(flat_normal["index"])]].any()
        assert abs(np.linalg.norm(last.primitives["n0"][slot[int(flat_normal["index"])]]) - 1.0) < 1e-6
        boxes = edit_cases.refit_model(after.boxes, want, k.info["viewDistance"])
        assert _same(last.boxes, boxes), _differing(last.boxes, boxes)
    finally:
        k.finalize()
    by_setters = _scenes_by_setters(solr, "mix", [batch, degenerate])
    _assert_same_scene(after, by_setters[0], "the setters one at a time")
    _assert_same_scene(last, by_setters[1], "the degenerate ones by the setters")


@pytest.mark.parametrize("engine", ["host-only", "host-replay"])
def test_an_unknown_index_refuses_the_batch(solr, engine):
    k = _kernel(solr, "sticks", engine)
    try:
        before = k.flat_scene()
        _frame(k)
        batch = edit_cases.batches(before, "sticks")[1][:5].copy()
        for unknown in (len(before.primitives), -1, 1 << 30):
            bad = batch.copy()
            bad["index"][3] = unknown
            assert k.set_primitives(bad) == -1
            assert k.pending_moves() == 0
            _assert_same_scene(k.flat_scene(), before, "index %d" % unknown)
        assert k.set_primitives(batch[:0]) == 0 and k.set_primitives([]) == 0      # nothing to do, nothing recorded
        assert k.pending_moves() == 0
        _assert_same_scene(k.flat_scene(), before)
        assert k.set_primitives(batch) == 0
        assert k.pending_moves() == (1 if engine == "host-replay" else 0)
        assert not _same(k.flat_scene().primitives, before.primitives)
    finally:
        k.finalize()


def test_a_list_of_dicts_is_the_same_batch(solr):
    k = _kernel(solr, "sticks")
    try:
        batch = edit_cases.batches(k.flat_scene(), "sticks")[1][:6]
        dicts = []
        for e in batch:
            d = dict(index=int(e["index"]), materialId=int(e["materialId"]), p0=tuple(e["p0"]), p1=tuple(e["p1"]),
                     p2=tuple(e["p2"]), size=tuple(e["size"]))
            if e["flags"] & solr.EDIT_NORMALS:
                d.update(n0=tuple(e["n0"]), n1=tuple(e["n1"]), n2=tuple(e["n2"]))
            if e["flags"] & solr.EDIT_TEXTURE_COORDINATES:
                d.update(vt0=tuple(e["vt0"]), vt1=tuple(e["vt1"]), vt2=tuple(e["vt2"]))
            dicts.append(d)
        assert len({int(f) for f in batch["flags"]}) >= 2
        assert k.set_primitives(batch) == 0
        from_records = k.flat_scene()
    finally:
        k.finalize()
    s = _kernel(solr, "sticks")
    try:
        assert s.set_primitives(dicts) == 0
        _assert_same_scene(from_records, s.flat_scene())
        with pytest.raises(solr.SolrError):
            s.set_primitives([dict(index=1, materialId=0, colour=3)])
        with pytest.raises(solr.SolrError):
            s.set_primitives(np.zeros(2, solr.PRIMITIVE_DTYPE))
    finally:
        s.finalize()


def test_lazy_replay_of_edits_among_the_other_moves_equals_the_eager_host_route(solr):
    """one journal, in order: batches of edits between a rotation, a lamp move and a translation; the store, once it looks,
    holds what the host route holds, field by field"""
    probe = _kernel(solr, "sticks")
    try:
        b = edit_cases.batches(probe.flat_scene(), "sticks")
    finally:
        probe.finalize()
    steps = [("edit", b[0]), ("rotate", TURNS[0]), ("lamp", (0, LAMP_THERE)), ("edit", b[1]), ("translate", TRANSLATION),
             ("edit", b[2]), ("rotate", TURNS[1])]
    lazy, eager = _lazy_and_eager(solr, "sticks", steps)
    _assert_same_scene(lazy, eager)
    assert np.array_equal(eager.lights["location"][0, :3], np.asarray(LAMP_THERE, f32))


def test_more_than_eight_rotations_with_edits_between_them_are_replayed(solr):
    """past eight rotations the store fetches the engine's primitives - which carry neither sizes nor texture coordinates: a
    journal that holds an edit is replayed whatever its length (the double hands nothing back either way; the engine's side
    of this is tests/test_edits_gpu.py's long sequence)"""
    probe = _kernel(solr, "mix")
    try:
        b = edit_cases.batches(probe.flat_scene(), "mix")
    finally:
        probe.finalize()
    steps = []
    for n in range(10):
        steps.append(("rotate", TURNS[n & 1]))
        if n in (2, 6):
            steps.append(("edit", b[1 + (n > 2)]))
    lazy, eager = _lazy_and_eager(solr, "mix", steps)
    _assert_same_scene(lazy, eager)


def test_an_edit_makes_the_unmovable_primitive_movable(solr):
    """setPrimitive sets movable: the one unmovable primitive of the mix, edited, follows the translation behind the edit -
    on the host route and in the replay alike"""
    probe = _kernel(solr, "mix")
    try:
        flat = probe.flat_scene()
    finally:
        probe.finalize()
    p = flat.primitives
    fixed = int(np.flatnonzero((p["type"] == solr.ptSphere) & (p["size"][:, 0] == 1300.0))[0])
    batch = edit_cases.records([edit_cases.record(p[fixed], seed=9, flags=solr.EDIT_TEXTURE_COORDINATES)])
    # without the edit the translation leaves it where it is
    still = _lazy_and_eager(solr, "mix", [("translate", TRANSLATION)])[1]
    assert np.array_equal(still.primitives["p0"][fixed], p["p0"][fixed])
    lazy, eager = _lazy_and_eager(solr, "mix", [("edit", batch), ("translate", TRANSLATION)])
    _assert_same_scene(lazy, eager)
    assert np.array_equal(eager.primitives["p0"][fixed], (batch["p0"][0] + np.asarray(TRANSLATION, f32)).astype(f32))


def test_a_duplicate_index_in_one_batch(solr):
    """several records for one index: the setters run in order, so the last one stands (setPrimitive resets everything a
    record can set); the journal keeps the batch as given"""
    probe = _kernel(solr, "sticks")
    try:
        flat = probe.flat_scene()
    finally:
        probe.finalize()
    p = flat.primitives
    a, b = flat.nb_lamps + 4, flat.nb_lamps + 9
    batch = edit_cases.records([edit_cases.record(p[a], seed=1, flags=3), edit_cases.record(p[b], seed=2),
                                edit_cases.record(p[a], seed=3, flags=0), edit_cases.record(p[b], seed=4, flags=2),
                                edit_cases.record(p[a], seed=5, flags=1)])
    lazy, eager = _lazy_and_eager(solr, "sticks", [("edit", batch), ("translate", TRANSLATION)])
    _assert_same_scene(lazy, eager)
    want = edit_cases.edit_model(p, batch)
    only_last = edit_cases.edit_model(p, batch[[3, 4]])
    assert _same(want, only_last)
    moved = move_cases.moved_by_a_translation(flat)
    assert _same(eager.primitives, move_cases.translation_model(want, moved, TRANSLATION))
    assert not eager.primitives["vt0"][a].any() and eager.primitives["vt0"][b].any()


def test_a_morph_behind_an_edit_takes_the_host_route(solr):
    """the blend on the device sets points, sizes and normals and leaves the texture coordinates and the movable flag as the
    edit set them, where morphPrimitives' loop takes the first key's: behind an edit over there the host serves the morph.
    An edit behind a pending morph is fine: the morph is replayed first"""
    probe = _kernel(solr, "mix")
    try:
        batch = edit_cases.batches(probe.flat_scene(), "mix")[2]
    finally:
        probe.finalize()
    k = _kernel(solr, "mix", engine="host-replay")
    try:
        _frame(k)
        assert k.morph_frame(0.25) == 0 and k.pending_morph()
        assert k.set_primitives(batch) == 0
        assert k.pending_moves() == 1 and k.pending_morph()        # (behind a morph: served over there)
        behind_a_morph = k.flat_scene()
        assert k.pending_moves() == 0 and not k.pending_morph()
        assert k.set_primitives(batch[:3]) == 0
        assert k.pending_moves() == 1
        assert k.morph_frame(0.75) == 0
        assert not k.pending_morph() and k.pending_moves() == 0, "the morph was served behind an edit"
        lazy = k.flat_scene()
        _frame(k)                                                  # uploaded again: morphs are served again
        assert k.morph_frame(0.25) == 0 and k.pending_morph()
    finally:
        k.finalize()
    h = _kernel(solr, "mix")
    try:
        assert h.morph_frame(0.25) == 0 and h.set_primitives(batch) == 0
        _assert_same_scene(behind_a_morph, h.flat_scene(), "an edit behind a morph")
        assert h.set_primitives(batch[:3]) == 0 and h.morph_frame(0.75) == 0
        _assert_same_scene(lazy, h.flat_scene(), "a morph behind an edit")
    finally:
        h.finalize()


def test_the_journals_batches_are_bounded(solr):
    """the journal keeps every batch as given; past ResidentScene::MAX_JOURNALLED_EDIT_RECORDS (2^20) records the store
    catches up before the next batch is offered - a replay, after which the batch is still served over there"""
    probe = _kernel(solr, "mesh")
    try:
        b = edit_cases.batches(probe.flat_scene(), "mesh")
    finally:
        probe.finalize()
    sequence, records = [], 0                        # batches of 289 and 257 records while they fit, and the one that does not
    while records <= 1 << 20:
        sequence.append(b[2 - (len(sequence) & 1)])
        records += len(sequence[-1])
    full = len(sequence) - 1
    k = _kernel(solr, "mesh", engine="host-replay")
    try:
        _frame(k)
        for batch in sequence[:full]:
            assert k.set_primitives(batch) == 0
        assert k.pending_moves() == full
        assert k.set_primitives(sequence[full]) == 0
        assert k.pending_moves() == 1, "the store did not catch up, or the batch behind it took the host route"
        k.translate_primitives(TRANSLATION)
        assert k.pending_moves() == 2
        lazy = k.flat_scene()
    finally:
        k.finalize()
    h = _kernel(solr, "mesh")
    try:
        for batch in sequence:
            assert h.set_primitives(batch) == 0
        h.translate_primitives(TRANSLATION)
        _assert_same_scene(lazy, h.flat_scene())
    finally:
        h.finalize()


def test_at_the_cap_an_edit_is_declined_not_counted(solr):
    """past ResidentScene::MAX_RECORDED_MOVES a rotation is counted and made up for by the engine's primitives; those could
    not restore an edit, so a journal never counts one - the edit takes the host route, which replays what is pending
    first - and never counts anything behind one either"""
    probe = _kernel(solr, "two_lamps")
    try:
        flat = probe.flat_scene()
        lamps = move_cases.lamp_indices(probe)
    finally:
        probe.finalize()
    assert flat.nb_lamps == 2
    slots = list(range(flat.nb_lamps, flat.nb_lamps + 9))
    batch = edit_cases.batch_of(flat, "sticks", slots, slots[0], seed=3)
    other = edit_cases.batch_of(flat, "sticks", slots[2:], slots[4], seed=4)
    k = _kernel(solr, "two_lamps", engine="host-replay")
    try:
        _frame(k)
        set_center = k.L.SolRx_SetPrimitiveCenter
        for n in range(MAX_RECORDED_MOVES):
            set_center(lamps[n & 1], 100.0, 9000.0, -7000.0 + (n & 7))
        assert k.pending_moves() == MAX_RECORDED_MOVES
        assert k.set_primitives(batch) == 0
        assert k.pending_moves() == 0, "an edit past the cap was counted"
        declined = k.flat_scene()
        _frame(k)
        assert k.set_primitives(other) == 0
        for n in range(MAX_RECORDED_MOVES - 1):
            set_center(lamps[n & 1], 100.0, 9000.0, -7000.0 + (n & 7))
        assert k.pending_moves() == MAX_RECORDED_MOVES
        k.rotate_primitives(*TURNS[1])
        assert k.pending_moves() == 0 and k.pending_rotations() == 0, "a move behind an edit was counted"
        behind = k.flat_scene()
    finally:
        k.finalize()
    h = _kernel(solr, "two_lamps")
    try:
        for n in (MAX_RECORDED_MOVES - 2, MAX_RECORDED_MOVES - 1):
            h.set_primitive_center(lamps[n & 1], (100.0, 9000.0, -7000.0 + (n & 7)))
        assert h.set_primitives(batch) == 0
        _assert_same_scene(declined, h.flat_scene(), "an edit at the cap")
        assert h.set_primitives(other) == 0
        for n in (MAX_RECORDED_MOVES - 3, MAX_RECORDED_MOVES - 2):
            h.set_primitive_center(lamps[n & 1], (100.0, 9000.0, -7000.0 + (n & 7)))
        h.rotate_primitives(*TURNS[1])
        _assert_same_scene(behind, h.flat_scene(), "a rotation at the cap behind an edit")
    finally:
        h.finalize()


@pytest.mark.parametrize("which", ["mesh", "sticks", "mix", "mixed", "long"])
def test_the_frames_held_to_the_oracle_do_not_rest_on_a_misrounded_power(solr, oracle, which):
    """tests/test_edits_gpu.py holds frames of these sequences to the oracle as pinned at 1 ULP.  The oracle as pinned calls
    libm's binary32 powf, sinf ..., the engine has correctly rounded ones, and where libm is off by an ULP or two the picture
    is (tests/helpers.py assert_parity_pinned counts such pixels; assert_parity cannot).  The batches' seeds (edit_cases.SEED)
    are chosen so that on every such frame both forms of the oracle agree within that ULP - held here, on the host route, so
    that a new seed or batch cannot quietly move a GPU test onto such a pixel; and the primitive every batch puts on the
    stage is in the picture"""
    from helpers import compare_frames, oracle_frame
    name = {"mixed": "sticks", "long": "mix"}.get(which, which)
    k = _kernel(solr, name)
    try:
        lamps = move_cases.lamp_indices(k)
        start = k.flat_scene()
        if which == "mixed":
            steps, checked = edit_cases.mixed_steps(start), edit_cases.MIXED_CHECKED
        elif which == "long":
            steps, checked = edit_cases.long_steps(start), edit_cases.LONG_CHECKED
        else:
            steps, checked = edit_cases.batch_steps(start, name), (0, 1, 2)
        _frame(k)                                    # (draws the random buffer)
        for n, step in enumerate(steps):
            edit_cases.apply(k, step, lamps)
            if n not in checked:
                continue
            pinned = oracle_frame(k, oracle)
            oracle.lib().oracle_set_rounded_transcendentals(1)
            try:
                rounded = oracle_frame(k, oracle)
            finally:
                oracle.lib().oracle_set_rounded_transcendentals(0)
            assert pinned[4] == 0 and rounded[4] == 0
            res = compare_frames(*pinned[:3], *rounded[:3])
            assert res["ids_all_equal"] and res["max_ulp"] <= 1 and res["rgb_max_diff"] == 0, (n, res)
            if step[0] == "edit":
                far = edit_cases.far_index(start, name, step[1])[0]
                assert (pinned[1][..., 0] == far).any(), "step %d: primitive %d is not in view" % (n, far)
    finally:
        k.finalize()


def test_the_records_size_is_the_headers(solr):
    assert solr.EDIT_DTYPE.itemsize == C.sizeof(solr.PrimitiveEdit) == solr.host_lib().SolRx_SizeofPrimitiveEdit() == 120
    for name in solr.EDIT_DTYPE.names:
        assert solr.EDIT_DTYPE.fields[name][1] == getattr(solr.PrimitiveEdit, name).offset, name
