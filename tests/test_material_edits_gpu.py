"""Materials edited under the resident scene: with Kernel.set_material_edits(True) the HIP engine follows a SolR_SetMaterial
between two frames in place (solr_hip_edit_materials: sol-r_amd/csrc/solr_materials.hip) - the changed records overwritten in
its table, one lane per primitive rewriting tag and colour key where the primitive has a changed material (k_retagMaterials),
the leaf records behind - where the table upload it replaces (h2d_materials) retags every primitive on the host and has the
whole arena laid out and uploaded again.

The bar: a kernel with the switch on and a kernel with it off run the same steps, and after every frame what the device
holds is compared BIT FOR BIT - the primitive rows, the light rows, the node rows, thin copies, sorted copies, leaf records and
start indices of every list the engine holds (walk, exact, order-free) - and so is the rendered frame: no tolerance, nothing
left out.  Per frame the three words of every primitive are held to the numpy model of the tags (tests/material_edit_cases.py),
solr_hip_device_material_edits advances exactly when the case says the engine has to serve,
solr_hip_device_material_retags exactly when the model says a tag or a colour key changes, no scene is uploaded on either
route, and a request the engine declines changes nothing before the upload that serves it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_cases  # noqa: E402
import engine_probes  # noqa: E402
import material_edit_cases as cases  # noqa: E402
import move_cases  # noqa: E402
from helpers import copy_frame, gpu_frame, same_frames  # noqa: E402

pytestmark = pytest.mark.gpu

LISTS = (engine_probes.WALK_LIST, engine_probes.EXACT_LIST, engine_probes.FREE_LISTS)
COPIES = (engine_probes.NODE_ROWS, engine_probes.THIN_COPY, engine_probes.SORTED_COPY, engine_probes.LEAF_RECORDS,
          engine_probes.START_INDICES)
SETTLE = 3      # frames after an upload until the order-free lists are built and in the arena
BANK = 1 << 28


def _same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _snapshot(k, hip):
    """what the device holds now: primitive rows, light rows, every copy of every list"""
    out = {"primitives": k.device_primitives().copy(), "lights": k.device_lights().copy()}
    for which in LISTS:
        for what in COPIES:
            out["copy %d of list %d" % (what, which)] = engine_probes.list_copy(hip, which, what)
    return out


def _assert_same_snapshot(a, b, what):
    assert a.keys() == b.keys()
    for part in a:
        assert _same_bits(a[part], b[part]), "%s: the %s differ" % (what, part)


def _settle(k):
    for _ in range(SETTLE - 1):
        gpu_frame(k)
    return copy_frame(gpu_frame(k))


def _counters(k, hip):
    return hip.solr_hip_device_material_edits(), hip.solr_hip_device_material_retags(), k.material_edits()


def _assert_words(rows, flat, table, what):
    """tag, material id and colour key of every primitive row against the model under that table"""
    got = np.stack([rows[:, 0, 3], rows[:, 1, 3], rows[:, 3, 3]], axis=1).view(np.int32)
    model = cases.three_words_model(flat, table)
    wrong = np.flatnonzero((got != model).any(axis=1))
    assert wrong.size == 0, "%s: slots %s, e.g. %s for %s" % (what, wrong[:8], got[wrong[0]], model[wrong[0]])


def _route(solr, case, on, flights=1, before=None, bank=False, between=None):
    """the case's frames on a kernel with the switch on or off: per frame (rendered frame, snapshot); on the switched-on
    kernel a frame the engine has to decline is also put to the engine directly, which must change nothing.
    before(k, lamps): moves made on the settled scene in front of the first frame; between(k, n): called in front of frame n"""
    hip = solr.hip_lib()
    k = cases.build_case(solr.Kernel(engine="hip", deterministic_seed=1), case)
    try:
        hip.solr_hip_set_frames_in_flight(flights)
        if bank:
            k.set_frame_bank(BANK)
        if on is not None:
            assert k.set_material_edits(on) == 0
        lamps = move_cases.lamp_indices(k)
        flat = k.flat_scene()
        frames = case["frames"](k, flat)
        _settle(k)
        pending = 0
        if before is not None:
            pending = before(k, lamps)
            assert k.pending_moves() == pending, "the moves took the host route"
        out = []
        for n, (frame, expect) in enumerate(zip(frames, case["expect"])):
            what = "frame %d (%s)" % (n, expect)
            if between is not None:
                between(k, n)
            counters, uploads = _counters(k, hip), k.scene_uploads()
            table = cases.materials_of(k)
            for step in frame:
                cases.apply(k, step)
            after = cases.materials_of(k)
            if on and expect != "served":
                held = _snapshot(k, hip)
                assert hip.solr_hip_edit_materials(*cases.table_pointer(k)) == 0, what + ": the engine served it"
                _assert_same_snapshot(_snapshot(k, hip), held, what + ", declined")
                assert _counters(k, hip) == counters
                k.check(0, what + ": a refusal is not an error")
            picture = copy_frame(gpu_frame(k))
            snapshot = _snapshot(k, hip)
            served = bool(on) and expect == "served"
            retagged = served and cases.retags_model(table, after)
            assert _counters(k, hip) == (counters[0] + served, counters[1] + retagged, counters[2] + served), what
            assert k.scene_uploads() == uploads, what + ": the scene was uploaded"
            assert k.pending_moves() == pending, what
            if before is None:       # (moved primitives keep their words; their rows are compared with the other route's)
                _assert_words(snapshot["primitives"], flat, after, what)
            out.append((picture, snapshot))
        k.check(0, "the frames")
        return out
    finally:
        hip.solr_hip_set_frames_in_flight(1)
        k.finalize()


def _both_routes(solr, case, **how):
    mine = _route(solr, case, True, **how)
    theirs = _route(solr, case, False, **how)
    assert len(mine) == len(theirs) == len(case["expect"])
    for n, ((picture, snapshot), (their_picture, their_snapshot)) in enumerate(zip(mine, theirs)):
        _assert_same_snapshot(snapshot, their_snapshot, "after frame %d" % n)
        assert same_frames(picture, their_picture), "after frame %d: the rendered frames differ" % n
    return mine


@pytest.mark.parametrize("name", sorted(cases.SERVED))
def test_a_served_edit_leaves_what_the_table_upload_leaves(solr, name):
    mine = _both_routes(solr, cases.SERVED[name])
    if name == "colour_of_the_most_used":
        # more than one workgroup of k_retagMaterials, the last wave partly idle, and order-free lists whose leaf records follow
        n = len(mine[0][1]["primitives"])
        assert n > 256 and n % 64 != 0
        assert mine[0][1]["copy %d of list %d" % (engine_probes.LEAF_RECORDS, engine_probes.FREE_LISTS)] is not None
    if name in ("colour_of_the_most_used", "transparent_and_back", "texture_swapped"):
        assert not same_frames(mine[0][0], mine[1][0]), "the second edit changed nothing in the picture"


@pytest.mark.parametrize("name", sorted(cases.DECLINED))
def test_a_declined_edit_changes_nothing_and_the_upload_serves_it(solr, name):
    _both_routes(solr, cases.DECLINED[name])


def test_the_switch_is_off_by_default(solr):
    """the counters stay where they are and the frames are those of a kernel that was told to leave it off"""
    case = cases.SERVED["transparent_and_back"]
    untold = _route(solr, case, None)
    off = _route(solr, case, False)
    for (picture, snapshot), (their_picture, their_snapshot) in zip(untold, off):
        _assert_same_snapshot(snapshot, their_snapshot, "switch never set")
        assert same_frames(picture, their_picture)


def test_the_served_route_uploads_nothing_where_the_other_lays_the_arena_out_again(solr, capfd, monkeypatch):
    """the two routes really differ: the engine reports every layout and upload of the arena under SOLR_HIP_DEBUG_TIMING
    (flushGeometry's "geometry: upload"), and the order-free lists stay in use behind the served edit"""
    monkeypatch.setenv("SOLR_HIP_DEBUG_TIMING", "1")
    hip = solr.hip_lib()
    case = cases.SERVED["colour_of_the_most_used"]
    for on in (True, False):
        k = cases.build_case(solr.Kernel(engine="hip", deterministic_seed=1), case)
        try:
            k.set_material_edits(on)
            frames = case["frames"](k, k.flat_scene())
            _settle(k)
            assert "geometry: upload" in capfd.readouterr().err         # (the scene's own upload: the report works)
            lists = hip.solr_hip_order_free_nodes()
            assert lists > 0
            for frame in frames:
                for step in frame:
                    cases.apply(k, step)
                gpu_frame(k)
                report = capfd.readouterr().err
                assert ("geometry: upload" in report) == (not on), report
                assert hip.solr_hip_order_free_nodes() == lists
            assert hip.solr_hip_device_material_edits() == (len(frames) if on else 0)
            k.check(0, "the frames")
        finally:
            k.finalize()


def test_an_edit_behind_a_rotation_and_a_translation_on_the_device(solr):
    """the served route pulls nothing: the moves stay pending for the host store, and the rows are the other route's, which
    pulled the geometry, retagged it and uploaded it again.  The mesh stands in front of an axis plane, so its lists have thin
    copies, whose margin the upload takes from the extent of the moved scene: the engine declines that edit, the upload
    serves it - and pulls -, and the edit behind it is followed in place again"""
    def moves(k, lamps):
        edit_cases.apply(k, ("rotate", edit_cases.TURNS[1]), lamps)
        edit_cases.apply(k, ("translate", edit_cases.TRANSLATIONS[0]), lamps)
        return 2
    _both_routes(solr, cases.SERVED["transparent_and_back"], before=moves)
    mesh = dict(cases.SERVED["colour_of_the_most_used"], expect=["moved", "served"])
    mine = _both_routes(solr, mesh, before=moves)
    assert mine[0][1]["copy %d of list %d" % (engine_probes.THIN_COPY, engine_probes.WALK_LIST)] is not None


def test_an_edit_behind_a_served_batch_of_material_sets(solr):
    """setPrimitiveMaterialsOne keeps the host image current: the census of an edit counts the primitives as they are now"""
    hip = solr.hip_lib()

    def moves(k, lamps):
        flat = k.flat_scene()
        spheres = [cases.sets.first_of_type(flat, cases.solr.ptSphere, n) for n in (1, 3, 4)]
        assert not set(int(m) for m in flat.primitives["materialId"][cases.sets.slots_of(flat, spheres)]) & {2}
        served = hip.solr_hip_device_material_sets()
        assert k.set_primitive_materials(spheres, [2, 2, k.extra["plain"]]) == 0
        assert hip.solr_hip_device_material_sets() == served + 1, "the batch took the host route"
        return 1
    _both_routes(solr, cases.SERVED["transparent_and_back"], before=moves)


@pytest.mark.parametrize("flights", [2, 3])
def test_edits_with_frames_in_flight(solr, flights):
    _both_routes(solr, cases.SERVED["transparent_and_back"], flights=flights)
    _both_routes(solr, cases.DECLINED["table_grown"], flights=flights)


def test_an_edit_while_another_frame_is_parked(solr):
    """with the frame bank on: frame 1 is set aside, a material is edited under frame 0, and frame 1 comes back under the new
    table - the same rows and the same picture as on a kernel without the bank, with the switch on as with it off"""
    case = cases.SERVED["transparent_and_back"]

    def run(on, bank):
        hip = solr.hip_lib()
        k = cases.build_case(solr.Kernel(engine="hip", deterministic_seed=1), case)
        try:
            if bank:
                k.set_frame_bank(BANK)
            k.set_material_edits(on)
            k.compact_boxes(False)      # (flattened under the table as it is: the three materials came after the build's)
            _settle(k)
            out = []
            k.set_frame(0)
            k.compact_boxes(False)
            _settle(k)
            assert k.parked_frames() == (1 if bank else 0)
            edits = hip.solr_hip_device_material_edits()
            cases.apply(k, ("edit", 2, dict(transparency=0.5, refraction=1.1, opacity=0.1)))
            out.append((copy_frame(gpu_frame(k)), _snapshot(k, hip)))
            assert hip.solr_hip_device_material_edits() == edits + (1 if on else 0)
            k.set_frame(1)
            k.compact_boxes(False)
            out.append((_settle(k), _snapshot(k, hip)))
            rows = out[-1][1]["primitives"]
            _assert_words(rows, k.flat_scene(), cases.materials_of(k), "frame 1 under the new table")
            k.check(0, "the frames")
            return out
        finally:
            k.finalize()

    plain = run(False, False)
    for on, bank in ((True, True), (False, True), (True, False)):
        got = run(on, bank)
        for n, ((picture, snapshot), (their_picture, their_snapshot)) in enumerate(zip(got, plain)):
            _assert_same_snapshot(snapshot, their_snapshot, "switch %s, bank %s, stage %d" % (on, bank, n))
            assert same_frames(picture, their_picture), "switch %s, bank %s, stage %d" % (on, bank, n)


def test_a_parked_scene_is_retagged_at_its_resume(solr):
    """engine level, the bank driven under the host's feet: frame 1 parked under the old table; with no scene resident an edit
    is declined; with frame 0 resident it is served, which moves the table's generation on - and the parked scene comes back
    with the tags and colour keys of the table as it is now"""
    hip = solr.hip_lib()
    case = cases.SERVED["transparent_and_back"]
    k = cases.build_case(solr.Kernel(engine="hip", deterministic_seed=1), case)
    try:
        k.set_material_edits(True)
        flat = k.flat_scene()
        _settle(k)
        hip.solr_hip_set_scene_bank_bytes(BANK)
        assert hip.solr_hip_park_scene(7) == 1
        counters = _counters(k, hip)
        assert hip.solr_hip_edit_materials(*cases.table_pointer(k)) == 0, "served without a resident scene"
        assert _counters(k, hip) == counters
        k.set_frame(0)
        k.compact_boxes(False)
        _settle(k)
        cases.apply(k, ("edit", 2, dict(transparency=0.5, refraction=1.1, opacity=0.1)))
        gpu_frame(k)
        assert _counters(k, hip) == (counters[0] + 1, counters[1] + 1, counters[2] + 1)
        assert hip.solr_hip_resume_scene(7) == 1
        _assert_words(k.device_primitives(), flat, cases.materials_of(k), "resumed under the new table")
        k.check(0, "park, edit, resume")
    finally:
        hip.solr_hip_drop_parked_scenes(-1)
        hip.solr_hip_set_scene_bank_bytes(0)
        k.finalize()
