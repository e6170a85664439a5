"""The frame bank on the host, no GPU: GPUKernel::setFrameBank (SolRx_SetFrameBank, Kernel.set_frame_bank) and the frame
switch behind setFrame - an animation of whole meshes, one per frame (scenes.animation, the reference's AnimationScene),
shown with set_frame + compact_boxes(False) per displayed frame (scenes.animation_step).

Held to: the rules of the switch - what is parked, what is resumed, what flattens and uploads again - through the
"host-replay" engine, the test double that claims every upload, park and resume for a device it does not have
(sol-r_amd/host/HipKernel.h ReplayKernel), and the flattened scene of every frame, bit for bit, against a kernel that never
heard of the bank and against the "host-only" engine.  The real engine's side is tests/test_frame_bank_gpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import morph_cases  # noqa: E402

K = 4
BANK = 1 << 30
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    """field by field: the structs carry padding that no one initialises"""
    return len(a) == len(b) and all(
        np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8))
        for f in a.dtype.names)


def _same_scene(a, b):
    return _same(a.boxes, b.boxes) and _same(a.primitives, b.primitives) and _same(a.lights, b.lights) and a.nb_lamps == b.nb_lamps


def _frame(k):
    """one frame of the frame protocol; without a device it renders nothing and says so"""
    k.L.SolRx_Render(0.0)


def _animation(solr, engine="host-replay", bank=None):
    k = solr.Kernel(engine=engine, deterministic_seed=1)
    solr.scenes.animation(k, frames=K)
    if bank is not None:
        k.set_frame_bank(bank)
    return k


def _lap(solr, k, first):
    """K displayed frames; per frame its flattened scene and what the counters grew by"""
    scenes, uploads, switches = [], [], []
    for i in range(first, first + K):
        before = (k.scene_uploads(), k.frame_switches())
        assert solr.scenes.animation_step(k, i) == i % K
        _frame(k)
        scenes.append(k.flat_scene())
        uploads.append(k.scene_uploads() - before[0])
        switches.append(k.frame_switches() - before[1])
    return scenes, uploads, switches


def test_the_frames_are_meshes_of_their_own(solr):
    k = _animation(solr)
    try:
        counts = []
        for i in range(K):
            solr.scenes.animation_step(k, i)
            counts.append(len(k.flat_scene().primitives))
        assert counts == k.animation["counts"] and len(set(counts)) == K
    finally:
        k.finalize()


@pytest.mark.parametrize("bank", [None, 0])
def test_bank_off_uploads_every_displayed_frame(solr, bank):
    k = _animation(solr, bank=bank)
    try:
        for lap in range(2):
            _, uploads, switches = _lap(solr, k, lap * K)
            assert uploads == [1] * K and switches == [0] * K
            assert k.parked_frames() == 0
        assert k.scene_uploads() == 2 * K and k.frame_switches() == 0
    finally:
        k.finalize()


def test_bank_on_the_second_lap_uploads_nothing(solr):
    plain = _animation(solr)                            # (one kernel at a time: the kernel is the process's)
    try:
        reference, _, _ = _lap(solr, plain, 0)
    finally:
        plain.finalize()
    k = _animation(solr, bank=BANK)
    try:
        first, uploads, switches = _lap(solr, k, 0)
        assert uploads == [1] * K and switches == [0] * K
        assert k.parked_frames() == K - 1               # every frame but the current one
        second, uploads, switches = _lap(solr, k, K)
        assert uploads == [0] * K and switches == [1] * K
        assert k.scene_uploads() == K and k.frame_switches() == K and k.parked_frames() == K - 1
        for f in range(K):
            assert len(second[f].primitives) == k.animation["counts"][f]
            assert _same_scene(second[f], first[f]), f
            assert _same_scene(second[f], reference[f]), f
    finally:
        k.finalize()


def test_the_bank_turned_off_again_is_the_route_of_before(solr):
    k = _animation(solr, bank=BANK)
    try:
        first, _, _ = _lap(solr, k, 0)
        _lap(solr, k, K)
        k.set_frame_bank(0)                             # frame K - 1 is current, resumed and resident
        assert k.parked_frames() == 0
        for lap in (2, 3):
            scenes, uploads, switches = _lap(solr, k, lap * K)
            assert uploads == [1] * K and switches == [0] * K and k.parked_frames() == 0
            for f in range(K):
                assert _same_scene(scenes[f], first[f]), (lap, f)
    finally:
        k.finalize()


def test_a_frame_entered_without_a_flatten_is_flattened_by_its_first_render(solr):
    """the flattened arrays went into the bank with the frame that was left; a host that renders the frame it entered without
    compact_boxes(False) gets that frame, flattened by the frame protocol, not arrays that are no longer there"""
    plain = _animation(solr)
    try:
        reference, _, _ = _lap(solr, plain, 0)
    finally:
        plain.finalize()
    k = _animation(solr, bank=BANK)
    try:
        solr.scenes.animation_step(k, 0)
        _frame(k)
        k.set_frame(1)                                  # parks frame 0; frame 1 has never been uploaded
        assert k.parked_frames() == 1
        _frame(k)
        assert k.scene_uploads() == 2 and k.frame_switches() == 0
        assert _same_scene(k.flat_scene(), reference[1])
        k.set_frame(0)                                  # ... and frame 0 comes back as it was
        _frame(k)
        assert k.scene_uploads() == 2 and k.frame_switches() == 1
        assert _same_scene(k.flat_scene(), reference[0])
    finally:
        k.finalize()


def _red_lamp(solr, k):
    """the lamp's material set anew, red: the light records of a flattened frame carry its colour"""
    vd = k.info["viewDistance"]
    k.L.SolR_SetMaterial(k.animation["lamp_material"], 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0.0, 0.0, solr.TEXTURE_NONE,
                         solr.TEXTURE_NONE, solr.TEXTURE_NONE, solr.TEXTURE_NONE, solr.TEXTURE_NONE, solr.TEXTURE_NONE,
                         solr.TEXTURE_NONE, 0.1, 200.0, 0.0, 2.0, vd * 10, vd, 0)


def _after_a_material_change(solr, bank, order):
    """two laps, the lamp recoloured while frame 1 is current - behind its frame ("rendered") or between its set_frame and
    its compact_boxes(False) ("entered") -, then two laps more: the lights of every displayed frame, and the uploads"""
    k = _animation(solr, bank=bank)
    try:
        _lap(solr, k, 0)
        _lap(solr, k, K)
        solr.scenes.animation_step(k, 0)
        _frame(k)
        if order == "rendered":
            solr.scenes.animation_step(k, 1)
            _frame(k)
            _red_lamp(solr, k)
        else:
            k.set_frame(1)
            _red_lamp(solr, k)
            k.compact_boxes(False)
            _frame(k)
        before = k.scene_uploads()
        scenes = [k.flat_scene()]
        for lap in (3, 4):
            for i in range(2 if lap == 3 else 0, K):
                solr.scenes.animation_step(k, lap * K + i)
                _frame(k)
                scenes.append(k.flat_scene())
        last, uploads, _ = _lap(solr, k, 5 * K)
        return scenes + last, k.scene_uploads() - before, uploads
    finally:
        k.finalize()


@pytest.mark.parametrize("order", ["rendered", "entered"])
def test_a_material_change_reaches_every_frame_s_light_records(solr, order):
    """a frame flattened under the table before is neither parked nor taken as resumed: it is flattened and uploaded again,
    once, and resumes from then on"""
    plain, _, _ = _after_a_material_change(solr, None, order)
    banked, uploads, last_lap = _after_a_material_change(solr, BANK, order)
    assert len(plain) == len(banked) == 1 + 2 + K + K
    for n, (a, b) in enumerate(zip(plain, banked)):
        if n > 0 or order == "entered":                 # ("rendered": the frame before the change shows the old lamp on both)
            assert tuple(a.lights["color"][0]) == (1.0, 0.0, 0.0, 2.0), n
        assert _same_scene(a, b), "displayed frame %d behind the change: the banked kernel's lights %s" % (n, b.lights["color"][0])
    assert last_lap == [0] * K, "a frame goes on being uploaded after every frame was flattened under the new table"
    assert uploads <= K + 1


def test_fewer_frames_and_reset_all_drop_what_is_parked(solr):
    k = _animation(solr, bank=BANK)
    try:
        first, _, _ = _lap(solr, k, 0)
        solr.scenes.animation_step(k, 0)
        _frame(k)
        assert k.parked_frames() == K - 1               # 1, 2, 3
        k.set_nb_frames(K - 1)                          # frame 3 is no frame any more
        assert k.parked_frames() == K - 2
        k.set_nb_frames(K)
        uploads, switches = k.scene_uploads(), k.frame_switches()
        solr.scenes.animation_step(k, 3)                # ... so it is flattened and uploaded again, and is what it was
        _frame(k)
        assert (k.scene_uploads() - uploads, k.frame_switches() - switches) == (1, 0)
        assert _same_scene(k.flat_scene(), first[3])
        solr.scenes.animation_step(k, 2)                # the others were kept
        _frame(k)
        assert (k.scene_uploads() - uploads, k.frame_switches() - switches) == (1, 1)
        assert k.parked_frames() == K - 1
        k.L.SolR_ResetKernel()                          # resetAll: every frame is emptied, nothing parked describes one
        assert k.parked_frames() == 0
        k.set_frame(1)
        assert k.frame_switches() - switches == 1 and k.parked_frames() == 0
    finally:
        k.finalize()


def test_a_store_access_while_current_uploads_that_frame_again(solr):
    k = _animation(solr, bank=BANK)
    try:
        first, _, _ = _lap(solr, k, 0)
        solr.scenes.animation_step(k, 1)
        _frame(k)
        p = first[1].primitives[first[1].primitives["type"] == solr.ptTriangle][0]
        moved = (float(p["p0"][0]) + 125.0, float(p["p0"][1]), float(p["p0"][2]))
        k.L.SolR_SetPrimitive(int(p["index"]), *moved, *map(float, p["p1"]), *map(float, p["p2"]), 0.0, 0.0, 0.0,
                              int(p["materialId"]))
        solr.scenes.animation_step(k, 2)                # frame 1 was touched: not parked
        _frame(k)
        assert k.parked_frames() == K - 2
        uploads, switches = k.scene_uploads(), k.frame_switches()
        solr.scenes.animation_step(k, 1)                # flattened and uploaded again, with the change in it
        _frame(k)
        assert (k.scene_uploads() - uploads, k.frame_switches() - switches) == (1, 0)
        again = k.flat_scene()
        at = np.flatnonzero(again.primitives["index"] == p["index"])
        assert len(at) == 1 and again.primitives["p0"][at[0]][0] == np.float32(moved[0])
        assert not _same(again.primitives, first[1].primitives)
        for f in (2, 3, 0):                             # the others still resume
            uploads, switches = k.scene_uploads(), k.frame_switches()
            solr.scenes.animation_step(k, f)
            _frame(k)
            assert (k.scene_uploads() - uploads, k.frame_switches() - switches) == (0, 1), f
            assert _same_scene(k.flat_scene(), first[f]), f
    finally:
        k.finalize()


def test_a_move_on_a_resumed_frame_is_served_and_synced_before_the_switch(solr):
    turn = ((0.0, 0.0, 0.0), (0.0, 0.05, 0.0))
    eager = _animation(solr, engine="host-only")
    try:
        solr.scenes.animation_step(eager, 1)
        eager.rotate_primitives(*turn)
        want = eager.flat_scene()
    finally:
        eager.finalize()
    k = _animation(solr, bank=BANK)
    try:
        _lap(solr, k, 0)
        solr.scenes.animation_step(k, 1)                # resumed
        _frame(k)
        switches = k.frame_switches()
        k.rotate_primitives(*turn)
        assert k.pending_moves() == 1, "the rotation took the host route on a resumed frame"
        assert k.compact_boxes(False) > 0
        _frame(k)
        solr.scenes.animation_step(k, 2)                # switching away syncs the store first
        assert k.pending_moves() == 0
        _frame(k)
        uploads = k.scene_uploads()
        solr.scenes.animation_step(k, 1)                # ... and the synced frame was parked: it resumes
        _frame(k)
        assert k.scene_uploads() == uploads and k.frame_switches() == switches + 2
        assert _same_scene(k.flat_scene(), want)
    finally:
        k.finalize()


def _morph_stage(solr, engine, bank):
    k = morph_cases.build(solr.Kernel(engine=engine, deterministic_seed=1), "mesh")
    if bank:
        k.set_frame_bank(bank)
    k.set_frame(0)                                      # key frame 0 rendered - and, with the bank, parked by the switch
    k.compact_boxes(False)
    _frame(k)
    k.set_frame(1)
    k.compact_boxes(False)
    _frame(k)
    return k


def test_morph_between_reads_a_parked_key_frame(solr):
    eager = _morph_stage(solr, "host-only", 0)
    try:
        assert eager.morph_between(0, 2, 0.3) == 0 and not eager.pending_morph()
        want = eager.flat_scene()
    finally:
        eager.finalize()
    k = _morph_stage(solr, "host-replay", BANK)
    try:
        assert k.parked_frames() == 1
        assert k.morph_between(0, 2, 0.3) == 0
        assert k.pending_morph(), "the morph took the host route"
        assert _same_scene(k.flat_scene(), want)
        assert k.parked_frames() == 1
    finally:
        k.finalize()


def test_host_only_engine_keeps_nothing(solr):
    scenes = []
    for bank in (None, BANK):
        k = _animation(solr, engine="host-only", bank=bank)
        try:
            laps = []
            for i in range(2 * K):
                solr.scenes.animation_step(k, i)
                _frame(k)
                laps.append(k.flat_scene())
                assert (k.parked_frames(), k.frame_switches(), k.scene_uploads()) == (0, 0, 0)
            scenes.append(laps)
        finally:
            k.finalize()
    for i in range(2 * K):
        assert _same_scene(scenes[0][i], scenes[1][i]), i


ENGINE_SYMBOLS = ["solr_hip_park_scene", "solr_hip_resume_scene", "solr_hip_drop_parked_scenes", "solr_hip_set_scene_bank_bytes",
                  "solr_hip_parked_scenes", "solr_hip_parked_bytes", "solr_hip_scene_switches", "solr_hip_scene_uploads"]
HOST_SYMBOLS = ["SolRx_SetFrameBank", "SolRx_ParkedFrames", "SolRx_FrameSwitches", "SolRx_SceneUploads"]


def test_the_new_symbols_are_exported_and_declared(solr):
    for library, header, names in ((solr.HIP_LIB, os.path.join(ROOT, "include", "solr_hip.h"), ENGINE_SYMBOLS),
                                   (solr.HOST_LIB, os.path.join(ROOT, "sol-r_amd", "host", "SolRStub.h"), HOST_SYMBOLS)):
        with open(library, "rb") as f:
            binary = f.read()
        with open(header) as f:
            text = f.read()
        for name in names:
            assert b"\0" + name.encode() + b"\0" in binary, (library, name)
            assert name + "(" in text, (header, name)
    for name in ("set_frame_bank", "parked_frames", "frame_switches", "scene_uploads"):
        assert callable(getattr(solr.Kernel, name))
