"""The modes of the F_FULL rows (renderer.h ROWS: the five-ray, anaglyph, fish-eye and 3D-vision cameras, global
illumination, the box-debug view) and fog, the gradient background and random illumination, on every kind of scene
(tests/mode_content_cases.py): triangles, cylinders, ellipsoids, cones, glass, wireframe and noisy materials, textures, a
plain-coloured skybox, and scenes that are open - in which primary rays and the global-illumination ray of phase 2 miss,
so that the sky, gradient and background arms of launchRayTracing's tail run (rt_device.h; CRT:271-286, 363-375).

Every pass of every case is the engine's frame against the oracle AS PINNED over the engine's own previous buffers
(helpers.assert_frame_pinned for pass 0, assert_pass_parity afterwards): ids and depth exact; on every pixel the oracle
did not mark, RGB8 exact and float colour and last sample within 1 ULP; every pixel outside that bar marked by the oracle
as behind a mis-rounded libm result, and at most 2 ULP and one RGB8 step off.  As many pixels may be outside the bar as
the oracle marked in that pass: tests/test_mode_content_cases.py caps that number at 2 % of the frame on the CPU.

solr_hip_probe_last_frame says which row ran: a scene that stops reaching the row it is here for fails."""
import ctypes as C

import pytest

import engine_probes as E
import mode_content_cases as MC
from helpers import copy_frame, gpu_frame, render_passes, same_frames

pytestmark = pytest.mark.gpu

F_TEX, F_FULL = 64, 128     # rt_device.h enum Feature
ALL_TRIPS = 16              # include/solr_hip.h solr_hip_set_variant
# The row a scene reaches (the features of its instantiation, F_DEEP and beyond masked off), renderer.h ROWS:
# without F_FULL - 127 every type + textures, 117 the textured mix, 17 spheres + triangles, 5 spheres + cylinders,
# 53 the untextured mix (open_sky: spheres, a plane and a cone, which walks as a cylinder), 33 spheres + planes
OWN_ROW = {"mix_plain": 127, "tex_flat": 117, "triangles": 17, "sticks": 5, "open_sky": 53, "open_room": 33}
# with F_FULL - 255 everything (ellipsoids, or textures), 181 the special cameras over the usual untextured primitives
FULL_ROW = {"mix_plain": 255, "tex_flat": 255, "triangles": 181, "sticks": 181, "open_sky": 181, "open_room": 181}
OPEN_SCENES = ("open_sky", "open_room", "triangles", "sticks")


def _mask(solr):
    hip = solr.hip_lib()
    E.declare(hip)
    out = (C.c_int * 6)()
    hip.solr_hip_probe_last_frame(out)
    return out[1] & 255


@pytest.mark.parametrize("case", MC.CASES, ids=MC.case_id)
def test_case(solr, oracle, case):
    scene, mode = case
    k = solr.Kernel(engine="hip")
    masks = []
    try:
        passes = MC.build(k, case)
        _, figures = render_passes(k, oracle, passes, max_exceptions=None, after_pass=lambda it: masks.append(_mask(solr)))
    finally:
        k.finalize()
    print("%s: mask %d; per pass %s: marked %s, outside the bar %s" % (
        MC.case_id(case), masks[0], list(passes), [f["pixels_with_a_misrounded_libm_result"] for f in figures],
        [f["pixels_outside_the_bar"] for f in figures]))
    assert all(f["pixels_with_a_misrounded_libm_result"] <= MC.MARKED_CAP for f in figures)
    mask = masks[0]
    assert bool(mask & F_FULL) == (mode in MC.FULL_MODES), mask
    assert scene != "tex_flat" or mask & F_TEX, mask
    assert mask == (FULL_ROW if mode in MC.FULL_MODES else OWN_ROW)[scene], mask
    assert set(masks) == {mask}, masks          # every pass of a case takes the same row


@pytest.mark.parametrize("case", [c for c in MC.CASES if c[1] in MC.GI_MODES and c[0] in OPEN_SCENES], ids=MC.case_id)
def test_the_same_frames_with_every_trip_made(solr, case):
    """solr_hip_set_variant(16) makes the trips that no lane takes: the edge into phase 2 whose tail shades the sky for
    the lanes that did not hit, in scenes in which lanes do not hit"""
    hip = solr.hip_lib()
    got = {}
    try:
        for variant in (0, ALL_TRIPS):
            hip.solr_hip_set_variant(variant)
            k = solr.Kernel(engine="hip")
            try:
                frames = []
                for it in MC.build(k, case):
                    k.set_scene_info(pathTracingIteration=it)
                    frames.append(copy_frame(gpu_frame(k)))
                k.check(0, "render")
                assert hip.solr_hip_get_variant() == variant
            finally:
                k.finalize()
            got[variant] = frames
    finally:
        hip.solr_hip_set_variant(0)
    assert len(got[0]) == len(got[ALL_TRIPS]) == len(MC.passes_of(case))
    for n, (a, b) in enumerate(zip(got[0], got[ALL_TRIPS])):
        assert same_frames(a, b), "frame %d differs with and without the skipped trips" % n
    assert (got[0][0][1][..., 0] < 0).any() and got[0][-1][2].any()


def test_both_full_rows_were_seen(solr):
    """the special-cameras row and the everything row both run in this module.  Every case above asserts its own mask
    against FULL_ROW; this test stands alone (it keeps nothing from them): it renders the box view, the shortest F_FULL
    case, once per scene and collects the rows that ran."""
    seen = set()
    for scene in MC.SCENES:
        k = solr.Kernel(engine="hip")
        try:
            MC.build(k, (scene, "boxes"))
            k.set_scene_info(pathTracingIteration=0)
            k.render()
            seen.add(_mask(solr))
        finally:
            k.finalize()
    assert seen == {181, 255} == set(FULL_ROW.values()), sorted(seen)
