"""The cases of tests/mode_content_cases.py themselves, without a GPU: every case through the host-only kernel and the
oracle as pinned, pass after pass over the oracle's own previous buffers.  What tests/test_mode_content_gpu.py rests on is
asserted here, so that it cannot erode unseen: the oracle never reads outside its random buffer, it marks few pixels of
any pass (the GPU test allows an engine frame as many pixels outside the bar as the oracle marked, no more: the cap on
that number is this file's, and comes from the reference alone), and every scene still holds what it is in the matrix
for - tiles in which every primary ray misses, tiles in which some do, several primitives in view."""
import numpy as np
import pytest

import mode_content_cases as MC
from helpers import tiles

solr = MC.solr

# Tiles of pass 0 per scene: (tiles in which every primary ray misses, tiles in which some do); True: there are some,
# False: there are none.  From the scene's own camera - the perspective rays, which the five-ray camera (its last ray is
# the centre ray) and the anaglyph camera (an eye 350 to the side, 12 000 and more away) keep or nearly keep.
OWN_CAMERA = {"mix_plain": (False, True), "tex_flat": (False, False), "triangles": (True, True), "sticks": (True, True),
              "open_sky": (True, True), "open_room": (True, True)}
# The 3D-vision camera shows the middle half of the view twice, side by side: what the rim of the frame holds is cut off
# (mix_plain's 11 tiles with a miss lie there), the open scenes stay open.
VISION = dict(OWN_CAMERA, mix_plain=(False, False))
# The fish-eye camera turns once round the eye over the width of the frame: most of every scene's frame looks away from it
FISH_EYE = {scene: (True, True) for scene in OWN_CAMERA}
# Distinct primitives in view, pass 0.  open_sky has five in view from its own camera; the 3D-vision camera's two half
# frames cut one off.
MIN_IDS = 5
MIN_IDS_OF = {("open_sky", "3d-vision"): 4}
# Distinct float colours of the box view (its ids are all -1 and its RGB8 may be one value: the float buffer is what the
# comparison sees).  A node's colour is its material's, startIndex % NB_MAX_MATERIALS (GI:693-696): open_sky is seven
# primitives and cannot show more.
MIN_BOX_COLOURS = 15
MIN_BOX_COLOURS_OF = {"open_sky": 7}


def oracle_passes(oracle, case, only=None, **changes):
    """[(pass, pp, ids, rgb, status, misround)] of the case: the oracle over its own previous buffers.
    only: these passes instead of the case's; changes: MC.build's"""
    k = solr.Kernel(engine="host-only")
    passes = MC.build(k, case, **changes)
    passes = passes if only is None else only
    out, pp, ids = [], None, None
    try:
        flat = k.flat_scene()
        for it in passes:
            k.set_scene_info(pathTracingIteration=it)
            si, ppi, eye, direction, angles = k.frame_parameters()
            assert (si.size_x, si.size_y, si.maxPathTracingIterations) == (MC.W, MC.H, MC.MAX_PATH_TRACING_ITERATIONS)
            assert (ppi.type, ppi.param1, ppi.param2) == (solr.ppe_none, np.float32(9000.0), np.float32(0.002))
            misround = np.zeros((MC.H, MC.W), np.uint8)
            pp, ids, rgb, _, status = oracle.render(flat, si, ppi, eye, direction, angles, pp=pp, ids=ids, misround=misround)
            out.append((it, pp, ids, rgb, status, misround))
    finally:
        k.finalize()
    return out


def test_the_matrix():
    assert len(MC.CASES) == len(set(MC.CASES)) == 6 * 11 + 2
    assert set(MC.FULL_MODES) | {"random-illumination", "fog", "gradient"} == set(MC.MODES)
    for case in MC.CASES:
        passes = MC.passes_of(case)
        assert passes[0] == 0 and list(passes) == sorted(set(passes)) and max(passes) < MC.MAX_PATH_TRACING_ITERATIONS
        if case[1] in MC.CAMERA_MODES + MC.GI_MODES:
            assert 11 in passes


@pytest.mark.parametrize("case", MC.CASES, ids=MC.case_id)
def test_case(oracle, case):
    scene, mode = case
    assert not oracle.lib().oracle_get_rounded_transcendentals()
    frames = oracle_passes(oracle, case)
    marked = [int((m != 0).sum()) for _, _, _, _, _, m in frames]
    print("%s: marked pixels per pass %s" % (MC.case_id(case), marked))
    for (it, _, _, _, status, _), n in zip(frames, marked):
        assert status == 0, "pass %d: the oracle read outside the random buffer" % it
        assert n <= MC.MARKED_CAP, "pass %d: %d pixels behind a mis-rounded libm result" % (it, n)
    _, pp, ids, rgb, _, _ = frames[0]
    if mode == "boxes":
        assert (ids[..., 0] == -1).all()
        colours = len(np.unique(pp[..., :3].reshape(-1, 3), axis=0))
        assert colours >= MIN_BOX_COLOURS_OF.get(scene, MIN_BOX_COLOURS), colours
    else:
        missed = tiles(ids[..., 0] < 0, MC.TILE)
        all_miss = sum(1 for n, m in missed if m == n)
        some_miss = sum(1 for n, m in missed if 0 < m < n)
        want = (VISION if mode == "3d-vision" else FISH_EYE if mode == "fish-eye" else OWN_CAMERA)[scene]
        assert (all_miss > 0, some_miss > 0) == want, (all_miss, some_miss)
        in_view = len(np.unique(ids[..., 0][ids[..., 0] >= 0]))
        assert in_view >= MIN_IDS_OF.get(case, MIN_IDS), in_view
    if mode in MC.GRADIENT_MODES:
        # The flag shows: the gradient arm scales the background by 0.5 + the ray's height (CRT:278-286), a factor that is
        # 1 only for a ray exactly 30 degrees above the horizon - so against the same scene without the flag (the same
        # background, no skybox either) every pixel whose primary ray misses has another colour, and a scene in which none
        # misses (tex_flat) shows it by reflection.
        _, flat_pp, flat_ids, _, status, _ = oracle_passes(oracle, case, only=(0,), gradientBackground=0)[0]
        assert status == 0 and np.array_equal(flat_ids, ids)
        differs = (pp[..., :3].view(np.uint32) != flat_pp[..., :3].view(np.uint32)).any(axis=-1)
        missed = ids[..., 0] < 0
        print("%s: %d pixels miss, %d differ from the frame without the flag" % (MC.case_id(case), missed.sum(), differs.sum()))
        assert differs[missed].all(), int((missed & ~differs).sum())
        assert differs.any()
    if mode in MC.CAMERA_MODES + MC.GI_MODES:
        eleventh = [f for f in frames if f[0] == 11][0]
        assert not np.array_equal(eleventh[3], rgb), "pass 11 shows pass 0's image"
