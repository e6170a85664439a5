"""The lamp's cut-off of the shadow walks that keep the reference's order (rt_device.h shadowWalk, `lampCut`; DESIGN.md
section 4): such a walk leaves out the boxes that begin beyond the lamp - whatever they hold can only give hits that
`l < lengthOL` rejects.  solr_hip_set_variant(15) walks without it.  Two things are held here: the frames are the same
bit for bit with and without, in every situation the argument has a clause for; and the work does drop - the leaves a
frame's walks enter (solr_hip_walk_bound) are fewer in the Cornell box, whose glass keeps its shadow walks in the
reference's order, and the same in the opaque scenes, whose order-free shadow walks were cut off at the lamp already."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO_LAMP_CUTOFF = 15


def _same_frames(a, b):
    return (np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]) and
            np.array_equal(a[2], b[2]))


def _frame(k):
    rgb = k.render()
    k.check(0, "render")
    return (np.array(k.postprocessing_buffer(), copy=True), np.array(k.primitive_ids(), copy=True), np.array(rgb, copy=True))


def _with_and_without(solr, frames_of):
    """frames_of(k-maker's variant) -> list of frames; run with variant 0 and with variant 15, compare all"""
    hip = solr.hip_lib()
    got = {}
    try:
        for variant in (0, NO_LAMP_CUTOFF):
            hip.solr_hip_set_variant(variant)
            got[variant] = frames_of(variant)
    finally:
        hip.solr_hip_set_variant(0)
    assert len(got[0]) == len(got[NO_LAMP_CUTOFF]) > 0
    for n, (a, b) in enumerate(zip(got[0], got[NO_LAMP_CUTOFF])):
        assert _same_frames(a, b), "frame %d differs with and without the lamp's cut-off" % n
    return got[0]


def _room(solr, k, lamp, width=160, height=120, iterations=3, lamp_radius=10.0, **info):
    """a Cornell-like room with a lamp of one's own: mirror spheres, two glass ones (the shadow walks keep the
    reference's order), six walls"""
    scenes = solr.scenes
    rng = scenes.LCG(77)
    info.setdefault("graphicsLevel", solr.glFull)
    k.initialize(width=width, height=height, nbRayIterations=iterations, **info)
    for cx, cy in ((2200.0, 0.0), (-2200.0, 0.0), (0.0, 2200.0)):
        m = k.add_material(0.8, 0.5, 0.3, reflection=0.5, specValue=1.0, specPower=234.0)
        k.add_primitive(solr.ptSphere, (cx, cy, 0.0), size=(2000.0, 0, 0), material=m)
    for i in range(2):
        m = k.add_material(0.9, 0.95, 1.0, reflection=1.0, refraction=1.1, transparency=0.7, specValue=1.0, specPower=200.0)
        k.add_primitive(solr.ptSphere, (-5000.0 + 10000.0 * i, 3500.0, -6000.0), size=(1200.0, 0, 0), material=m)
    scenes.add_room(k, rng)
    scenes.add_light(k, position=lamp, radius=lamp_radius)
    k.compact_boxes(True)
    k.set_camera((0.0, 0.0, -15000.0))
    return k


CAMERAS = [((0.0, 0.0, -15000.0), (0.0, 0.0, 0.0)),
           ((9000.0, 6000.0, -12000.0), (0.0, 0.0, 0.0)),
           ((-12000.0, 20000.0, 5000.0), (0.0, 3000.0, -2000.0)),
           ((3000.0, -3000.0, 15000.0), (0.0, 0.0, 0.0))]


def test_cornell_frames_are_the_same_at_1080p_and_from_several_cameras(solr):
    hip = solr.hip_lib()

    def frames_of(variant):
        out = []
        k = solr.Kernel(engine="hip")
        solr.scenes.cornell(k, width=1920, height=1080, iterations=3)
        try:
            for _ in range(3):          # (the order-free lists arrive with the second frame)
                out.append(_frame(k))
            assert hip.solr_hip_order_free_shadows() == 0          # glass: the reference's order
            assert hip.solr_hip_shadow_lamp_cutoff() == (1 if variant == 0 else 0)
        finally:
            k.finalize()
        k = solr.Kernel(engine="hip")
        solr.scenes.cornell(k, width=200, height=136, iterations=3)
        try:
            for eye, look_at in CAMERAS:
                k.set_camera(eye, look_at=look_at)
                out.append(_frame(k))
        finally:
            k.finalize()
        return out

    frames = _with_and_without(solr, frames_of)
    assert not _same_frames(frames[3], frames[4])          # the cameras do see different frames


def test_after_a_rotation_on_the_device(solr):
    hip = solr.hip_lib()

    def frames_of(variant):
        out = []
        k = solr.Kernel(engine="hip")
        solr.scenes.cornell(k, width=200, height=136, iterations=3)
        try:
            for _ in range(2):
                out.append(_frame(k))
            for n in range(3):
                k.rotate_primitives((0.0, 0.0, 0.0), (0.02, 0.1, 0.0))
                assert k.pending_rotations() == n + 1, "the rotation took the host route"
                out.append(_frame(k))
                # the refitted list holds what it names, and was asked
                assert hip.solr_hip_shadow_lamp_cutoff() == (1 if variant == 0 else 0)
        finally:
            k.finalize()
        return out

    _with_and_without(solr, frames_of)


@pytest.mark.parametrize("lamp, radius, eye, look_at", [
    ((8000.0, 50000.0, -8000.0), 10.0, (0.0, 0.0, -15000.0), (0.0, 0.0, 0.0)),            # above the ceiling (y = 35 000)
    ((-30000.0, 9000.0, -26000.0), 10.0, (9000.0, 6000.0, -12000.0), (0.0, 0.0, 0.0)),    # behind two walls
    # one unit above the floor (y = -5000): the points around its foot are closer than 2 to it, their lanes keep the
    # reference's cut-off alone - seen from thirty units away and from the room's middle
    ((3000.0, -4999.0, -3000.0), 0.5, (3000.0, -4985.0, -3030.0), (3000.0, -5000.0, -3000.0)),
    ((3000.0, -4999.0, -3000.0), 0.5, (0.0, 0.0, -15000.0), (0.0, 0.0, 0.0)),
], ids=["outside-above", "outside-corner", "close-to-the-floor-near", "close-to-the-floor-far"])
def test_lamps_outside_the_room_and_next_to_a_surface(solr, lamp, radius, eye, look_at):
    def frames_of(variant):
        k = solr.Kernel(engine="hip")
        _room(solr, k, lamp, lamp_radius=radius)
        try:
            k.set_camera(eye, look_at=look_at)
            return [_frame(k) for _ in range(3)]
        finally:
            k.finalize()

    frames = _with_and_without(solr, frames_of)
    assert frames[-1][2].any()


def test_a_scene_with_a_textured_plane(solr):
    import scenes_extra as X

    def frames_of(variant):
        k = solr.Kernel(engine="hip")
        X.textured(k, width=160, height=120)
        try:
            return [_frame(k) for _ in range(3)]
        finally:
            k.finalize()

    _with_and_without(solr, frames_of)


def _strip_frame(solr, k, first, rows, width):
    hip = solr.hip_lib()
    rgb = k.render()
    k.check(0, "render")
    pp = np.zeros((rows, width, 8), np.float32)
    hip.solr_hip_d2h_postprocessing(C.c_void_p(pp.ctypes.data))
    return pp, np.array(k.primitive_ids()[first:first + rows], copy=True), np.array(rgb[first:first + rows], copy=True)


def test_two_accumulation_passes_of_cfg4_with_the_jittered_lamp(solr):
    """3840 x 2160 with ambient occlusion, passes 0 ... 12 on a strip of the frame: 11 and 12 are accumulated samples,
    their lamp jittered from the random buffer"""
    hip = solr.hip_lib()
    W, H, first, rows = 3840, 2160, 1000, 48

    def frames_of(variant):
        out = []
        k = solr.Kernel(engine="hip")
        k.set_post_processing(type=solr.ppe_ambientOcclusion, param1=11000.0, param2=10.0, param3=0)
        solr.scenes.cornell(k, width=W, height=H, iterations=1, maxPathTracingIterations=74)
        try:
            hip.solr_hip_set_strip(first, rows)
            for it in range(13):
                k.set_scene_info(pathTracingIteration=it, maxPathTracingIterations=74)
                frame = _strip_frame(solr, k, first, rows, W)
                if it >= 10:
                    out.append(frame)
        finally:
            hip.solr_hip_set_strip(0, -1)
            k.finalize()
        return out

    frames = _with_and_without(solr, frames_of)
    assert not np.array_equal(frames[1][0], frames[2][0])          # the passes did accumulate


def test_strips(solr):
    hip = solr.hip_lib()
    W, H = 640, 360

    def frames_of(variant):
        out = []
        k = solr.Kernel(engine="hip")
        solr.scenes.cornell(k, width=W, height=H, iterations=3)
        try:
            out.append(_frame(k))
            out.append(_frame(k))
            for first, rows in ((0, 120), (123, 61), (352, 8)):
                hip.solr_hip_set_strip(first, rows)
                out.append(_strip_frame(solr, k, first, rows, W))
        finally:
            hip.solr_hip_set_strip(0, -1)
            k.finalize()
        return out

    frames = _with_and_without(solr, frames_of)
    full = frames[1]
    for (first, rows), strip in zip(((0, 120), (123, 61), (352, 8)), frames[2:]):
        assert np.array_equal(strip[0].view(np.uint32), full[0][first:first + rows].view(np.uint32))
        assert np.array_equal(strip[1], full[1][first:first + rows])


def _walk_entries(solr, k):
    """leaves entered by the walks of the frame, as solr_hip_walk_bound replays them; the frame's shadow walks"""
    hip = solr.hip_lib()
    flat = k.flat_scene()
    si, ppi, eye, direction, angles = k.frame_parameters()
    si.pathTracingIteration = 0
    objects = solr.Vec4i(len(flat.boxes), len(flat.primitives), flat.nb_lamps, len(flat.lights))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    ms, stats = (C.c_double * 3)(), (C.c_ulonglong * 4)()
    status = hip.solr_hip_walk_bound(C.byref(si), C.byref(objects), C.byref(ppi), fp(eye), fp(direction), fp(angles), 1, ms, stats)
    k.check(status, "solr_hip_walk_bound")
    walks, left_out, entries, workgroups = [int(x) for x in stats]
    assert left_out == 0
    counts = (C.c_ulonglong * 8)()
    hip.solr_hip_render_counting(C.byref(si), C.byref(objects), C.byref(ppi), fp(eye), fp(direction), fp(angles), counts)
    k.check(0, "solr_hip_render_counting")
    return entries, int(counts[1]), float(ms[2])


@pytest.mark.parametrize("scene", ["cornell", "molecule", "height_field"])
def test_the_work_drops_where_the_walks_keep_the_reference_s_order_and_only_there(solr, scene):
    hip = solr.hip_lib()
    W, H = 1920, 1080
    got = {}
    try:
        for variant in (0, NO_LAMP_CUTOFF):
            hip.solr_hip_set_variant(variant)
            k = solr.Kernel(engine="hip")
            if scene == "cornell":
                solr.scenes.cornell(k, width=W, height=H, iterations=3)
            elif scene == "molecule":
                solr.scenes.molecule(k, atoms=20000, width=W, height=H)
            else:
                solr.scenes.height_field(k, n=96, width=W, height=H)
            try:
                for _ in range(3):
                    k.render()
                k.check(0, "render")
                assert hip.solr_hip_order_free_shadows() == (0 if scene == "cornell" else 1)
                got[variant] = _walk_entries(solr, k)
            finally:
                k.finalize()
    finally:
        hip.solr_hip_set_variant(0)
    (with_cut, shadow_walks, ms_with), (without, shadow_walks_15, ms_without) = got[0], got[NO_LAMP_CUTOFF]
    assert shadow_walks == shadow_walks_15 > 0
    print("%s %dx%d: leaf entries of the frame's walks %d with the lamp's cut-off, %d without: %d fewer, %.3f per shadow "
          "walk (%d shadow walks, %.3f leaf entries per pixel -> %.3f); node loop alone %.4f ms, %.4f ms without"
          % (scene, W, H, with_cut, without, without - with_cut, (without - with_cut) / shadow_walks, shadow_walks,
             without / (W * H), with_cut / (W * H), ms_with, ms_without))
    if scene == "cornell":
        assert with_cut < without
    else:
        assert with_cut == without
