"""Thin boxes for leaves of spheres (sol-r_amd/csrc/build_bounds.h sphereBuildExtent; solr_arena.hip k_tightenLeaves) on the
device.  The reference boxes the lamps' cell +-viewDistance, so every walk of every frame entered it; in the thin copies
of the lists it is now the lamps' own box.  Held here:
  - the engine's thin copies of the walk-order list and the eight order-free lists are the numpy model's
    (tests/sphere_leaves_model.py) bit for bit - the Cornell scene, a room with two lamps, a hand-made list with a loose
    leaf of spheres; after the upload, after a rotation, a translation, a lamp move, a batch of primitives set anew and a
    key-frame blend on the device; with solr_hip_set_variant(18) they are the copies of before (tests/list_copies_model.py);
  - frames are the oracle's under helpers.assert_parity_pinned and the same bits with variant 18: the Cornell box with
    glass and three bounces, the open room without glass (order-free shadow walks), a camera whose primary rays hit the
    lamp in some lanes of a tile and pass it in others, a room where the shadow rays towards one lamp cross the other's
    sphere, frames after each of the changes above, a frame whose viewDistance lies beyond the scene's extent (the copies
    are made again for that reach);
  - the work does drop: the leaves the walks of a 200 x 120 Cornell frame enter (solr_hip_walk_bound) are fewer than with
    variant 18 by at least the primary rays that miss the cell's thin box, counted on the host."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_probes as E  # noqa: E402
import helpers as H  # noqa: E402
import list_copies_model as M  # noqa: E402
import sphere_leaves_model as S  # noqa: E402

pytestmark = pytest.mark.gpu
f4, i4 = np.float32, np.int32
UPLOADED_SPHERE_LEAVES = 18
SMALL, LARGER = (64, 48), (200, 120)
LAMP_A, LAMP_B = (8000.0, 8000.0, -8000.0), (4000.0, 1500.0, -4000.0)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(i4), np.ascontiguousarray(b).view(i4))


def _frame(k):
    frame = H.copy_frame(H.gpu_frame(k))
    k.check(0, "render")
    return frame


def copies_are_the_model_s(solr, k, label, clause=True, offered=True):
    """the thin copies of the lists the walks take against the model, from the rows, start indices and primitive records
    the arena holds now; returns the thin box of the lamps' cell in the walk-order list as (lo, hi)"""
    hip = solr.hip_lib()
    si = k.frame_parameters()[0]
    offer = E.walk_offer(hip, si)
    assert offer["tightLists"] == 1 or not offered, (label, offer)
    margin, extent = f4(offer["margin"]), f4(offer["extent"])
    assert margin.view(i4) == M.margin_of(extent).view(i4)
    reach = S.reach_of(extent, si.viewDistance) if clause else f4(0.0)
    records = E.primitive_records(hip)
    kinds = M.kinds_of_records(records)
    cell = None
    for which, name in ((E.WALK_LIST, "the walk-order list"), (E.FREE_LISTS, "the order-free lists")):
        rows = E.list_copy(hip, which, E.NODE_ROWS)
        if rows is None:
            assert which == E.FREE_LISTS
            continue
        start, thin = E.list_copy(hip, which, E.START_INDICES), E.list_copy(hip, which, E.THIN_COPY)
        assert thin is not None, (label, name)
        nb = len(rows) // (8 if which == E.FREE_LISTS else 1)
        want = S.thin_copy(rows, start, records, kinds, margin, reach, list_length=nb)
        differing = np.flatnonzero((thin.view(i4) != want.view(i4)).reshape(len(rows), -1).any(axis=1))
        assert _same(thin, want), (label, name, differing[:8])
        plain = M.thin_copy(rows, start, records, np.where(np.isin(kinds, S.PLANES), kinds, 0), margin, list_length=nb)
        loose = S.loose_sphere_leaves(rows, start, records, kinds)
        assert len(loose) == (8 if which == E.FREE_LISTS else 1), (label, name, loose)
        for leaf in loose:
            assert _same(plain[leaf], rows[leaf])
            assert _same(thin[leaf], rows[leaf]) == (not clause), (label, name, leaf)
        if which == E.WALK_LIST:
            cell = (M.lo(thin)[loose[0]].copy(), M.hi(thin)[loose[0]].copy())
    return cell


def with_and_without(solr, frames_of):
    """frames_of(variant) -> frames, with variant 0 and with 18: the same bits; returns variant 0's"""
    hip = solr.hip_lib()
    got = {}
    try:
        for variant in (0, UPLOADED_SPHERE_LEAVES):
            hip.solr_hip_set_variant(variant)
            got[variant] = frames_of(variant)
    finally:
        hip.solr_hip_set_variant(0)
    assert len(got[0]) == len(got[UPLOADED_SPHERE_LEAVES]) > 0
    for n, (a, b) in enumerate(zip(got[0], got[UPLOADED_SPHERE_LEAVES])):
        assert H.same_frames(a, b), "frame %d differs with thin sphere leaves and without" % n
    return got[0]


def two_lamps(solr, k, size, iterations=2):
    """a room with two mirror spheres and two lamps: B, of radius 300, lies on the way from the floor around (0, -5000, 0) to
    A - the shadow rays towards A from there cross B's sphere"""
    scenes = solr.scenes
    rng = scenes.LCG(91)
    k.initialize(width=size[0], height=size[1], nbRayIterations=iterations, graphicsLevel=solr.glFull)
    for cx, cy in ((2200.0, 2000.0), (-4200.0, 0.0)):
        m = k.add_material(0.8, 0.5, 0.3, reflection=0.5, specValue=1.0, specPower=234.0)
        k.add_primitive(solr.ptSphere, (cx, cy, 3000.0), size=(1500.0, 0, 0), material=m)
    scenes.add_room(k, rng)
    scenes.add_light(k, position=LAMP_A)
    scenes.add_light(k, position=LAMP_B, radius=300.0)
    k.compact_boxes(True)
    k.set_camera((0.0, 4000.0, -15000.0), look_at=(0.0, -3000.0, 0.0))
    return k


def _checked_scene(solr, oracle, build, frames=3, after=None):
    """build(k) the scene; `frames` frames (the order-free lists arrive with the second); the last one and the copies are
    held to the oracle and the model with the clause, the copies to the model of before with variant 18"""
    def frames_of(variant):
        k = solr.Kernel(engine="hip")
        build(k)
        try:
            out = [_frame(k) for _ in range(frames)]
            cell = copies_are_the_model_s(solr, k, "variant %d" % variant, clause=variant == 0)
            if variant == 0:
                H.assert_frame_pinned(k, oracle, out[-1], None, "thin sphere leaves")
                if after is not None:
                    after(k, out[-1], cell)
            return out
        finally:
            k.finalize()

    return with_and_without(solr, frames_of)


def test_cornell_with_glass_and_three_bounces(solr, oracle):
    hip = solr.hip_lib()

    def after(k, frame, cell):
        assert hip.solr_hip_order_free_shadows() == 0          # glass: the shadow walks keep the reference's order
        lo, hi = cell
        assert (lo < np.array(LAMP_A) - 10).all() and (hi > np.array(LAMP_A) + 10).all() and (hi - lo < 2000).all()

    _checked_scene(solr, oracle, lambda k: solr.scenes.cornell(k, width=SMALL[0], height=SMALL[1], iterations=3), after=after)


def test_the_open_room_without_glass(solr, oracle):
    hip = solr.hip_lib()

    def after(k, frame, cell):
        assert hip.solr_hip_order_free_shadows() == 1

    _checked_scene(solr, oracle, lambda k: solr.scenes.cornell(k, width=LARGER[0], height=LARGER[1], iterations=2, glass=0), after=after)


def test_primary_rays_that_hit_the_lamp_and_pass_it(solr, oracle):
    def build(k):
        solr.scenes.cornell(k, width=LARGER[0], height=LARGER[1], iterations=2)
        # (200 units in front of the lamp, looking along z a few units beside its centre)
        k.set_camera((LAMP_A[0] - 4.0, LAMP_A[1] - 3.0, LAMP_A[2] - 200.0), look_at=(LAMP_A[0] - 4.0, LAMP_A[1] - 3.0, 0.0))

    def after(k, frame, cell):
        lamp = len(k.flat_scene().primitives) - 1
        on_lamp = frame[1][..., 0] == lamp
        tiles = H.tiles(on_lamp)
        mixed = sum(1 for size, hit in tiles if 0 < hit < size)
        print("pixels on the lamp: %d of %d; tiles with lanes on it and lanes beside it: %d" % (on_lamp.sum(), on_lamp.size, mixed))
        assert on_lamp.sum() >= 8 and mixed >= 2

    _checked_scene(solr, oracle, build, after=after)


def _shadows_towards_a(solr, k):
    """shadowWalk from points a unit above the floor towards lamp A, lamp A's sphere left out as the renderer leaves it out:
    64 points within 150 units of (0, -5000, 0), whose rays pass B's centre within 75 units (B's radius is 300), and 64
    points 3000 to 5000 units from there along x or z, whose rays pass B at more than 1400 and nothing else.  (result > 0:
    something shadows)"""
    hip = solr.hip_lib()
    rng = np.random.default_rng(7)
    under = np.stack([rng.uniform(-150, 150, 64), np.full(64, -4999.0), rng.uniform(-150, 150, 64)], axis=1)
    aside = under.copy()
    axis = rng.choice([0, 2], 64)
    aside[np.arange(64), axis] -= rng.uniform(3000, 5000, 64)
    origins = np.ascontiguousarray(np.concatenate([under, aside]), f4)
    si = k.frame_parameters()[0]
    records = E.primitive_records(hip)
    lamp_a = int(records[np.flatnonzero((records[:, M.ROW_P0_TYPE, :3] == f4(LAMP_A)).all(axis=1))[0], M.ROW_P1_INDEX, 3].view(i4))
    case = dict(name="shadow", si=si, origins=origins, lamps=np.ascontiguousarray(np.tile(f4(LAMP_A), (128, 1))),
                object_id=np.full(128, lamp_a, i4), iteration=np.zeros(128, i4))
    return E.walk_outputs(hip, case)


def test_a_shadow_ray_through_the_other_lamp(solr, oracle):
    hip = solr.hip_lib()

    def after(k, frame, cell):
        flat = k.flat_scene()
        assert flat.nb_lamps == 2
        lo, hi = cell          # one cell for both lamps: its thin box holds both
        for p in (LAMP_A, LAMP_B):
            assert (lo < np.array(p) - 10).all() and (hi > np.array(p) + 10).all()
        # B does shadow: the walks towards A enter the cell - its thin box - and find B's sphere there; beside it nothing
        _frame(k)          # (the scene the oracle looked at is resident again)
        mine = _shadows_towards_a(solr, k)
        assert (mine["result"][:64] > 0).all() and (mine["result"][64:] == 0).all(), mine["result"]
        try:
            hip.solr_hip_set_variant(UPLOADED_SPHERE_LEAVES)
            theirs = _shadows_towards_a(solr, k)
        finally:
            hip.solr_hip_set_variant(0)
        assert _same(mine["result"], theirs["result"]) and _same(mine["color"], theirs["color"])

    _checked_scene(solr, oracle, lambda k: two_lamps(solr, k, LARGER), after=after)


def test_a_viewdistance_beyond_the_scene_s_extent(solr, oracle):
    """the reach follows the frame: the copies are made again for it, and again for the smaller one"""
    hip = solr.hip_lib()
    k = solr.Kernel(engine="hip")
    solr.scenes.cornell(k, width=SMALL[0], height=SMALL[1], iterations=2)
    try:
        for _ in range(2):
            _frame(k)
        near = copies_are_the_model_s(solr, k, "viewDistance within the extent")
        k.set_scene_info(viewDistance=400000.0)
        frame = _frame(k)
        far = copies_are_the_model_s(solr, k, "viewDistance beyond the extent")
        assert (far[1] - far[0] > 4 * (near[1] - near[0])).all()
        H.assert_frame_pinned(k, oracle, frame, None, "viewDistance 400 000")
        k.set_scene_info(viewDistance=50000.0)
        _frame(k)
        again = copies_are_the_model_s(solr, k, "viewDistance within the extent again")
        assert _same(again[0], near[0]) and _same(again[1], near[1])
    finally:
        k.finalize()
        hip.solr_hip_set_variant(0)


def test_a_hand_made_list_with_loose_sphere_leaves(solr, oracle):
    """through the C ABI alone: two lamps in a cell boxed +-viewDistance and a sphere in a box of another host's"""
    from oracle import probes
    hip = solr.hip_lib()
    scene = S.light_cell(solr, 50000.0, lamps=2, extra=[("loose", [((2000.0, 2000.0, 2000.0), 300.0)], ([0.0] * 3, [9000.0] * 3))])
    si = probes._scene_info()
    lights = np.zeros(1, solr.LIGHT_DTYPE)
    lights["primitiveId"], lights["materialId"] = scene.lamp, M.LAMP
    lights["location"], lights["color"] = scene.prims["p0"][scene.lamp], (1.0, 1.0, 1.0, 2.0)
    materials = M.hand_made_materials(solr.MATERIAL_DTYPE)
    with E.Resident(solr, si, scene.boxes, scene.prims, materials, M.texture_atlas(), lights, nb_lamps=1):
        offer = E.walk_offer(hip, si)
        margin = M.margin_of(M.extent(scene.prims))
        assert f4(offer["margin"]).view(i4) == margin.view(i4)
        reach = S.reach_of(M.extent(scene.prims), si.viewDistance)
        records = E.primitive_records(hip)
        kinds = S.kinds(scene.prims, materials)
        assert np.array_equal(np.where(np.isin(M.kinds_of_records(records), (1, 2, 3, 4)), M.kinds_of_records(records), 0), kinds)
        for which in (E.WALK_LIST, E.FREE_LISTS):
            rows = E.list_copy(hip, which, E.NODE_ROWS)
            if rows is None:
                continue
            start, thin = E.list_copy(hip, which, E.START_INDICES), E.list_copy(hip, which, E.THIN_COPY)
            nb = len(rows) // (8 if which == E.FREE_LISTS else 1)
            want = S.thin_copy(rows, start, records, kinds, margin, reach, list_length=nb)
            assert _same(thin, want), which
            loose = S.loose_sphere_leaves(rows, start, records, kinds)
            assert len(loose) == 2 * (8 if which == E.FREE_LISTS else 1)
            assert all(not _same(thin[leaf], rows[leaf]) for leaf in loose)




def test_a_scene_whose_only_thin_leaves_are_sphere_leaves(solr, oracle):
    """every plane of the hand-made list wireframe (mode 2: none is a plain one): no thin copy was made for such a scene - now
    one is, for the loose leaves of spheres, and the walks are offered it; the same list with every sphere leaf boxed
    p0 -+ r has nothing to gain and gets none"""
    from oracle import probes
    hip = solr.hip_lib()
    materials = M.hand_made_materials(solr.MATERIAL_DTYPE)
    for material in (M.PLAIN, M.TEXTURED, M.EMISSIVE, M.WIRE):
        materials["attributes"][material, 2], materials["attributes"][material, 3] = 2, 5
    si = probes._scene_info()
    for loose in (True, False):
        scene = S.light_cell(solr, 50000.0, extra=[("loose", [((2000.0, 2000.0, 2000.0), 300.0)], ([0.0] * 3, [9000.0] * 3))]) \
            if loose else M.panels(solr)
        assert not M.plain_kinds(scene.prims, materials).any()
        lights = np.zeros(1, solr.LIGHT_DTYPE)
        lights["primitiveId"], lights["materialId"] = scene.lamp, M.LAMP
        lights["location"], lights["color"] = scene.prims["p0"][scene.lamp], (1.0, 1.0, 1.0, 2.0)
        with E.Resident(solr, si, scene.boxes, scene.prims, materials, M.texture_atlas(), lights, nb_lamps=1):
            offer = E.walk_offer(hip, si)
            rows, thin = E.list_copy(hip, E.WALK_LIST, E.NODE_ROWS), E.list_copy(hip, E.WALK_LIST, E.THIN_COPY)
            if not loose:
                assert offer["tightLists"] == 0 and thin is None
                continue
            assert offer["tightLists"] == 1 and thin is not None, offer
            records, start = E.primitive_records(hip), E.list_copy(hip, E.WALK_LIST, E.START_INDICES)
            kinds = S.kinds(scene.prims, materials)
            assert np.array_equal(np.where(np.isin(M.kinds_of_records(records), (1, 2, 3, 4)), M.kinds_of_records(records), 0), kinds)
            margin, reach = M.margin_of(M.extent(scene.prims)), S.reach_of(M.extent(scene.prims), si.viewDistance)
            assert _same(thin, S.thin_copy(rows, start, records, kinds, margin, reach))
            changed = np.flatnonzero((thin.view(i4) != rows.view(i4)).reshape(len(rows), -1).any(axis=1))
            leaves = changed[M.counts(rows)[changed] > 0].tolist()
            assert leaves == S.loose_sphere_leaves(rows, start, records, kinds) and len(leaves) == 2


# ---- the resident scene changes ------------------------------------------------------------------------------------------
LAMP_THERE = (-6000.0, 12000.0, 3000.0)


@pytest.mark.parametrize("what", ["rotation", "translation", "lamp move", "primitives set anew"])
def test_the_thin_cell_follows_the_resident_scene(solr, oracle, what):
    """a rotation, a translation, a lamp move, a batch of primitives set anew - a sphere moved and resized - on the device:
    the copies are the model of the records as they are now, and the frame is the oracle's"""
    k = solr.Kernel(engine="hip")
    solr.scenes.cornell(k, width=SMALL[0], height=SMALL[1], iterations=2)
    try:
        for _ in range(3):
            _frame(k)
        before = copies_are_the_model_s(solr, k, "uploaded")
        records = E.primitive_records(solr.hip_lib())
        # (the ids of the scene store, which the setters take: the records are in the order of the leaves, the lamp first)
        ids = records[:, M.ROW_P1_INDEX, 3].view(i4)
        lamp, ball = len(records) - 1, 5
        at = {i: int(np.flatnonzero(ids == i)[0]) for i in (lamp, ball)}
        assert (records[at[lamp], M.ROW_P0_TYPE, 3].view(i4) & 0xff) == solr.ptSphere and records[at[lamp], M.ROW_SIZE_MAT, 0] == 10.0
        assert (records[at[ball], M.ROW_P0_TYPE, 3].view(i4) & 0xff) == solr.ptSphere and records[at[ball], M.ROW_SIZE_MAT, 0] == 600.0
        if what == "rotation":
            k.rotate_primitives((0.0, 0.0, 0.0), (0.02, 0.1, 0.0))
        elif what == "translation":
            k.translate_primitives((150.0, -40.0, 60.0))
        elif what == "lamp move":
            k.set_primitive_center(lamp, LAMP_THERE)
        else:
            assert k.set_primitives([{"index": ball, "materialId": int(records[at[ball], M.ROW_SIZE_MAT, 3].view(i4)),
                                      "p0": (7000.0, -3000.0, 5000.0), "size": (900.0, 0.0, 0.0)}]) == 0
        assert k.pending_moves() == 1, "the %s took the host route" % what
        frame = _frame(k)
        cell = copies_are_the_model_s(solr, k, "after the " + what)
        assert not _same(E.primitive_records(solr.hip_lib()), records)
        if what == "lamp move":
            assert (cell[0] < np.array(LAMP_THERE) - 10).all() and (cell[1] > np.array(LAMP_THERE) + 10).all()
            assert (cell[1] - cell[0] < 2000).all() and not _same(cell[0], before[0])
        assert k.pending_moves() == 1          # (reading the device does not wake the host store; the oracle's scene does)
        H.assert_frame_pinned(k, oracle, frame, None, "after the " + what)
    finally:
        k.finalize()


def test_the_cell_of_two_lamps_after_a_rotation(solr, oracle):
    """two spheres in one cell that nobody refits: its thin box is the union of their boxes.  The scene's lamps are not
    movable (scenes.add_light), so a rotation turns everything else: every copy is made again from the rotated records, and
    the cell's thin box must come out the same bits as before"""
    k = two_lamps(solr, solr.Kernel(engine="hip"), SMALL)
    try:
        for _ in range(3):
            _frame(k)
        before = copies_are_the_model_s(solr, k, "two lamps, uploaded")
        records = E.primitive_records(solr.hip_lib())
        for n in range(2):
            k.rotate_primitives((0.0, 0.0, 0.0), (0.03, -0.2, 0.05))
            assert k.pending_rotations() == n + 1, "the rotation took the host route"
            frame = _frame(k)
            cell = copies_are_the_model_s(solr, k, "two lamps, after rotation %d" % (n + 1))
        moved = E.primitive_records(solr.hip_lib())
        lamps = [i for i in range(len(moved)) if moved[i, M.ROW_SIZE_MAT, 0] in (10.0, 300.0) and
                 (moved[i, M.ROW_P0_TYPE, 3].view(i4) & 0xff) == solr.ptSphere]
        others = [i for i in range(len(moved)) if i not in lamps]
        assert len(lamps) == 2 and _same(moved[lamps], records[lamps])
        assert not _same(moved[others][:, M.ROW_P0_TYPE, :3], records[others][:, M.ROW_P0_TYPE, :3])     # (the rest did turn)
        for i in lamps:
            r = moved[i, M.ROW_SIZE_MAT, 0]
            assert (cell[0] < moved[i, M.ROW_P0_TYPE, :3] - r).all() and (cell[1] > moved[i, M.ROW_P0_TYPE, :3] + r).all()
        assert _same(cell[0], before[0]) and _same(cell[1], before[1])
        H.assert_frame_pinned(k, oracle, frame, None, "two lamps after two rotations")
    finally:
        k.finalize()


def test_the_thin_cell_after_a_key_frame_blend(solr, oracle):
    """tests/morph_cases.py's mixed scene (spheres, planes, triangles, a cylinder, a lamp in its cell) blended between its key
    frames on the device: the blend ends in the refit every other move ends in, and the copies are made from the blended
    records"""
    import morph_cases
    k = morph_cases.build(solr.Kernel(engine="hip", deterministic_seed=1), "mix")
    try:
        for _ in range(3):
            _frame(k)
        copies_are_the_model_s(solr, k, "uploaded", offered=False)
        records = E.primitive_records(solr.hip_lib())
        assert k.morph_frame(0.3) == 0 and k.pending_morph(), "the blend took the host route"
        frame = _frame(k)
        copies_are_the_model_s(solr, k, "after the blend", offered=False)
        assert not _same(E.primitive_records(solr.hip_lib()), records)
        # (textured triangles: a texel index behind a mis-rounded libm result selects the neighbouring texel - counted, not bounded)
        H.assert_frame_pinned(k, oracle, frame, None, "after the blend", marked_bounds=(None, None))
    finally:
        k.finalize()


# ---- the work drops ------------------------------------------------------------------------------------------------------
def _primary_rays(size, eye, target, aw):
    """origin, directions (H, W, 3) of a frame's primary rays: renderer_kernel.h's perspective camera with angles
    (0, 0, 0, aw) in binary32; the walks take target - origin"""
    w, h = size
    stepx = f4(f4(f4(w) / f4(h)) * f4(aw)) / f4(w)
    stepy = f4(aw) / f4(h)
    x = np.arange(w, dtype=i4) - i4(w // 2)
    y = np.arange(h, dtype=i4) - i4(h // 2)
    d = np.zeros((h, w, 3), f4)
    d[..., 0] = (f4(target[0]) - stepx * x.astype(f4))[None, :]
    d[..., 1] = (f4(target[1]) + stepy * y.astype(f4))[:, None]
    d[..., 2] = f4(target[2])
    return np.asarray(eye, f4), (d - np.asarray(eye, f4)).astype(f4)


def _misses(lo, hi, origin, d):
    """per ray: the node loop's slab test of the box fails ((bound - o) * (1 / d), min / max; entered if near <= far, far > 0)"""
    d = d.reshape(-1, 3)
    with np.errstate(divide="ignore"):
        inv = np.where(d != 0, f4(1) / d, f4(1)).astype(f4)
    a, b = ((lo - origin).astype(f4) * inv).astype(f4), ((hi - origin).astype(f4) * inv).astype(f4)
    near, far = np.minimum(a, b).max(axis=1), np.maximum(a, b).min(axis=1)
    return ~((near <= far) & (far > 0))


def test_fewer_leaves_are_entered(solr):
    """The walks of a 200 x 120 Cornell frame, replayed by solr_hip_walk_bound.  With sphere leaves as uploaded (variant 18)
    every walk enters the lamps' cell: its origin lies inside +-viewDistance.  With the clause a walk enters it only if its
    ray passes the cell's thin box.  Counted on the host, from the thin box read back and the frame's camera: the primary
    rays whose slab test misses that box - each of them is one leaf entry less, so the entries must fall by at least that
    count (an unchanged copy gives a difference of zero, a copy that thinned the cell for part of the walks less than the
    count).  Not in the count: the bounce walks, which lose the entry too where they pass the box by (the host does not
    have their rays), and the shadow walks, which do not - a shadow ray ends in the lamp, inside the thin box whatever its
    size."""
    import test_shadow_lamp_cutoff_gpu as L
    hip = solr.hip_lib()
    W, H_ = LARGER
    got = {}
    try:
        for variant in (0, UPLOADED_SPHERE_LEAVES):
            hip.solr_hip_set_variant(variant)
            k = solr.Kernel(engine="hip")
            solr.scenes.cornell(k, width=W, height=H_, iterations=3)
            try:
                for _ in range(3):
                    k.render()
                k.check(0, "render")
                got[variant] = L._walk_entries(solr, k)
                if variant == 0:
                    lo, hi = copies_are_the_model_s(solr, k, "the frame's copies")
                    si, _, eye, target, angles = k.frame_parameters()
                    assert not np.asarray(angles[:3]).any()
                    origin, d = _primary_rays((W, H_), eye, target, float(angles[3]))
                    missing = int(_misses(lo, hi, origin, d).sum())
            finally:
                k.finalize()
    finally:
        hip.solr_hip_set_variant(0)
    (thin, shadow_walks, _), (uploaded, shadow_walks_18, _) = got[0], got[UPLOADED_SPHERE_LEAVES]
    print("Cornell %d x %d: leaf entries %d with thin sphere leaves, %d without: %d fewer; primary rays that miss the cell's thin "
          "box %d of %d; %d shadow walks" % (W, H_, thin, uploaded, uploaded - thin, missing, W * H_, shadow_walks))
    assert shadow_walks == shadow_walks_18 > 0
    assert missing > (W * H_ * 9) // 10          # (the count is worth asserting: the box is small from the camera)
    assert uploaded - thin >= missing
