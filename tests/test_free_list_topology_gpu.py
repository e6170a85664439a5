"""The order-free lists built on build bounds (sol-r_amd/csrc/build_bounds.h) in the engine: whatever hierarchy lies over
the leaves, a frame is the oracle's; it is the same frame bit for bit with solr_hip_set_variant(17) - the hierarchy on
the boxes as uploaded - and with SOLR_HIP_LISTS_ON_HOST=1; the device builder's lists are the host builder's bit for
bit, every copy of them, as built, with a material more (the arena laid out again), after a rotation on the device that
moves the rectangles' thin boxes, and after finalize_scene and a second upload.  Scenes without an axis-plane leaf - the
open room, the mesh, the molecule - get the same node rows with the variant on and off.  64 x 48 and 200 x 120: the
second has tiles on both sides of both camera axes, so walks of four octants, and ragged last tiles."""
import ctypes as C
import os

import numpy as np
import pytest

import engine_probes as E
import list_copies_model as M
import test_list_copies_gpu as L
from helpers import assert_frame_pinned, assert_parity_pinned, gpu_frame

pytestmark = pytest.mark.gpu
UPLOADED_BUILD_BOXES = 17
SIZES = [(64, 48), (200, 120)]
COPIES = (E.NODE_ROWS, E.THIN_COPY, E.SORTED_COPY, E.LEAF_RECORDS, E.START_INDICES)


def _cornell_glass(solr, k, w, h):
    solr.scenes.cornell(k, width=w, height=h, iterations=3, glass=2)


def _cornell_no_glass(solr, k, w, h):
    solr.scenes.cornell(k, width=w, height=h, iterations=3, glass=0)


def _open_room(solr, k, w, h):
    solr.scenes.cornell(k, width=w, height=h, iterations=3, room=False, gradientBackground=1, bgColor=(0.3, 0.5, 0.7, 0.2))


SCENES = {"cornell-glass": _cornell_glass, "cornell-no-glass": _cornell_no_glass, "open-room-gradient": _open_room}


def _copy(frame):
    return tuple(np.array(a, copy=True) for a in frame)


def _free_lists(hip):
    out = {}
    for what in COPIES:
        c = E.list_copy(hip, E.FREE_LISTS, what)
        out[what] = None if c is None else np.ascontiguousarray(c).view(np.int32).copy()
    return out


def _assert_same_lists(a, b, label):
    for what in COPIES:
        assert (a[what] is None) == (b[what] is None), (label, what)
        if a[what] is not None:
            assert a[what].shape == b[what].shape and np.array_equal(a[what], b[what]), "%s: copy %d of the order-free lists differs" % (label, what)


class _Mode:
    """variant and SOLR_HIP_LISTS_ON_HOST for the scenes made inside; both taken back afterwards"""

    def __init__(self, solr, variant=0, on_host=False):
        self.hip, self.variant, self.on_host = solr.hip_lib(), variant, on_host

    def __enter__(self):
        self.hip.solr_hip_set_variant(self.variant)
        if self.on_host:
            os.environ["SOLR_HIP_LISTS_ON_HOST"] = "1"
        else:
            os.environ.pop("SOLR_HIP_LISTS_ON_HOST", None)

    def __exit__(self, *exc):
        self.hip.solr_hip_set_variant(0)
        os.environ.pop("SOLR_HIP_LISTS_ON_HOST", None)
        return False


def _history(solr, oracle, make, w, h, against_oracle):
    """a scene's life: upload, the frames until its lists are built, a frame from them; a material more, a frame; a rotation
    on the device, a frame; finalize_scene and the same scene again, a frame - each with every copy of the lists"""
    hip = solr.hip_lib()
    E.declare(hip)
    out = []
    for life in range(2):
        k = solr.Kernel(engine="hip")
        try:
            make(solr, k, w, h)
            k.render()
            k.render()
            frame = _copy(gpu_frame(k))
            k.check(0, "frames")
            if against_oracle and life == 0:
                print(assert_frame_pinned(k, oracle, frame, 2, "%d x %d" % (w, h)))
            out.append(("life %d, as built" % life, frame, _free_lists(hip), hip.solr_hip_order_free_nodes()))
            if life == 1:
                continue
            k.add_material(0.1, 0.9, 0.2, specValue=0.5, specPower=10.0)
            out.append(("a material more", _copy(gpu_frame(k)), _free_lists(hip), hip.solr_hip_order_free_nodes()))
            k.rotate_primitives((0.0, 0.0, 0.0), (0.05, 0.1, 0.0))      # (no wall stays an axis plane's box where it was)
            frame = _copy(gpu_frame(k))
            k.check(0, "rotated frame")
            out.append(("rotated", frame, _free_lists(hip), hip.solr_hip_order_free_nodes()))
        finally:
            k.finalize()
    return out


@pytest.mark.parametrize("size", SIZES, ids=["64x48", "200x120"])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_the_frame_is_the_oracles_and_the_same_on_either_hierarchy_from_either_builder(solr, oracle, scene, size):
    make, (w, h) = SCENES[scene], size
    with _Mode(solr):
        device = _history(solr, oracle, make, w, h, True)
    with _Mode(solr, on_host=True):
        host = _history(solr, oracle, make, w, h, False)
    with _Mode(solr, variant=UPLOADED_BUILD_BOXES):
        uploaded = _history(solr, oracle, make, w, h, False)
    assert device[0][3] > 0, "no order-free lists"
    for (label, frame, lists, n), (_, frame_h, lists_h, n_h), (_, frame_u, lists_u, n_u) in zip(device, host, uploaded):
        for a, b, c in zip(frame, frame_h, frame_u):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%s: the frame differs with the lists built on the host" % label
            assert np.array_equal(a.view(np.uint8), c.view(np.uint8)), "%s: the frame differs on the hierarchy of the uploaded boxes" % label
        assert n == n_h, label
        _assert_same_lists(lists, lists_h, label)
        if label.endswith("as built"):
            rows, rows_u = lists[E.NODE_ROWS], lists_u[E.NODE_ROWS]
            same = rows.shape == rows_u.shape and np.array_equal(rows, rows_u)
            # (the switch switches something exactly where there is a rectangle to build on)
            assert same == (scene == "open-room-gradient"), (label, rows.shape, rows_u.shape)


def _panels_frame(solr, scene, si, frames=3):
    """the resident panels rendered `frames` times through the C ABI (the lists are built with the second): pp, ids, RGB8"""
    hip = solr.hip_lib()
    w, h = si.size_x, si.size_y
    objects = solr.Vec4i(len(scene.boxes), len(scene.prims), 1, 1)
    ppi = solr.PostProcessingInfo()
    fp = lambda a: np.array(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    for _ in range(frames):
        hip.solr_hip_render(C.byref(si), C.byref(objects), C.byref(ppi), fp(L.EYE), fp(L.LOOK), fp(L.ANGLES))
        E._check(hip, 0, "render")
    pp, ids, rgb = np.zeros((h, w, 8), np.float32), np.zeros((h, w, 4), np.int32), np.zeros((h, w, 3), np.uint8)
    hip.solr_hip_d2h_postprocessing(C.c_void_p(pp.ctypes.data))
    hip.solr_hip_d2h(C.byref(si), C.c_void_p(rgb.ctypes.data), C.c_void_p(ids.ctypes.data))
    E._check(hip, 0, "read-back")
    return (pp, ids, rgb), ppi


@pytest.mark.parametrize("size", SIZES, ids=["64x48", "200x120"])
def test_panels_the_frame_is_the_oracles(solr, oracle, size):
    """the hand-made list of plane leaves, the scene whose hierarchy build bounds change most (32 leaves of rectangles that
    stay inside it): the frame from the order-free lists on build bounds against the oracle's on the same arrays, by
    helpers.assert_parity_pinned; and the frame on the hierarchy of the uploaded boxes is the same frame"""
    from oracle import probes
    scene = M.panels(solr, opaque=True)
    materials = M.hand_made_materials(solr.MATERIAL_DTYPE)
    si = probes._scene_info(size_x=size[0], size_y=size[1])
    frames = {}
    for variant in (0, UPLOADED_BUILD_BOXES):
        with _Mode(solr, variant=variant):
            hip = solr.hip_lib()
            with E.Resident(solr, si, scene.boxes, scene.prims, materials, M.texture_atlas(), L._lights(solr, scene), nb_lamps=1):
                hip.solr_hip_set_variant(variant)       # (Resident sets 0)
                frames[variant], ppi = _panels_frame(solr, scene, si)
                offer = E.walk_offer(hip, si)
                assert offer["nbBoxesFree"] > 0, offer
    gpu = frames[0]
    assert len(np.unique(gpu[2].reshape(-1, 3), axis=0)) > 1, "the frame is one colour"
    flat = solr.FlatScene(scene.boxes, scene.prims, L._lights(solr, scene), 1, materials, np.zeros(4096, np.float32), M.texture_atlas())
    misround = np.zeros((size[1], size[0]), np.uint8)
    assert not oracle.lib().oracle_get_rounded_transcendentals()
    opp, oids, orgb, _, status = oracle.render(flat, si, ppi, L.EYE, L.LOOK, L.ANGLES, misround=misround)
    assert status == 0, "the oracle read outside the random buffer"
    print(assert_parity_pinned(gpu, (opp, oids, orgb), misround, 2, "panels %d x %d" % size))
    for a, b in zip(gpu, frames[UPLOADED_BUILD_BOXES]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the frame differs on the hierarchy of the uploaded boxes"


def test_panels_the_same_state_from_either_builder_and_the_same_frame_on_either_hierarchy(solr, oracle):
    """the hand-made list of plane leaves (tests/list_copies_model.py): everything the engine holds of it - every copy of
    every list, the frame - with the lists built on the device and on the host, as uploaded, with the materials uploaded
    again and after a rotation; and the frame alone on the hierarchy of the uploaded boxes"""
    scene = M.panels(solr, opaque=True)
    states = {}
    for mode, kw in (("device", {}), ("host", dict(on_host=True)), ("uploaded", dict(variant=UPLOADED_BUILD_BOXES))):
        with _Mode(solr, **kw):
            hip = solr.hip_lib()
            with L.fresh(solr, scene):
                hip.solr_hip_set_variant(kw.get("variant", 0))      # (Resident sets 0)
                keep, mine = [], []
                mine.append(L.snapshot(solr, scene))
                mine.append(L.snapshot(solr, scene))                # (the lists are built by now)
                L.upload_materials(solr, M.hand_made_materials(solr.MATERIAL_DTYPE), keep)
                mine.append(L.snapshot(solr, scene))
                L.rotate(solr, L._frame_info(), 1)
                mine.append(L.snapshot(solr, scene))
                states[mode] = mine
    assert states["device"][1]["order-free nodes, lamp cut-off"][0] > 0, "no order-free lists for panels"
    for n, (a, b, c) in enumerate(zip(states["device"], states["host"], states["uploaded"])):
        L.assert_same_state(a, b, "panels, snapshot %d, device against host" % n)
        for key in a:
            if key.startswith("frame"):
                assert a[key] == c[key], "panels, snapshot %d: %s differs on the hierarchy of the uploaded boxes" % (n, key)
    assert states["device"][1]["list %d, copy %d" % (E.FREE_LISTS, E.NODE_ROWS)] != states["uploaded"][1]["list %d, copy %d" % (E.FREE_LISTS, E.NODE_ROWS)]


@pytest.mark.parametrize("scene,kw", [("height_field", dict(n=64, width=64, height=48)), ("molecule", dict(atoms=3000, width=64, height=48))],
                         ids=["small-mesh", "small-molecule"])
def test_scenes_without_axis_plane_leaves_keep_their_lists(solr, scene, kw):
    """the variant on and off in THIS build: the switch changes nothing where there is no rectangle to build on.  That these
    lists are also the bytes of the builder before build bounds rests elsewhere: on the hashes recorded from that builder
    (tests/test_free_list_topology.py, host builder) and on the device builder being held to the host's bit for bit on the
    mesh and the molecule (tests/test_lists_gpu.py)"""
    hip = solr.hip_lib()
    E.declare(hip)
    rows = {}
    for variant in (0, UPLOADED_BUILD_BOXES):
        with _Mode(solr, variant=variant):
            k = solr.Kernel(engine="hip")
            try:
                getattr(solr.scenes, scene)(k, **kw)
                for _ in range(3):
                    k.render()
                k.check(0, "frames")
                rows[variant] = _free_lists(hip)
            finally:
                k.finalize()
    assert rows[0][E.NODE_ROWS] is not None
    _assert_same_lists(rows[0], rows[UPLOADED_BUILD_BOXES], scene)


def test_the_variant_builds_the_lists_of_a_resident_scene_again(solr):
    """set while the scene's lists exist, the variant has them built again with the next frame - and taken back, again: the
    lists of the uploaded boxes and back to the ones on build bounds, the frame the same throughout"""
    hip = solr.hip_lib()
    E.declare(hip)
    with _Mode(solr):
        k = solr.Kernel(engine="hip")
        try:
            _cornell_glass(solr, k, 64, 48)
            seen = []
            for variant in (0, UPLOADED_BUILD_BOXES, 0):
                hip.solr_hip_set_variant(variant)
                k.render()
                frame = _copy(gpu_frame(k))
                k.check(0, "frames")
                seen.append((frame, _free_lists(hip)))
        finally:
            k.finalize()
    for frame, _ in seen[1:]:
        for a, b in zip(seen[0][0], frame):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    _assert_same_lists(seen[0][1], seen[2][1], "back on build bounds")
    a, b = seen[0][1][E.NODE_ROWS], seen[1][1][E.NODE_ROWS]
    assert a.shape != b.shape or not np.array_equal(a, b), "the variant did not change the lists"
