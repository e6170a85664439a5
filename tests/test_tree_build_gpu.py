"""GPUKernel::compactBoxes(true) on the device (sol-r_amd/csrc/solr_tree.hip, solr_hip_build_tree) against the
host builder: the flattened node list - bounds, primitive counts, start indices, skip pointers - and the order
in which the primitives are streamed must be the host builder's, bit for bit, which tests/
test_builder_reference_model.py in turn holds to a line-by-line model of the reference's builder.  Scenes: the
small ones of that test (key wraps, several lamps, five primitive types), BASELINE's cfg2 (100 352
triangles) and cfg3 (50 000 atoms, 100k spheres and cylinders), and the synthetic ones of tests/tree_builder_cases.py,
each of which steers one of the places where the builder's header says the tree is decided: there the model also says
whether the device must build the tree or leave it to the host (-2).  Some of them go through the engine's own
route as well (GPUKernel::buildTreeOnDevice), next to a second kernel that builds on the host."""
import ctypes as C
import importlib
import time

import numpy as np
import pytest

import test_builder_reference_model as M
import tree_builder_cases as K

pytestmark = pytest.mark.gpu


def _build(solr, by_index, emissive, lo, hi, view_distance, capacity=None, depth_before=2):
    hip = solr.hip_lib()
    hip.solr_hip_build_tree_message.restype = C.c_char_p
    n = len(by_index)
    boxes = np.zeros(12 * n + 64 if capacity is None else capacity, solr.BOX_DTYPE)
    order = np.zeros(n, np.int32)
    nb_boxes, nb_lamps = C.c_int(), C.c_int()
    t0 = time.perf_counter()
    args = [C.c_void_p(by_index.ctypes.data), C.c_void_p(emissive.ctypes.data), n, C.c_void_p(lo.ctypes.data),
            C.c_void_p(hi.ctypes.data), C.c_float(view_distance), C.c_void_p(boxes.ctypes.data), len(boxes),
            C.c_void_p(order.ctypes.data), C.byref(nb_boxes), C.byref(nb_lamps)]
    if depth_before == 2:                                   # a fresh kernel
        depth = hip.solr_hip_build_tree(*args)
    else:                                                   # one that has built a tree of that depth before
        depth = hip.solr_hip_build_tree_after(*args[:6], depth_before, *args[6:])
    seconds = time.perf_counter() - t0
    return depth, boxes[: max(nb_boxes.value, 0)], order, nb_lamps.value, seconds


def _device_tree(solr, flat, view_distance):
    n = len(flat.primitives)
    by_index = np.zeros(n, flat.primitives.dtype)
    by_index[flat.primitives["index"]] = flat.primitives            # the scene's primitives in index order
    assert np.array_equal(np.sort(flat.primitives["index"]), np.arange(n))
    emissive = (flat.materials["innerIllumination"][by_index["materialId"], 0] != 0).astype(np.uint8)
    p0 = by_index["p0"]
    lo = np.minimum(p0.min(axis=0), 0).astype(np.float32)           # a fresh kernel's extent: primitives and the origin
    hi = np.maximum(p0.max(axis=0), 0).astype(np.float32)
    depth, boxes, order, nb_lamps, seconds = _build(solr, by_index, emissive, lo, hi, view_distance)
    assert depth >= 1, (depth, solr.hip_lib().solr_hip_build_tree_message())
    return boxes, order, nb_lamps, depth, seconds


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_nodes(boxes, expected):
    """every field of the node record; the floats as the words they are: the sign of a zero counts"""
    assert len(boxes) == len(expected)
    for field in ("min", "max"):
        assert np.array_equal(_words(boxes[field]), _words(expected[field])), field
    for field in ("nbPrimitives", "startIndex", "indexForNextBox"):
        assert np.array_equal(boxes[field], expected[field]), field
    assert set(boxes.dtype.names) == {"min", "max", "nbPrimitives", "startIndex", "indexForNextBox"}


def _same_tree(boxes, order, nb_lamps, flat):
    _same_nodes(boxes, flat.boxes)
    assert np.array_equal(order, flat.primitives["index"])
    assert nb_lamps == flat.nb_lamps


@pytest.mark.parametrize("name", list(M.SCENES))
def test_small_scenes(solr, name):
    k = solr.Kernel(engine="hip")
    k.initialize(width=64, height=48, viewDistance=50000.0)
    plain = k.add_material(0.5, 0.5, 0.5)
    glow = k.add_material(1.0, 1.0, 1.0, innerIllumination=2.0)
    for t, p0, p1, p2, size, lamp in M.SCENES[name](solr):
        k.add_primitive(t, p0, p1 or (0, 0, 0), p2 or (0, 0, 0), size=size, material=glow if lamp else plain)
    k.L.SolRx_HostBuild(1)                      # the host builder's tree is the expectation
    k.compact_boxes(True)
    flat = k.flat_scene()
    boxes, order, nb_lamps, depth, _ = _device_tree(solr, flat, 50000.0)
    _same_tree(boxes, order, nb_lamps, flat)
    k.L.SolRx_HostBuild(0)
    k.finalize()


@pytest.mark.parametrize("scene,kw", [("height_field", dict(n=224)), ("molecule", dict(atoms=50000)),
                                      ("cornell", dict())], ids=["cfg2-mesh", "cfg3-molecule", "cfg1-cornell"])
def test_baseline_scenes(solr, scene, kw):
    k = solr.Kernel(engine="hip")
    k.L.SolRx_HostBuild(1)
    getattr(solr.scenes, scene)(k, width=64, height=48, **kw)
    flat = k.flat_scene()
    si = k.frame_parameters()[0]
    boxes, order, nb_lamps, depth, seconds = _device_tree(solr, flat, si.viewDistance)
    _same_tree(boxes, order, nb_lamps, flat)
    boxes, order, nb_lamps, depth, seconds = _device_tree(solr, flat, si.viewDistance)   # warm: allocations aside
    print("%s: %d primitives, %d nodes, depth %d, device build + copies %.1f ms" % (scene, len(order), len(boxes), depth,
                                                                                   seconds * 1e3))
    k.L.SolRx_HostBuild(0)
    k.finalize()


# ---- the synthetic cases: the raw entry point -------------------------------------------------------------------------------
def _records(solr, spec, move, movable):
    """the case as the Primitive records and emissive flags GPUKernel::buildTreeOnDevice would hand over (the fields the
    builder does not read - normals, texture coordinates - left at zero)"""
    plain, glow = 0, 1
    own = M.records_of(solr, spec, plain, glow, move, movable)
    by_index = np.zeros(len(spec), solr.PRIMITIVE_DTYPE)
    for i, rec in own.items():
        for field in ("p0", "p1", "p2", "size"):
            by_index[field][i] = rec[field]
        by_index["type"][i], by_index["index"][i], by_index["materialId"][i] = rec["type"], i, rec["material"]
    emissive = np.array([1 if s[5] else 0 for s in spec], np.uint8)
    return by_index, emissive


@pytest.mark.parametrize("name", list(K.CASES))
def test_synthetic_cases(solr, name):
    """the model says which way the device must go; where it builds, the host's tree word for word"""
    c = K.CASES[name]
    spec = c.spec(solr)
    model, host_boxes, host_order, host_lights = M._build_both(solr, spec, c.view_distance, move=c.move, capacity=c.capacity,
                                                               movable=c.movable)
    by_index, emissive = _records(solr, spec, c.move, c.movable)
    lo, hi = M.extent_of(spec)                              # the extent the kernel kept: from before the move
    depth, boxes, order, nb_lamps, _ = _build(solr, by_index, emissive, lo, hi, c.view_distance, c.capacity,
                                              model.depth_before)
    message = solr.hip_lib().solr_hip_build_tree_message()
    if model.declined:
        assert depth == -2, (depth, message, model.declined)
        return
    assert depth == model.tree_depth, (depth, message)
    _same_nodes(boxes, host_boxes)
    assert [int(v) for v in order] == host_order and len(order) == len(host_order)
    assert nb_lamps == len(host_lights) and [int(v) for v in order[:nb_lamps]] == host_lights


def test_bad_arguments(solr):
    hip = solr.hip_lib()
    hip.solr_hip_build_tree_message.restype = C.c_char_p
    spec = K.CASES["counts: n = 11, one outer level"].spec(solr)
    by_index, emissive = _records(solr, spec, None, None)
    lo, hi = M.extent_of(spec)
    n = len(spec)
    boxes, order = np.zeros(12 * n + 64, solr.BOX_DTYPE), np.zeros(n, np.int32)
    nb_boxes, nb_lamps = C.c_int(), C.c_int()
    good = [C.c_void_p(by_index.ctypes.data), C.c_void_p(emissive.ctypes.data), n, C.c_void_p(lo.ctypes.data),
            C.c_void_p(hi.ctypes.data), C.c_float(50000.0), C.c_void_p(boxes.ctypes.data), len(boxes),
            C.c_void_p(order.ctypes.data), C.byref(nb_boxes), C.byref(nb_lamps)]
    assert hip.solr_hip_build_tree(*good) == 1
    assert hip.solr_hip_build_tree_message() == b""
    for at, bad in [(2, 0), (2, -5)] + [(i, C.c_void_p(None)) for i in (0, 1, 3, 4, 6, 8, 9, 10)]:
        args = list(good)
        args[at] = bad
        assert hip.solr_hip_build_tree(*args) == -1, at
        assert b"bad arguments" in hip.solr_hip_build_tree_message(), at
    assert hip.solr_hip_build_tree(*good) == 1              # ... and the builder is as before afterwards


# ---- the synthetic cases: the engine's route --------------------------------------------------------------------------------
def _through_the_engine(solr, c, spec, host_build):
    k = solr.Kernel(engine="hip")
    k.initialize(width=64, height=48, viewDistance=c.view_distance)
    plain = k.add_material(0.5, 0.5, 0.5)
    glow = k.add_material(1.0, 1.0, 1.0, innerIllumination=2.0)
    M.add_case(k, spec, plain, glow, c.movable)
    k.L.SolRx_HostBuild(1 if host_build else 0)
    try:
        k.compact_boxes(True)
        rebuilt = k.flat_scene()
        k.compact_boxes(False)                              # the level maps, made lazily after a device build
        again = k.flat_scene()
        # no frame was rendered: the scene is not resident and the rotation runs on the host, over m_hMovable's flags
        k.rotate_primitives(center=(10.0, -20.0, 30.0), angles=(0.3, -0.2, 0.1))
        turned = k.flat_scene()
    finally:
        k.L.SolRx_HostBuild(0)
        k.finalize()
    return rebuilt, again, turned


def _same_bytes(a, b, what):
    """every field of every record, byte for byte (the padding between and behind the fields is nobody's: a record copied
    member by member carries whatever the stack held there)"""
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.shape, b.shape)
    for field in a.dtype.names:
        assert np.ascontiguousarray(a[field]).tobytes() == np.ascontiguousarray(b[field]).tobytes(), (what, field)


@pytest.mark.parametrize("name", K.ENGINE_CASES)
def test_engine_route_is_the_host_route(solr, name):
    c = K.CASES[name]
    spec = c.spec(solr)
    device = _through_the_engine(solr, c, spec, host_build=False)
    host = _through_the_engine(solr, c, spec, host_build=True)
    for step, d, h in zip(("compactBoxes(true)", "compactBoxes(false)"), device, host):
        _same_bytes(d.boxes, h.boxes, step + ": boxes")
        _same_bytes(d.primitives, h.primitives, step + ": primitives")
        _same_bytes(d.lights, h.lights, step + ": lights")
        assert d.nb_lamps == h.nb_lamps, step
    _same_bytes(device[2].primitives, host[2].primitives, "after a rotation: primitives")
    moved = np.any(device[2].primitives["p0"] != device[1].primitives["p0"], axis=1)
    if c.movable is not None:                               # the rotation asked the flags, and they were the host's
        fixed = np.array([not c.movable[i] for i in device[2].primitives["index"]])
        assert not moved[fixed].any() and moved[~fixed & (np.arange(len(moved)) >= device[2].nb_lamps)].all()
