"""Batches and the binary32 model for the tests of primitives set anew (tests/test_edits_host.py, tests/test_edits_gpu.py):
GPUKernel::setPrimitives on the host and on the resident scene (solr_hip_set_primitives, k_setPrimitives).

  batches      per scene three batches of records (solr.EDIT_DTYPE) at the sizes where one thread per edit can go wrong:
               1 edit; 65 edits (a second, ragged wave); 257 edits on the mesh (a second block); every primitive that is no
               lamp.  The lamps come first in the flattened order and are emissive, which the device declines: "the first
               slot" of a batch is the first one behind them, and the batches of 65 and of all hold it and the last slot.
               In every batch one primitive - a round one or a triangle, never a plane that would hide the scene - is put
               on the stage, half way between the camera and what it looks at: outside the old bounds of its leaf
               (outside_old_leaf) and in view, so a refit that did not happen shows in the picture.
  edit_model   what the three setters leave of the flattened primitives: GPUKernel::setPrimitive per type, setPrimitiveNormals
               and setPrimitiveTextureCoordinates by flag, every operation a binary32 step of its own, in their order
  refit_model  move_cases', unchanged: the box updates behind the setters

The scenes are morph_cases' (mesh, sticks, mix: frame 1 of three, flattened), through move_cases.build."""
import importlib

import numpy as np

import move_cases

solr = importlib.import_module("sol-r_amd")

f32 = np.float32
refit_model = move_cases.refit_model
STAGE = {"mesh": (0.0, 2000.0, -7500.0), "sticks": (0.0, 0.0, -7000.0), "mix": (100.0, 150.0, -7000.0)}
# The seeds of the batches' pseudo-random steps.  The GPU tests hold frames to the oracle as pinned - libm's binary32 powf, where
# the engine's is correctly rounded (tests/helpers.py assert_parity_pinned) - at assert_parity's bar of 1 ULP, which has no room
# for a pixel where libm misrounds by more: the seeds are such that the oracle as pinned and the oracle with correctly rounded
# transcendentals agree within that ULP on every frame of the sequences below, which tests/test_edits_host.py checks on the CPU
SEED = {"mesh": 20, "sticks": 0, "mix": 20}
TURNS = [((0.0, 0.0, 0.0), (0.0, 0.02, 0.0)), ((10.0, -20.0, 30.0), (0.11, -0.07, 0.05)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.3))]
TRANSLATIONS = [(300.0, 0.0, -250.5), (-450.0, 120.0, 80.25)]
LAMP_THERE = (-3000.0, 6000.0, -12000.5)
SOLID = (solr.ptSphere, solr.ptCylinder, solr.ptCone, solr.ptEllipsoid, solr.ptTriangle)
# setPrimitiveNormals on a cylinder would replace its axis, on a plane its shading normal: the batches set normals where
# the renderer reads interpolated ones or none at all
NORMALS_FOR = (solr.ptSphere, solr.ptEllipsoid, solr.ptTriangle)


def record(primitive, seed, to=None, flags=0):
    """one record for the flattened primitive: its points pushed by a small pseudo-random step - or so that p0 lands on `to` -,
    its size scaled unevenly (what a type derives from size.x shows), normals and texture coordinates of its own"""
    rng = np.random.RandomState(seed)
    step = rng.uniform(-150.0, 150.0, 3).astype(f32)
    if to is not None:
        step = (np.asarray(to, f32) - primitive["p0"]).astype(f32)
    r = np.zeros(1, solr.EDIT_DTYPE)[0]
    r["index"], r["materialId"], r["flags"] = primitive["index"], primitive["materialId"], flags
    r["p0"] = primitive["p0"] + step if to is None else np.asarray(to, f32)
    r["p1"] = primitive["p1"] + step + rng.uniform(-40.0, 40.0, 3).astype(f32)
    r["p2"] = primitive["p2"] + step + rng.uniform(-40.0, 40.0, 3).astype(f32)
    r["size"] = primitive["size"] * np.array([1.125, 0.875, 1.0625], f32)
    for field in ("n0", "n1", "n2"):
        r[field] = f32(3.0) * primitive[field] + rng.uniform(-0.2, 0.2, 3).astype(f32) + np.array([0.0, -0.5, 0.0], f32)
    for field in ("vt0", "vt1", "vt2"):
        r[field] = rng.uniform(0.0, 1.0, 2).astype(f32)
    return r


def stage(name, seed):
    """where the batch of that seed puts its primitive: a step nearer to the camera and to the right with every seed, so
    that the place is outside the bounds a leaf got from a batch before"""
    x, y, z = STAGE[name]
    return (x + 350.0 * (seed % 5), y, z - 500.0 * (seed % 5))


def records(some):
    """a batch from a list of records"""
    out = np.zeros(len(some), solr.EDIT_DTYPE)
    for n, r in enumerate(some):
        out[n] = r
    return out


def batch_of(flat, name, slots, far, seed):
    """the records for those slots of the flattened order, the primitive of slot `far` put on the stage"""
    p = flat.primitives
    assert far in slots and int(p["type"][far]) in SOLID
    out = np.zeros(len(slots), solr.EDIT_DTYPE)
    for n, slot in enumerate(slots):
        kind = int(p["type"][slot])
        if name == "mesh":
            flags = (solr.EDIT_NORMALS | solr.EDIT_TEXTURE_COORDINATES) if kind == solr.ptTriangle else 0
        else:
            flags = ((solr.EDIT_NORMALS if (n & 1) and kind in NORMALS_FOR else 0) |
                     (solr.EDIT_TEXTURE_COORDINATES if (n & 2) else 0))
        out[n] = record(p[slot], seed * 1000 + n, to=stage(name, seed) if slot == far else None, flags=flags)
    return out


def _last_solid(flat, slots):
    return max(s for s in slots if int(flat.primitives["type"][s]) in SOLID)


def batches(flat, name):
    """the three batches of scene `name`, each against the scene as flattened before the first of them (a record names its
    primitive by index and carries everything that is set, so the batches do not depend on one another)"""
    n, lamps = len(flat.primitives), flat.nb_lamps
    everything = list(range(lamps, n))
    solid = [s for s in everything if int(flat.primitives["type"][s]) in SOLID]
    if name == "mesh":
        assert n == 290 and lamps == 1
        sizes = (65, 257, len(everything))
    elif name == "sticks":
        assert n == 85 and lamps == 1
        sizes = (1, 65, len(everything))
    else:
        sizes = (1, 7, len(everything))
    out = []
    for b, size in enumerate(sizes):
        if size == 1:
            slots = [solid[-1]]
        elif size == len(everything):
            slots = everything[::-1]            # the last slot first: the order of a batch is not the flattened one
        else:
            # the first slot, the last one, and every other slot from the first on until the batch is full
            slots = list(dict.fromkeys([everything[0], everything[-1]] + everything[2::2]))[:size]
            slots += [s for s in everything if s not in slots][:size - len(slots)]
        assert len(slots) == size == len(set(slots))
        far = solid[(3, 10, 76)[b] % len(solid)] if size > 1 else slots[0]      # (three different ones in every scene)
        if far not in slots:
            far = _last_solid(flat, slots)
        out.append(batch_of(flat, name, slots, far, seed=SEED[name] + b + 1))
    return out


def batch_steps(flat, name):
    """the three batches, one after the other"""
    return [("edit", b) for b in batches(flat, name)]


def mixed_steps(flat):
    """the batches of the sticks among rotations, translations and a move of lamp 0: one journal, in order"""
    b = batches(flat, "sticks")
    return [("edit", b[0]), ("rotate", TURNS[0]), ("translate", TRANSLATIONS[0]), ("lamp", (0, LAMP_THERE)), ("edit", b[1]),
            ("rotate", TURNS[1]), ("edit", b[2]), ("translate", TRANSLATIONS[1])]


def long_steps(flat):
    """ten rotations of the mix, more than a store replays without an edit among them, with two batches between them"""
    b = batches(flat, "mix")
    out = []
    for n in range(10):
        out.append(("rotate", TURNS[n % 3]))
        if n in (2, 6):
            out.append(("edit", b[1 + (n > 2)]))
    return out


MIXED_CHECKED = (0, 3, 4, 6, 7)      # the steps of mixed_steps and long_steps whose frames the GPU tests hold to the oracle
LONG_CHECKED = (3, 8, 11)


def apply(k, step, lamps):
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


def far_index(flat, name, batch):
    """the index of the primitive that batch puts on the stage, and where"""
    for seed in range(5):
        there = np.all(batch["p0"] == np.asarray(stage(name, seed), f32), axis=1)
        if there.any():
            assert there.sum() == 1
            return int(batch["index"][there][0]), stage(name, seed)
    raise AssertionError("no primitive on the stage")


def outside_old_leaf(flat, index, p0):
    """does p0 lie outside the bounds the leaf of primitive `index` has in the flattened scene `flat`"""
    slot = int(np.flatnonzero(flat.primitives["index"] == index)[0])
    b = flat.boxes
    leaf = np.flatnonzero((b["nbPrimitives"] > 0) & (b["startIndex"] <= slot) & (slot < b["startIndex"] + b["nbPrimitives"]))
    leaf = leaf[leaf > 0]      # (node 0, the lamps' cell, holds the first slots)
    assert len(leaf) == 1
    p0 = np.asarray(p0, f32)
    return bool(np.any(p0 < b["min"][leaf[0]]) or np.any(p0 > b["max"][leaf[0]]))


def _normalize(v):
    """GPUKernel::normalizeVector on three binary32: division by the length, a zero vector left alone"""
    x, y, z = f32(v[0]), f32(v[1]), f32(v[2])
    length = np.sqrt(f32(f32(x * x + y * y) + z * z))
    if length != 0:
        return np.array([x / length, y / length, z / length], f32)
    return np.array([x, y, z], f32)


def _cross(b, c):
    """GPUKernel::crossProduct"""
    return np.array([f32(b[1] * c[2]) - f32(b[2] * c[1]), f32(b[2] * c[0]) - f32(b[0] * c[2]),
                     f32(b[0] * c[1]) - f32(b[1] * c[0])], f32)


def set_primitive_model(kind, e):
    """GPUKernel::setPrimitive for a primitive of that type with record e's arguments: p0 p1 p2 size n0 n1 n2"""
    p0, p1, p2, size = (np.array(e[field], f32) for field in ("p0", "p1", "p2", "size"))
    zero = np.zeros(3, f32)
    n0, n1, n2 = zero.copy(), zero.copy(), zero.copy()
    if kind == solr.ptSphere:
        size = np.array([size[0]] * 3, f32)
    elif kind in (solr.ptCylinder, solr.ptCone):
        n1 = _normalize((p1 - p0).astype(f32))
        p2 = ((p0 + p1).astype(f32) / f32(2)).astype(f32)
        size = np.array([size[0]] * 3, f32)
    elif kind == solr.ptXYPlane:
        n0 = n1 = n2 = np.array([0, 0, 1], f32)
    elif kind == solr.ptYZPlane:
        n0 = n1 = n2 = np.array([1, 0, 0], f32)
    elif kind in (solr.ptXZPlane, solr.ptCheckboard):
        n0 = n1 = n2 = np.array([0, 1, 0], f32)
    elif kind == solr.ptTriangle:
        v0 = _normalize((p1 - p0).astype(f32))
        v1 = _normalize((p2 - p0).astype(f32))
        n0 = n1 = n2 = _normalize(_cross(v0, v1))
    return p0, p1, p2, size, n0, n1, n2


def edit_model(primitives, batch):
    """what set_primitives(batch) leaves of the flattened primitives: per record, in order, setPrimitive by the primitive's
    type, setPrimitiveNormals' three normalisations with EDIT_NORMALS, the texture coordinates with
    EDIT_TEXTURE_COORDINATES and setPrimitive's zeros without; type and index stay"""
    assert primitives.dtype == solr.PRIMITIVE_DTYPE and batch.dtype == solr.EDIT_DTYPE
    out = primitives.copy()
    slot_of = {int(index): slot for slot, index in enumerate(out["index"])}
    with np.errstate(all="ignore"):
        for e in batch:
            slot = slot_of[int(e["index"])]
            p0, p1, p2, size, n0, n1, n2 = set_primitive_model(int(out["type"][slot]), e)
            vt = [np.zeros(2, f32)] * 3
            if e["flags"] & solr.EDIT_NORMALS:
                n0, n1, n2 = _normalize(e["n0"]), _normalize(e["n1"]), _normalize(e["n2"])
            if e["flags"] & solr.EDIT_TEXTURE_COORDINATES:
                vt = [e["vt0"], e["vt1"], e["vt2"]]
            for field, value in (("p0", p0), ("p1", p1), ("p2", p2), ("size", size), ("n0", n0), ("n1", n1), ("n2", n2),
                                 ("vt0", vt[0]), ("vt1", vt[1]), ("vt2", vt[2])):
                out[field][slot] = value
            out["materialId"][slot] = e["materialId"]
    return out


def by_setters(k, batch):
    """the yardstick through calls that were there before set_primitives: the three setters one record at a time, then a
    translation by (-0, -0, -0) - x + -0 == x bit for bit, for +-0 too, so it contributes its box updates and nothing else -
    which flattens with compactBoxes(false) like every move of the stub"""
    for e in batch:
        index = int(e["index"])
        k.L.SolR_SetPrimitive(index, *[float(c) for field in ("p0", "p1", "p2", "size") for c in e[field]], int(e["materialId"]))
        if e["flags"] & solr.EDIT_NORMALS:
            k.set_normals(index, *[[float(c) for c in e[field]] for field in ("n0", "n1", "n2")])
        if e["flags"] & solr.EDIT_TEXTURE_COORDINATES:
            k.set_texture_coordinates(index, *[[float(c) for c in e[field]] for field in ("vt0", "vt1", "vt2")])
    k.translate_primitives((-0.0, -0.0, -0.0))
