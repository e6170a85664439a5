"""A numpy binary32 model of what the arena holds of a node list beyond its rows (test infrastructure, no test functions):
the thin copy, the copy with sorted bounds, the leaf records - sol-r_amd/csrc/solr_arena.hip k_tightenLeaves,
k_tightenInner, k_sortNodeBounds, k_buildLeafRecords - written from the comments above those kernels and from
scene_layout.h, one function per kernel; and the hand-made node lists the copies are read back for
(tests/test_list_copies_model.py holds the model to its own properties, tests/test_list_copies_gpu.py the engine to the
model, bit for bit; tests/walk_margin_cases.py aims rays at the margins of the same lists).

A node list is an (n, 2, 4) float32 array, scene_layout.h's two rows a node: {min.xyz, max.z} {max.xy, bits(count),
bits(skip)}.  Primitive records are (n, 8, 4) float32 (PRIM_ROWS rows), as solr_hip_read_primitives returns them.
"""
import numpy as np

f4, i4 = np.float32, np.int32

ptSphere, ptCylinder, ptTriangle, ptXYPlane, ptYZPlane, ptXZPlane = 0, 1, 2, 5, 6, 7
KIND_SHIFT, KIND_PLANE_XY, KIND_PLANE_YZ, KIND_PLANE_XZ = 24, 2, 3, 4
ROW_P0_TYPE, ROW_SIZE_MAT, ROW_P1_INDEX, ROW_P2, ROW_N0 = 0, 1, 2, 3, 4
TEXTURE_NONE = -1
BIG = f4(3.0e38)


def fmin(a, b):
    """minNum of two binary32 numbers: the one that is a number when the other is not, -0 below +0"""
    a, b = f4(a), f4(b)
    if np.isnan(a):
        return b
    if np.isnan(b):
        return a
    if a == b:
        return a if np.signbit(a) else b
    return a if a < b else b


def fmax(a, b):
    a, b = f4(a), f4(b)
    if np.isnan(a):
        return b
    if np.isnan(b):
        return a
    if a == b:
        return b if np.signbit(a) else a
    return a if a > b else b


def counts(rows):
    return rows[:, 1, 2].view(i4)


def skips(rows):
    return rows[:, 1, 3].view(i4)


def lo(rows):
    return rows[:, 0, :3]


def hi(rows):
    return np.stack([rows[:, 1, 0], rows[:, 1, 1], rows[:, 0, 3]], axis=1)


def rows_of(boxes):
    """BoundingBox records (sol-r_amd BOX_DTYPE) as node rows"""
    rows = np.zeros((len(boxes), 2, 4), f4)
    rows[:, 0, :3] = boxes["min"]
    rows[:, 0, 3] = boxes["max"][:, 2]
    rows[:, 1, :2] = boxes["max"][:, :2]
    rows[:, 1, 2] = boxes["nbPrimitives"].astype(i4).view(f4)
    rows[:, 1, 3] = np.ascontiguousarray(boxes["indexForNextBox"][:, 0]).astype(i4).view(f4)
    return rows


# ---- what retagPrimitives settles -------------------------------------------------------------------------------------
def extent(prims):
    """the scene's extent: the largest finite |coordinate| of p0 / p1 / p2, at least 1, plus the largest finite |size|
    component (the thin copies' margin is 2^-10 of it)"""
    with np.errstate(invalid="ignore"):
        coords = np.abs(np.concatenate([prims["p0"].ravel(), prims["p1"].ravel(), prims["p2"].ravel()]).astype(f4))
        sizes = np.abs(prims["size"].ravel().astype(f4))
        e = max([f4(1.0)] + [c for c in coords if c < BIG])
        reach = max([f4(0.0)] + [s for s in sizes if s < BIG])
    return f4(f4(e) + f4(reach))


def margin_of(scene_extent):
    return f4(f4(scene_extent) * f4(1.0 / 1024.0))


def plain_kinds(prims, materials):
    """per primitive: KIND_PLANE_XY / _YZ / _XZ for a plain axis plane, 0 for everything else.  Plain: an axis plane whose
    material has no fast transparency (attributes.x == 0), no texture, no wireframe mode 2 - and, a YZ plane, no emission."""
    out = np.zeros(len(prims), i4)
    for i, p in enumerate(prims):
        m = materials[int(p["materialId"])]
        t = int(p["type"]) & 0xff
        if t not in (ptXYPlane, ptYZPlane, ptXZPlane) or int(m["attributes"][0]) != 0:
            continue
        if int(m["textureIds"][0]) != TEXTURE_NONE or int(m["attributes"][2]) == 2:
            continue
        if t == ptYZPlane and float(m["innerIllumination"][0]) != 0.0:
            continue
        out[i] = {ptXYPlane: KIND_PLANE_XY, ptYZPlane: KIND_PLANE_YZ, ptXZPlane: KIND_PLANE_XZ}[t]
    return out


def kinds_of_records(records):
    """the kind the engine wrote into the tag of every primitive record"""
    return (records[:, ROW_P0_TYPE, 3].view(i4) >> KIND_SHIFT) & 15


def records_of(prims, kinds):
    """primitive records as h2d_scene lays them out (scene_layout.h), the kind in the tag and no material facts: what the
    model's functions read of them (p0, size, type, kind, p1, p2, n0, index)"""
    r = np.zeros((len(prims), 8, 4), f4)
    r[:, ROW_P0_TYPE, :3], r[:, ROW_SIZE_MAT, :3] = prims["p0"], prims["size"]
    r[:, ROW_P1_INDEX, :3], r[:, ROW_P2, :3], r[:, ROW_N0, :3] = prims["p1"], prims["p2"], prims["n0"]
    r[:, ROW_P0_TYPE, 3] = ((prims["type"].astype(i4) & 0xff) | (np.asarray(kinds, i4) << KIND_SHIFT)).astype(i4).view(f4)
    r[:, ROW_SIZE_MAT, 3] = prims["materialId"].astype(i4).view(f4)
    r[:, ROW_P1_INDEX, 3] = prims["index"].astype(i4).view(f4)
    return r


# ---- k_tightenLeaves -------------------------------------------------------------------------------------------------
def rectangle_box(p0, size, kind, margin):
    """the box of one plain plane: p0 +- (|size| + margin) in the plane, +- margin across it"""
    across = {KIND_PLANE_XY: 2, KIND_PLANE_YZ: 0, KIND_PLANE_XZ: 1}[int(kind)]
    e = [f4(margin) if a == across else f4(np.abs(f4(size[a])) + f4(margin)) for a in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        return [f4(f4(p0[a]) - e[a]) for a in range(3)], [f4(f4(p0[a]) + e[a]) for a in range(3)]


def _ordered_and_finite(l, h):
    return all(l[a] <= h[a] and np.abs(l[a]) < BIG and np.abs(h[a]) < BIG for a in range(3))


def _cut(row, l, h):
    """bounds l, h cut with the box of a node's rows; None where the result is not ordered"""
    box_lo, box_hi = [row[0, 0], row[0, 1], row[0, 2]], [row[1, 0], row[1, 1], row[0, 3]]
    nl = [fmax(box_lo[a], l[a]) for a in range(3)]
    nh = [fmin(box_hi[a], h[a]) for a in range(3)]
    return (nl, nh) if all(nl[a] <= nh[a] for a in range(3)) else None


def _with_bounds(row, l, h):
    out = row.copy()
    out[0, :3], out[0, 3], out[1, :2] = l, h[2], h[:2]
    return out


def thin_leaves(rows, start, records, kinds, margin):
    """the thin copy, leaves only: a leaf whose primitives are all plain planes becomes the union of their rectangles cut
    with its box; kept as uploaded where that union or the cut is not ordered or not finite; everything else copied"""
    out = rows.copy()
    cnt = counts(rows)
    for i in range(len(rows)):
        nb = int(cnt[i])
        if nb <= 0:
            continue
        mine = range(int(start[i]), int(start[i]) + nb)
        if not all(kinds[k] in (KIND_PLANE_XY, KIND_PLANE_YZ, KIND_PLANE_XZ) for k in mine):
            continue
        l, h = [f4(np.inf)] * 3, [f4(-np.inf)] * 3
        for k in mine:
            rl, rh = rectangle_box(records[k, ROW_P0_TYPE, :3], records[k, ROW_SIZE_MAT, :3], kinds[k], margin)
            l = [fmin(l[a], rl[a]) for a in range(3)]
            h = [fmax(h[a], rh[a]) for a in range(3)]
        if not _ordered_and_finite(l, h):
            continue
        cut = _cut(rows[i], l, h)
        if cut is not None:
            out[i] = _with_bounds(rows[i], *cut)
    return out


# ---- k_tightenInner --------------------------------------------------------------------------------------------------
def thin_inner(thin, list_length):
    """the inner nodes of a thin copy (leaves done): the union of the leaves of its skip interval - clamped to its own list,
    where several lie one behind the other - cut with its own box; as it was where there is no leaf or no ordered result"""
    out = thin.copy()
    cnt, skip = counts(thin), skips(thin)
    for i in range(len(thin)):
        if cnt[i] > 0 or skip[i] <= 1:
            continue
        end = min(i + int(skip[i]), (i // list_length + 1) * list_length)
        l, h = [f4(np.inf)] * 3, [f4(-np.inf)] * 3
        for j in range(i + 1, end):
            if cnt[j] <= 0:
                continue
            l = [fmin(l[a], lo(thin)[j][a]) for a in range(3)]
            h = [fmax(h[a], hi(thin)[j][a]) for a in range(3)]
        cut = _cut(thin[i], l, h)
        if cut is not None:
            out[i] = _with_bounds(thin[i], *cut)
    return out


def thin_copy(rows, start, records, kinds, margin, list_length=None):
    return thin_inner(thin_leaves(rows, start, records, kinds, margin), list_length or len(rows))


# ---- k_sortNodeBounds ------------------------------------------------------------------------------------------------
def sorted_copy(rows, nb):
    """eight lists of nb nodes one behind the other -> their copy with (near, far) bounds per axis for the octant each
    list was flattened for (bit 0: x, 1: y, 2: z negative), the skip word in bytes (32 a node), a zero pad record behind"""
    assert len(rows) == 8 * nb
    out = np.zeros((8 * nb + 1, 2, 4), f4)
    out[:-1] = rows
    octant = np.arange(8 * nb) // nb
    x, y, z = (octant & 1) != 0, (octant & 2) != 0, (octant & 4) != 0
    out[:-1][x, 0, 0], out[:-1][x, 1, 0] = rows[x, 1, 0], rows[x, 0, 0]
    out[:-1][y, 0, 1], out[:-1][y, 1, 1] = rows[y, 1, 1], rows[y, 0, 1]
    out[:-1][z, 0, 2], out[:-1][z, 0, 3] = rows[z, 0, 3], rows[z, 0, 2]
    out[:-1, 1, 3] = (skips(rows) << 5).astype(i4).view(f4)
    return out


def unsorted(sorted_rows, nb):
    """the inverse of sorted_copy (without the pad record)"""
    back = sorted_copy(sorted_rows[:-1], nb)[:-1]       # (the swaps are their own inverse)
    back[:, 1, 3] = (skips(sorted_rows[:-1]) >> 5).astype(i4).view(f4)
    return back


# ---- k_buildLeafRecords ----------------------------------------------------------------------------------------------
def plane_class(ptype):
    return ptype not in (0, 9, 1, 12, 10, 2)     # sphere, environment, cylinder, cone, ellipsoid, triangle


def leaf_records(rows, start, records):
    """one 64-byte line a node: a leaf's first primitive - {p0, tag} {size, material} {p1, index} {p2, start}; of a
    plane-class primitive {n0, index} {average colour, 0, 0, start} in the last two; zeros for an inner node"""
    out = np.zeros((len(rows), 4, 4), f4)
    cnt = counts(rows)
    for i in range(len(rows)):
        if cnt[i] <= 0:
            continue
        r = records[int(start[i])]
        out[i, :4] = r[:4]
        if plane_class(int(r[ROW_P0_TYPE, 3].view(i4)) & 0xff):
            out[i, 2, :3] = r[ROW_N0, :3]
            out[i, 3] = [r[ROW_P2, 3], 0.0, 0.0, 0.0]
        out[i, 3, 3] = i4(start[i]).view(f4)
    return out


# ---- the hand-made lists ---------------------------------------------------------------------------------------------
PLAIN, GLASS, TEXTURED, EMISSIVE, WIRE, LAMP = 0, 1, 2, 3, 4, 5     # material ids of hand_made_materials


def hand_made_materials(dtype):
    """six material records: plain, transparent, textured (4 x 4 texels at offset 0), emissive, wireframe mode 2, the lamp"""
    m = np.zeros(6, dtype)
    m["color"] = [0.7, 0.6, 0.5, 0.0]
    m["specular"] = [0.1, 200.0, 0.0, 0.0]
    m["innerIllumination"] = [0.0, 500000.0, 50000.0, 0.0]
    for key in ("textureIds", "advancedTextureIds"):
        m[key] = TEXTURE_NONE
    m["textureOffset"], m["advancedTextureOffset"] = -1, -1
    m["opacity"][GLASS], m["transparency"][GLASS], m["refraction"][GLASS], m["reflection"][GLASS] = 0.2, 0.6, 1.1, 0.5
    m["textureIds"][TEXTURED, 0] = 0
    m["textureOffset"][TEXTURED, 0] = 0
    m["textureMapping"][TEXTURED] = [4, 4, 0, 3]
    m["innerIllumination"][EMISSIVE, 0] = 0.4
    m["attributes"][WIRE, 2], m["attributes"][WIRE, 3] = 2, 5
    m["innerIllumination"][LAMP, 0] = 2.0
    m["color"][LAMP] = [1.0, 1.0, 1.0, 0.0]
    return m


def texture_atlas():
    rng = np.random.default_rng(5)
    return rng.integers(0, 256, 4 * 4 * 3 + 16).astype(np.uint8)


def _box_of(prims):
    """the box the reference's builder gives a leaf: p0 -+ size of every primitive (the radius in all three axes of a
    sphere), smallest and largest from seeds of +-1e6 - a bound that is no number or lies beyond the seed leaves it"""
    l, h = [f4(1.0e6)] * 3, [f4(-1.0e6)] * 3
    for p in prims:
        size = [p["size"][0]] * 3 if int(p["type"]) == ptSphere else p["size"]
        for a in range(3):
            with np.errstate(invalid="ignore"):
                if f4(p["p0"][a] - size[a]) < l[a]:
                    l[a] = f4(p["p0"][a] - size[a])
                if f4(p["p0"][a] + size[a]) > h[a]:
                    h[a] = f4(p["p0"][a] + size[a])
    return l, h


def _prim(dtype, ptype, p0, size, material):
    p = np.zeros(1, dtype)[0]
    p["type"], p["p0"], p["size"], p["materialId"] = ptype, p0, size, material
    if ptype in (ptXYPlane, ptYZPlane, ptXZPlane):
        p["n0"] = {ptXYPlane: (0, 0, 1), ptYZPlane: (1, 0, 0), ptXZPlane: (0, 1, 0)}[ptype]
        p["n1"] = p["n2"] = p["n0"]
    p["vt1"] = (1.0, 1.0)
    return p


class HandMade:
    """boxes, primitives and the leaf every primitive lies in, with names for the leaves the tests aim at"""

    def __init__(self, boxes, prims, names, lamp):
        self.boxes, self.prims, self.names, self.lamp = boxes, prims, names, lamp


def panels(solr, nodes=None, odd=False, glass=False, opaque=False, seed=3):
    """Leaves of plain axis planes - and of everything a leaf's thin copy has a clause for - under two levels of inner nodes,
    boxes as the reference's builder gives them; the lamp's leaf last.  odd: also the leaves whose bounds are no ordinary
    numbers (an infinite size, a NaN in p0) - such a list is not `ordered`, the engine builds no lists of its own for it.
    nodes: padded with sphere leaves to that many nodes.  glass: two transparent spheres more.  opaque: the textured plane
    takes the wireframe material (nothing then scales a shadow: the shadow walks may take the order-free lists)."""
    P, B = solr.PRIMITIVE_DTYPE, solr.BOX_DTYPE
    rng = np.random.default_rng(seed)
    planes = (ptXYPlane, ptYZPlane, ptXZPlane)

    def plane(t, material=PLAIN, size=None, p0=None):
        p0 = rng.uniform(-5000, 5000, 3).round() if p0 is None else p0
        size = rng.uniform(400, 1800, 3).round() if size is None else size
        return _prim(P, t, p0, size, material)

    def sphere(material=PLAIN, p0=None, radius=None):
        p0 = rng.uniform(-5000, 5000, 3).round() if p0 is None else p0
        return _prim(P, ptSphere, p0, (radius or float(np.round(rng.uniform(200, 700))), 0, 0), material)

    groups = []          # [(name, [primitives]) ...] per group: an inner node over its leaves
    singles = [("plane%d_%d" % (t, n), [plane(t)]) for n in range(4) for t in planes]
    groups.append(singles[:6])
    groups.append(singles[6:])
    twin = plane(ptXYPlane)
    mixed = [("two_a", [plane(ptXYPlane), plane(ptYZPlane)]), ("two_b", [plane(ptXZPlane), plane(ptYZPlane)]),
             ("three_a", [plane(ptXYPlane), plane(ptYZPlane), plane(ptXZPlane)]),
             ("three_b", [plane(ptXZPlane), plane(ptXZPlane), plane(ptXYPlane)]),
             ("plane_sphere", [plane(ptXYPlane), sphere()]), ("sphere_plane", [sphere(), plane(ptYZPlane)]),
             ("twin_a", [twin.copy()]), ("twin_b", [twin.copy()])]
    groups.append(mixed)
    base = plane(ptXYPlane, size=(1500.0, 1500.0, 1500.0))
    special = [("textured", [plane(ptXZPlane, WIRE if opaque else TEXTURED)]), ("emissive_yz", [plane(ptYZPlane, EMISSIVE)]),
               ("emissive_xy", [plane(ptXYPlane, EMISSIVE)]), ("wireframe", [plane(ptXYPlane, WIRE)]),
               ("negative_size", [base, plane(ptXYPlane, size=(-600.0, 500.0, 300.0), p0=base["p0"] + f4(200.0))]),
               ("zero_size", [plane(ptYZPlane, size=(700.0, 0.0, 900.0))]),
               ("zero_across", [plane(ptXZPlane, size=(700.0, 0.0, 900.0))])]
    if odd:
        nan_p0 = rng.uniform(-3000, 3000, 3).round()
        nan_p0[1] = np.nan
        partner = plane(ptXYPlane)
        special += [("infinite_size", [plane(ptXYPlane, size=(np.inf, 500.0, 300.0))]),
                    ("nan_alone", [plane(ptXZPlane, p0=nan_p0)]),
                    ("nan_with_partner", [partner, plane(ptYZPlane, p0=nan_p0)])]
    groups.append(special)
    # three planes the coordinate axes run through (rays with zero direction components can reach them)
    groups.append([("across_z", [plane(ptXYPlane, p0=(100.0, -200.0, 3000.0), size=(1500.0, 1500.0, 1500.0))]),
                   ("across_x", [plane(ptYZPlane, p0=(-3500.0, 150.0, 100.0), size=(1200.0, 1400.0, 1300.0))]),
                   ("across_y", [plane(ptXZPlane, p0=(50.0, -4000.0, -100.0), size=(1600.0, 1000.0, 1100.0))])])
    # four parallel planes a few units apart, a leaf each: hits within a tenth of each other's distance for a ray through them
    groups.append([("stack%d" % n, [plane(ptXYPlane, p0=(-2500.0, 2500.0, -4000.0 + dz), size=(900.0, 900.0, 900.0))])
                   for n, dz in enumerate((43.0, 0.0, 13.0, 3.0))])
    balls = [("sphere%d" % n, [sphere()]) for n in range(4)]
    if glass:
        balls += [("glass%d" % n, [sphere(GLASS, radius=900.0)]) for n in range(2)]
    groups.append(balls)
    lamp = _prim(P, ptSphere, (1500.0, 6500.0, -2500.0), (10.0, 0, 0), LAMP)

    # root { group { leaf ... } ... {empty inner} {inner {empty inner}} {padding} lamp leaf }
    fixed = 1 + sum(1 + len(g) for g in groups) + 1 + 2 + 1
    padding = 0 if nodes is None else nodes - fixed - 1
    assert padding >= 0 or nodes is None
    if nodes is not None:
        groups.append([("pad%d" % n, [sphere(radius=50.0)]) for n in range(padding)])
    prims, rows, names = [], [], {}

    def node(l, h, count, start, skip):
        b = np.zeros(1, B)[0]
        b["min"], b["max"], b["nbPrimitives"], b["startIndex"] = l, h, count, start
        b["indexForNextBox"] = (skip, 0)
        rows.append(b)
        return len(rows) - 1

    def union(first, last):
        with np.errstate(invalid="ignore"):
            l = np.min([rows[j]["min"] for j in range(first, last) if np.isfinite(rows[j]["min"]).all()], axis=0)
            h = np.max([rows[j]["max"] for j in range(first, last) if np.isfinite(rows[j]["max"]).all()], axis=0)
        return l, h

    root = node([0] * 3, [0] * 3, 0, 0, 0)
    for gi, group in enumerate(groups):
        if gi == 3:     # (in the middle of the list) an inner node with nothing below it, and one over only such a node
            where = rng.uniform(-3000, 3000, 3).round()
            node(where - 300, where + 300, 0, 0, 1)
            node(where - 900, where + 900, 0, 0, 2)
            node(where - 500, where + 500, 0, 0, 1)
        inner = node([0] * 3, [0] * 3, 0, 0, 0)
        for name, members in group:
            l, h = _box_of(members)
            if name == "nan_alone":
                l, h = [-4000.0] * 3, [4000.0] * 3          # (the builder's box of it is its seeds, inverted: a box of ours)
            names[name] = node(l, h, len(members), len(prims), 1)
            for p in members:
                p["index"] = len(prims)
                prims.append(p)
        l, h = union(inner + 1, len(rows))
        rows[inner]["min"], rows[inner]["max"], rows[inner]["indexForNextBox"] = l, h, (len(rows) - inner, 0)
    names["lamp"] = node(*_box_of([lamp]), 1, len(prims), 1)
    lamp["index"] = len(prims)
    prims.append(lamp)
    l, h = union(1, len(rows))
    rows[root]["min"], rows[root]["max"], rows[root]["indexForNextBox"] = l, h, (len(rows), 0)
    assert nodes is None or len(rows) == nodes, (len(rows), nodes)
    return HandMade(np.array(rows, B), np.array(prims, P), names, len(prims) - 1)


FOREIGN_SMALLER = ("plane5_0", "plane6_1", "plane7_2", "two_a")
FOREIGN_LARGER = "plane5_3"


def foreign(solr, **kw):
    """panels as another host might upload it: four leaf boxes smaller than their planes' rectangles (a ray through such a
    box can hit the plane beside it), one larger.  The inner nodes still hold their children; the leaves no longer hold
    their primitives."""
    scene = panels(solr, **kw)
    b = scene.boxes
    for name in FOREIGN_SMALLER:
        i = scene.names[name]
        mid, half = (b["min"][i] + b["max"][i]) * f4(0.5), (b["max"][i] - b["min"][i]) * f4(0.5)
        b["min"][i], b["max"][i] = mid - half * f4(0.55), mid + half * f4(0.55)
    i = scene.names[FOREIGN_LARGER]
    parent = max(j for j in range(i) if b["nbPrimitives"][j] == 0 and j + b["indexForNextBox"][j, 0] > i)
    b["min"][i], b["max"][i] = b["min"][parent], b["max"][parent]
    return scene
