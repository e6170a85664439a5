"""Rays aimed at the margins and thresholds the walks' short cuts rest on (test infrastructure: a generator, seeded, no GPU).

rt_device.h's closestHitWalk and shadowWalk do not walk the reference's node list as the reference does: thin copies of
plain-plane leaves (tightRay), the short rays' form of them (tightShort / fatCheck), order-free lists with a distance
cut-off, copies with sorted bounds, the lamp's cut-off of the shadow walks.  Each is argued to give the same bits, from
margins (2^-10 of the scene's extent, 1.0002 + 1e-4 sum|o| / length) and thresholds (|direction|^2 against 0.25, 4, 1e24;
no zero direction component; |origin| <= viewDistance) and a ballot over the wave.  The cases built here put rays ON those:
the edges of rectangles inside and outside the margin, origins at +-viewDistance, direction components of +0, -0 and
denormals, rays of length 0.5, 2, 1e12, hits at the initial bound, lamps a hair before and behind a box's face - in the layout
of oracle.probes.case_closest / case_shadow, so that oracle.probes and tests/engine_probes.py take them unchanged
(tests/test_walk_margins_gpu.py compares; tests/test_walk_margin_cases.py holds this generator to being worth comparing).

The predicates that select a path are restated here (tight_ray, short_tight_lane, long_ray, octant) ONLY to compose waves:
a probe wave is 64 consecutive rays, and a ballot over it decides the path, so every class comes as pure waves, as waves
with exactly one stray lane, and in cases of 64 k + 1 and 64 k + 63 rays.  Nothing here judges a result.
"""
import ctypes as C

import numpy as np

import list_copies_model as M

f4, i4 = np.float32, np.int32
VIEW_DISTANCE = 50000.0
RAY_EPSILON = 0.05
WAVE = 64


# ---- the predicates of rt_device.h, for composing waves ---------------------------------------------------------------
def direction(case_or_origins, targets=None):
    if targets is None:
        case_or_origins, targets = case_or_origins["origins"], case_or_origins["targets"]
    return (targets.astype(f4) - case_or_origins.astype(f4)).astype(f4)


def _dd(d):
    """|d|^2 exactly enough (binary64 of binary32 components), and whether a binary32 evaluation - fused or not - could
    land on the other side of one of the thresholds"""
    dd = (d.astype(np.float64) ** 2).sum(axis=1)
    unsure = np.zeros(len(d), bool)
    for threshold in (0.25, 4.0, 1.0e24, 0.9998):
        unsure |= np.abs(dd - threshold) <= threshold * 2.0 ** -20
    return dd, unsure


def long_ray(d):
    dd, _ = _dd(d)
    return (dd >= 4.0) & (dd <= 1.0e24)


def _framed(o, d, view_distance):
    return (d != 0).all(axis=1) & (np.abs(o) <= f4(view_distance)).all(axis=1)


def tight_ray(o, d, view_distance=VIEW_DISTANCE):
    return long_ray(d) & _framed(o, d, view_distance)


def short_tight_lane(o, d, view_distance=VIEW_DISTANCE):
    dd, _ = _dd(d)
    return (dd >= 0.25) & (dd < 4.0) & _framed(o, d, view_distance)


def octant(d):
    return (d[:, 0] < 0).astype(i4) | ((d[:, 1] < 0).astype(i4) << 1) | ((d[:, 2] < 0).astype(i4) << 2)


def sure(d):
    return ~_dd(d)[1]


PREDICATES = {
    "tight": lambda o, d, vd: tight_ray(o, d, vd),
    "short_tight": lambda o, d, vd: short_tight_lane(o, d, vd),
    "long_only": lambda o, d, vd: long_ray(d) & ~tight_ray(o, d, vd),           # order-free, never the thin copy
    "neither": lambda o, d, vd: ~long_ray(d) & ~short_tight_lane(o, d, vd),
    "long": lambda o, d, vd: long_ray(d),
    "short": lambda o, d, vd: ~long_ray(d),
}


# ---- scenes ------------------------------------------------------------------------------------------------------------
class Scene:
    """hand-made arrays in the shape of oracle.probes.SceneData"""

    def __init__(self, solr, made, view_distance=VIEW_DISTANCE):
        from oracle import loader, probes
        self._loader = loader
        self.made, self.names = made, made.names
        self.boxes, self.prims = made.boxes, made.prims
        self.materials = np.zeros(65506 + 30 + 1, solr.MATERIAL_DTYPE)
        self.materials[:6] = M.hand_made_materials(solr.MATERIAL_DTYPE)
        self.textures = M.texture_atlas()
        self.lights = np.zeros(1, solr.LIGHT_DTYPE)
        self.lights["primitiveId"], self.lights["materialId"] = made.lamp, M.LAMP
        self.lights["location"], self.lights["color"] = made.prims["p0"][made.lamp], (1.0, 1.0, 1.0, 2.0)
        self.nb_lamps = 1
        self.randoms = np.zeros(0, f4)
        self.si = probes._scene_info(viewDistance=view_distance, rayEpsilon=RAY_EPSILON)
        self.ppi = solr.PostProcessingInfo()
        self.kinds = M.plain_kinds(self.prims, self.materials)
        self.extent = M.extent(self.prims)
        self.margin = M.margin_of(self.extent)

    def oracle_scene(self):
        rnd = np.zeros(1, f4)
        self._keep = rnd          # (the oracle's scene holds its address: it must outlive the call)
        return self._loader.OracleScene(self.boxes.ctypes.data, len(self.boxes), self.prims.ctypes.data, len(self.prims),
                                        self.lights.ctypes.data, len(self.lights), self.nb_lamps, self.materials.ctypes.data,
                                        self.textures.ctypes.data, rnd.ctypes.data, len(rnd))

    def rectangles(self):
        """(primitive, leaf, across axis) of every plain plane with a rectangle one can aim at"""
        out = []
        for leaf in np.flatnonzero(self.boxes["nbPrimitives"] > 0):
            for k in range(int(self.boxes["startIndex"][leaf]), int(self.boxes["startIndex"][leaf] + self.boxes["nbPrimitives"][leaf])):
                if self.kinds[k] and np.isfinite(self.prims["p0"][k]).all() and np.isfinite(self.prims["size"][k]).all():
                    across = {M.KIND_PLANE_XY: 2, M.KIND_PLANE_YZ: 0, M.KIND_PLANE_XZ: 1}[int(self.kinds[k])]
                    if (np.delete(self.prims["size"][k], across) > 4 * self.margin).all():
                        out.append((k, int(leaf), across))
        return out


def deep(solr, seed=8):
    """F_DEEP: 1 100 leaves of spheres, triangles and cylinders on a jittered grid under two levels of inner nodes, boxes as
    the reference's builder gives them, no plane (no thin copies: the copies with sorted bounds are walked)"""
    P, B = solr.PRIMITIVE_DTYPE, solr.BOX_DTYPE
    rng = np.random.default_rng(seed)
    prims, rows, names = [], [], {}

    def node(l, h, count, start, skip):
        b = np.zeros(1, B)[0]
        b["min"], b["max"], b["nbPrimitives"], b["startIndex"], b["indexForNextBox"] = l, h, count, start, (skip, 0)
        rows.append(b)
        return len(rows) - 1

    def close(first):
        rows[first]["min"] = np.min([rows[j]["min"] for j in range(first + 1, len(rows))], axis=0)
        rows[first]["max"] = np.max([rows[j]["max"] for j in range(first + 1, len(rows))], axis=0)
        rows[first]["indexForNextBox"] = (len(rows) - first, 0)

    root = node([0] * 3, [0] * 3, 0, 0, 0)
    for ix in range(10):
        slab = node([0] * 3, [0] * 3, 0, 0, 0)
        for iy in range(10):
            row = node([0] * 3, [0] * 3, 0, 0, 0)
            for iz in range(11):
                c = (np.array([ix - 5.0, iy - 5.0, iz - 5.0]) * 1000.0 + rng.uniform(-250, 250, 3)).round(1)
                kind = (ix + iy + iz) % 3
                p = np.zeros(1, P)[0]
                p["materialId"], p["vt1"], p["index"] = M.PLAIN, (1.0, 1.0), len(prims)
                if kind == 0:
                    r = float(np.round(rng.uniform(120, 330)))
                    p["type"], p["p0"], p["size"] = M.ptSphere, c, (r, 0, 0)
                    l, h = c - r, c + r
                elif kind == 1:
                    v = (c + rng.uniform(-320, 320, (3, 3))).round(1).astype(f4)
                    p["type"], p["p0"], p["p1"], p["p2"] = M.ptTriangle, v[0], v[1], v[2]
                    a, b = v[1] - v[0], v[2] - v[0]
                    n = np.cross(a / np.linalg.norm(a), b / np.linalg.norm(b))
                    p["n0"] = p["n1"] = p["n2"] = (n / np.linalg.norm(n)).astype(f4)
                    l, h = v.min(axis=0), v.max(axis=0)
                else:
                    e = (c + rng.uniform(-300, 300, (2, 3))).round(1).astype(f4)
                    w = float(np.round(rng.uniform(40, 110)))
                    axis = e[1] - e[0]
                    p["type"], p["p0"], p["p1"], p["size"] = M.ptCylinder, e[0], e[1], (w, w, w)
                    p["n1"], p["p2"] = (axis / np.linalg.norm(axis)).astype(f4), ((e[0] + e[1]) / f4(2.0)).astype(f4)
                    l, h = e.min(axis=0) - f4(w), e.max(axis=0) + f4(w)
                node(l, h, 1, len(prims), 1)
                prims.append(p)
            close(row)
        close(slab)
    lamp = M._prim(P, M.ptSphere, (2100.0, 7300.0, -3400.0), (10.0, 0, 0), M.LAMP)
    lamp["index"] = len(prims)
    names["lamp"] = node(*M._box_of([lamp]), 1, len(prims), 1)
    prims.append(lamp)
    close(root)
    return M.HandMade(np.array(rows, B), np.array(prims, P), names, len(prims) - 1)


_SCENES = {}


def scene(solr, name):
    """panels, foreign, panels_opaque, panels_glass, deep; `panels@<viewDistance>`: panels under another view distance"""
    name = {"panels@64E": "panels@%r" % float(f4(64.0) * M.extent(M.panels(solr).prims)),
            "panels@64E+": "panels@%r" % float(np.nextafter(f4(64.0) * M.extent(M.panels(solr).prims), f4(np.inf)))}.get(name, name)
    if name not in _SCENES:
        base, _, vd = name.partition("@")
        made = {"panels": lambda: M.panels(solr), "foreign": lambda: M.foreign(solr),
                "panels_opaque": lambda: M.panels(solr, opaque=True),
                "panels_glass": lambda: M.panels(solr, glass=True), "deep": lambda: deep(solr)}[base]()
        _SCENES[name] = Scene(solr, made, float(vd) if vd else VIEW_DISTANCE)
    return _SCENES[name]


# ---- composing waves ---------------------------------------------------------------------------------------------------
class Block:
    """rays of one class; `wants`: the predicate its pure waves satisfy on every lane (None: no claim)"""

    def __init__(self, cls, wants, origins, targets, iteration=None, current=None):
        n = len(origins)
        self.cls, self.wants = cls, wants
        self.origins, self.targets = np.asarray(origins, f4).reshape(n, 3), np.asarray(targets, f4).reshape(n, 3)
        self.iteration = np.zeros(n, i4) if iteration is None else np.asarray(iteration, i4)
        self.current = np.full(n, -2, i4) if current is None else np.asarray(current, i4)

    def take(self, keep):
        return Block(self.cls, self.wants, self.origins[keep], self.targets[keep], self.iteration[keep], self.current[keep])


def compose(scene_name, sc, blocks, strays, rng, stray=False, ragged=0):
    """blocks -> one closest-hit case.  Per block: the rays that surely satisfy its predicate as whole waves (the last one
    filled up with the block's own rays again), the others as waves nothing is claimed of.  stray: one lane of every pure
    wave replaced by a ray that surely fails the predicate.  ragged: the case is cut to a multiple of 64 plus that many."""
    vd = float(sc.si.viewDistance)
    parts, cls, waves = [], [], []          # waves: (class, predicate or None, stray lane or -1)

    def add(block, wants, lanes=None):
        for w in range(0, len(block.origins), WAVE):
            piece = block.take(slice(w, w + WAVE))
            lane = -1
            if wants and stray and len(piece.origins) == WAVE:
                pool = strays[wants]
                lane, pick = int(rng.integers(0, WAVE)), int(rng.integers(0, len(pool.origins)))
                for key in ("origins", "targets", "iteration", "current"):
                    getattr(piece, key)[lane] = getattr(pool, key)[pick]
            parts.append(piece)
            cls.extend([block.cls] * len(piece.origins))
            waves.append((block.cls, wants if len(piece.origins) == WAVE else None, lane))

    for block in blocks:
        if block.wants is None:
            pure = np.zeros(len(block.origins), bool)
        else:
            d = direction(block.origins, block.targets)
            pure = PREDICATES[block.wants](block.origins, d, vd) & sure(d)
        if pure.any():
            keep = np.flatnonzero(pure)
            fill = (-len(keep)) % WAVE
            keep = np.concatenate([keep, keep[:fill] if fill <= len(keep) else np.resize(keep, fill)])
            add(block.take(keep), block.wants)
        if (~pure).any():
            rest = np.flatnonzero(~pure)
            fill = (-len(rest)) % WAVE
            add(block.take(np.concatenate([rest, np.resize(rest, fill)])), None)
    case = dict(name="closest", scene_name=scene_name, scene=sc, si=sc.si,
                origins=np.concatenate([p.origins for p in parts]), targets=np.concatenate([p.targets for p in parts]),
                iteration=np.concatenate([p.iteration for p in parts]), current=np.concatenate([p.current for p in parts]),
                cls=np.array(cls), waves=waves)
    if ragged:
        n = (len(case["origins"]) // WAVE - 1) * WAVE + ragged
        for key in ("origins", "targets", "iteration", "current", "cls"):
            case[key] = np.ascontiguousarray(case[key][:n])
        case["waves"] = waves[: n // WAVE] + [(waves[n // WAVE][0], None, -1)]
    for key in ("origins", "targets", "iteration", "current"):
        case[key] = np.ascontiguousarray(case[key])
    return case


def _unit(rng, n):
    """directions with no small component (every component at least 0.15 of the length)"""
    v = rng.uniform(0.15, 1.0, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _on_rectangles(sc, rng, n, inside=0.8):
    """n points on plain rectangles, within `inside` of their half sizes; returns (points, rectangle indices)"""
    rects = sc.rectangles()
    pick = rng.integers(0, len(rects), n)
    pts = np.empty((n, 3))
    for j, r in enumerate(pick):
        k, _, across = rects[r]
        s = np.abs(sc.prims["size"][k].astype(np.float64)) * inside
        s[across] = 0.0
        pts[j] = sc.prims["p0"][k] + rng.uniform(-1, 1, 3) * s
    return pts, pick


ITERATIONS = [0, 0, 1, 2, 3, 5, 9]


# ---- closest-hit classes on the panels ---------------------------------------------------------------------------------
def edge_blocks(sc, rng):
    """targets on the edges and corners of every plain rectangle: on the edge, one ULP, half a margin, a margin and two
    margins inside and outside it.  `side` (kept next to the rays): -1 inside, 0 on, +1 outside."""
    m = float(sc.margin)
    offsets = [("ulp", -1), ("ulp", 1), 0.0, -m / 2, m / 2, -m, m, -2 * m, 2 * m]
    origins, targets, side = [], [], []
    for k, leaf, across in sc.rectangles():
        p0, size = sc.prims["p0"][k].astype(f4), np.abs(sc.prims["size"][k].astype(f4))
        u, v = [a for a in range(3) if a != across]
        for su, sv in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)):
            for off in offsets:
                t = p0.copy()
                for axis, s in ((u, su), (v, sv)):
                    if s == 0:
                        t[axis] = p0[axis] + f4(rng.uniform(-0.8, 0.8)) * size[axis]
                    elif isinstance(off, tuple):
                        edge = f4(p0[axis] + f4(s) * size[axis])
                        t[axis] = np.nextafter(edge, f4(np.inf) * f4(s * off[1]))
                    else:
                        t[axis] = f4(p0[axis] + f4(s) * f4(size[axis] + f4(off)))
                reach = rng.choice([rng.uniform(30, 400), rng.uniform(400, 9000), rng.uniform(9000, 30000)])
                origins.append(t.astype(np.float64) - _unit(rng, 1)[0] * reach)
                targets.append(t)
                side.append(0 if off == 0.0 else (off[1] if isinstance(off, tuple) else int(np.sign(off))))
    n = len(origins)
    block = Block("edges", "tight", origins, targets, rng.choice(ITERATIONS, n))
    block.side = np.array(side)
    return [block]


def frame_blocks(sc, rng, n=384):
    """origins with a coordinate at +-viewDistance (the thin copy's last ray) and one step beyond it"""
    vd = f4(sc.si.viewDistance)
    blocks = []
    for label, value, wants in (("at_view_distance", vd, "tight"), ("beyond_view_distance", np.nextafter(vd, f4(np.inf)), "long_only")):
        pts, _ = _on_rectangles(sc, rng, n)
        o = rng.uniform(-5000, 5000, (n, 3))
        axis = rng.integers(0, 3, n)
        o[np.arange(n), axis] = rng.choice([-1.0, 1.0], n) * float(value)
        aim = np.where(rng.random((n, 1)) < 0.6, pts, rng.uniform(-9000, 9000, (n, 3)))
        t = o + (aim - o) * rng.uniform(0.3, 1.5, (n, 1))
        blocks.append(Block(label, wants, o, t, rng.choice([0, 0, 0, 1, 1, 2], n)))
    return blocks


def zero_component_blocks(sc, rng, n=320):
    """direction components of +0, -0, +-1e-30 and +-1e-38 (a denormal) on one or two axes: the origin is 0 on those axes
    (target - origin is then the target's component, sign and all); the other components aim at the planes the axes run
    through, or past them"""
    blocks = []
    for label, values, wants in (("zero_components", [0.0, -0.0], "long_only"),
                                 ("tiny_components", [1e-30, -1e-30, 1e-38, -1e-38], "tight")):
        o = rng.uniform(-6000, 6000, (n, 3))
        t = rng.uniform(-6000, 6000, (n, 3))
        for j in range(n):
            axes = rng.choice(3, rng.choice([1, 1, 2]), replace=False)
            free = [a for a in range(3) if a not in axes]
            name = {0: "across_x", 1: "across_y", 2: "across_z"}[free[0]] if len(free) == 1 else \
                rng.choice(["across_x", "across_y", "across_z"])
            k = int(sc.boxes["startIndex"][sc.names[name]])
            if rng.random() < 0.5:          # through that plane
                t[j] = sc.prims["p0"][k] + rng.uniform(-0.9, 0.9, 3) * np.abs(sc.prims["size"][k])
                across = {"across_x": 0, "across_y": 1, "across_z": 2}[name]
                t[j, across] = sc.prims["p0"][k][across]
                o[j] = t[j] + rng.uniform(-1, 1, 3) * 5000
            o[j, axes], t[j, axes] = 0.0, rng.choice(values, len(axes))
            grow = rng.uniform(0.4, 2.5)
            for a in free:
                t[j, a] = o[j, a] + (t[j, a] - o[j, a]) * grow
        blocks.append(Block(label, wants, o, t, rng.choice(ITERATIONS, n)))
    return blocks


def box_face_blocks(sc, rng, per_rectangle=12):
    """a zero direction component on an axis IN a rectangle's plane, the ray's coordinate on that axis at the far face of
    the leaf's box minus the crossing parameter, give or take a margin: the reference gives a zero component the reciprocal
    1, its slab test then compares `face - coordinate` with the crossing parameter - a hit inside the rectangle that the
    reference's own box lets in or keeps out by that comparison, which only the reference's own boxes reproduce"""
    m = float(sc.margin)
    origins, targets = [], []
    for k, leaf, across in sc.rectangles():
        if sc.boxes["nbPrimitives"][leaf] != 1:
            continue
        p0, size = sc.prims["p0"][k].astype(np.float64), np.abs(sc.prims["size"][k].astype(np.float64))
        for _ in range(per_rectangle):
            a = int(rng.choice([x for x in range(3) if x != across]))
            b = 3 - a - across
            t = p0.copy()
            t[a] = p0[a] + size[a] - 1.0 + rng.uniform(-m, m)          # (the crossing is at parameter 1: the target)
            t[b] = p0[b] + rng.uniform(-0.8, 0.8) * size[b]
            u = rng.uniform(0.2, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
            u[a] = 0.0
            o = t - u / np.linalg.norm(u) * rng.uniform(30, 3000)
            o[a] = t[a] = f4(t[a])
            origins.append(o), targets.append(t)
    return [Block("zero_component_at_a_box_face", "long_only", origins, targets, rng.choice([0, 0, 1], len(origins)))]


LENGTHS = [0.25, 0.5, 0.95, 1.0 - RAY_EPSILON, 1.0, float(np.nextafter(f4(2.0), f4(0.0))), 2.0, 1.0e12, 2.0e12]


def length_blocks(sc, rng, per_length=128):
    """rays of the lengths the predicates split at, started a little in front of a rectangle (as a bounce ray is) or
    anywhere; the three lengths that ARE thresholds (0.5, 2, 1e12) also along an axis, where |d|^2 is exact"""
    blocks = []
    for length in LENGTHS:
        pts, _ = _on_rectangles(sc, rng, per_length, inside=1.5)         # (some past the rectangle's edge)
        u = _unit(rng, per_length)
        back = np.where(rng.random((per_length, 1)) < 0.5, rng.uniform(0.02, 3.0, (per_length, 1)), rng.uniform(3.0, 3000.0, (per_length, 1)))
        o = (pts - u * back).astype(f4)
        if length >= 1e12:
            o = o.round()
        t = o.astype(np.float64) + u * length
        dd = length * length
        wants = "short_tight" if 0.25 < dd < 4.0 else ("tight" if 4.0 < dd < 1e24 else ("neither" if dd < 0.25 or dd > 1e24 else None))
        blocks.append(Block("length_%g" % length, wants, o, t, rng.choice(ITERATIONS, per_length)))
    for length, wants in ((0.5, "neither"), (2.0, "long_only"), (1.0e12, "long_only")):     # exact: 0.25, 4, 1e24
        n = 64
        pts, _ = _on_rectangles(sc, rng, n)
        axis, sign = rng.integers(0, 3, n), rng.choice([-1.0, 1.0], n)
        o = pts.round()
        o[np.arange(n), axis] -= sign * rng.uniform(0.1, 1.5, n).round(2) * min(length, 64.0)
        o = o.astype(f4)
        t = o.copy()
        t[np.arange(n), axis] = (o[np.arange(n), axis].astype(np.float64) + sign * length).astype(f4)
        d = direction(o, t)
        exact = (np.abs(d[np.arange(n), axis].astype(np.float64)) == length) | (length >= 1e12)
        blocks.append(Block("axis_length_%g" % length, None if length >= 1e12 else wants, o[exact], t[exact],
                            rng.choice(ITERATIONS, int(exact.sum()))))
    # |d|^2 within a few ULP of 4 and of 0.25, general directions: whichever way the sum is rounded, both sides are here
    for length in (2.0, 0.5):
        n = 128
        pts, _ = _on_rectangles(sc, rng, n, inside=1.5)
        u = _unit(rng, n)
        o = (pts - u * rng.uniform(0.05, 1.5, (n, 1)) * length).astype(f4)
        t = o.astype(np.float64) + u * length * (1.0 + rng.integers(-6, 7, (n, 1)) * 2.0 ** -24)
        blocks.append(Block("near_length_%g" % length, None, o, t, rng.choice(ITERATIONS, n)))
    return blocks


def box_blocks(sc, rng, n=256):
    """origins inside a leaf's box, on one of its faces, on one of its corners"""
    leaves = np.flatnonzero(sc.boxes["nbPrimitives"] > 0)
    leaves = leaves[np.isfinite(sc.boxes["min"][leaves]).all(axis=1) & np.isfinite(sc.boxes["max"][leaves]).all(axis=1)]
    pick = rng.choice(leaves, n)
    lo, hi = sc.boxes["min"][pick].astype(np.float64), sc.boxes["max"][pick].astype(np.float64)
    o = lo + (hi - lo) * rng.uniform(0.05, 0.95, (n, 3))
    where = rng.integers(0, 3, n)                 # 0 inside, 1 on a face, 2 on a corner
    face_axis, side = rng.integers(0, 3, n), rng.integers(0, 2, (n, 3))
    corner = np.where(side == 0, lo, hi)
    on_face = where == 1
    o[on_face, face_axis[on_face]] = corner[on_face, face_axis[on_face]]
    o[where == 2] = corner[where == 2]
    pts, _ = _on_rectangles(sc, rng, n)
    aim = np.where(rng.random((n, 1)) < 0.4, pts, rng.uniform(-9000, 9000, (n, 3)))
    return [Block("origins_on_boxes", "tight", o, o + (aim - o) * rng.uniform(0.5, 1.5, (n, 1)), rng.choice(ITERATIONS, n))]


def tie_blocks(sc, rng, n=128):
    """two equal planes in different leaves: a tie in distance on every hit (the smaller flattened index wins)"""
    k = int(sc.boxes["startIndex"][sc.names["twin_a"]])
    p0, size = sc.prims["p0"][k].astype(np.float64), np.abs(sc.prims["size"][k].astype(np.float64))
    t = p0 + rng.uniform(-1.5, 1.5, (n, 3)) * size
    t[:, 2] = p0[2]
    o = t - _unit(rng, n) * rng.uniform(50, 9000, (n, 1))
    return [Block("ties", "tight", o, t, rng.choice(ITERATIONS, n))]


def bound_blocks(sc, rng, per_iteration=32):
    """hits at the initial bound - viewDistance, viewDistance / (iteration + 1) from the third bounce on - and a few ULP to
    either side of it, for every iteration 0 ... 9"""
    origins, targets, iteration = [], [], []
    vd = f4(sc.si.viewDistance)
    for it in range(10):
        bound = float(vd if it < 2 else vd / f4(it + 1))
        pts, _ = _on_rectangles(sc, rng, per_iteration, inside=0.5)
        u = _unit(rng, per_iteration)
        steps = rng.integers(-4, 5, (per_iteration, 1))
        o = pts - u * bound * (1.0 + steps * 2.0 ** -23)
        origins.append(o)
        targets.append(o + u * bound * rng.uniform(0.2, 1.2, (per_iteration, 1)))
        iteration.append(np.full(per_iteration, it))
    return [Block("initial_bound", "tight", np.concatenate(origins), np.concatenate(targets), np.concatenate(iteration))]


def rival_blocks(sc, rng, per_length=128):
    """short rays through the stack of parallel planes, from either side: the nearest hit has rivals within a tenth of its
    distance, in leaves that come earlier and later in the list (what the short rays' widened cut-off must not hide)"""
    k = int(sc.boxes["startIndex"][sc.names["stack1"]])
    p0, size = sc.prims["p0"][k].astype(np.float64), np.abs(sc.prims["size"][k].astype(np.float64))
    blocks = []
    for length in (0.5001, 0.95, 1.0, 1.9):
        n = per_length
        through = p0 + rng.uniform(-1.7, 1.7, (n, 3)) * size
        through[:, 2] = p0[2] + rng.uniform(-5, 50, n)
        u = _unit(rng, n)
        o = through - u * rng.uniform(60, 1500, (n, 1))
        blocks.append(Block("rivals_%g" % length, "short_tight", o, o + u * length, rng.choice([0, 0, 1, 2, 3], n)))
    return blocks


def _stray_pools(sc, rng, n=64):
    """for every predicate, rays that surely fail it (and are rays of the scene like the others)"""
    pts, _ = _on_rectangles(sc, rng, n)
    u = _unit(rng, n)
    o = (pts - u * rng.uniform(50, 4000, (n, 1))).astype(f4)
    long_rays = Block("stray", None, o, o + (pts - o) * 1.2)
    short_rays = Block("stray", None, o, o.astype(np.float64) + u * 0.95)
    flat = o.copy()
    flat[:, 0] = 0.0
    flat_t = (flat + (pts - flat) * 1.2).astype(f4)
    flat_t[:, 0] = 0.0
    in_plane = Block("stray", None, flat, flat_t)                 # long, a zero component: never the thin copy
    return {"tight": in_plane, "short_tight": long_rays, "long_only": short_rays, "neither": long_rays, "long": short_rays,
            "short": long_rays}


def closest_cases(solr, scene_name, seed=31):
    """the closest-hit cases of a scene of panels: {composition: case}"""
    sc = scene(solr, scene_name)
    rng = np.random.default_rng(seed)
    blocks = (edge_blocks(sc, rng) + frame_blocks(sc, rng) + zero_component_blocks(sc, rng) + box_face_blocks(sc, rng) +
              length_blocks(sc, rng) +
              box_blocks(sc, rng) + tie_blocks(sc, rng) + bound_blocks(sc, rng) + rival_blocks(sc, rng))
    mats = np.array([M.PLAIN, M.GLASS, M.EMISSIVE])
    for b in blocks:
        n = len(b.origins)
        b.current = np.where(rng.random(n) < 0.7, -2, rng.choice(mats, n)).astype(i4)
    strays = _stray_pools(sc, rng)
    if "@" in scene_name:         # another view distance: the classes that depend on it
        blocks = [b for b in blocks if b.cls in ("edges", "at_view_distance", "beyond_view_distance", "initial_bound")]
        return {"pure": compose(scene_name, sc, blocks, strays, rng)}
    return {"pure": compose(scene_name, sc, blocks, strays, rng),
            "one_stray": compose(scene_name, sc, blocks, strays, rng, stray=True),
            "ragged_1": compose(scene_name, sc, blocks[1:4], strays, rng, ragged=1),
            "ragged_63": compose(scene_name, sc, blocks[1:4], strays, rng, stray=True, ragged=63)}


# ---- direction components of +-0 and denormals in waves of ONE octant (the deep list) ----------------------------------
def _tiny(rng, negative):
    """a component the octant test (d < 0) counts as positive - +0, -0, 1e-30, a denormal - or as negative"""
    return float(rng.choice([-1e-30, -1e-38]) if negative else rng.choice([0.0, -0.0, 1e-30, 1e-38]))


def _at_zero(sc, rng, axis, inside):
    """a point of an opaque sphere that a coordinate plane runs through, its coordinate on `axis` exactly 0: on the surface
    (inside = 1) or nearer the centre; the sphere's primitive"""
    spheres = np.flatnonzero((sc.prims["type"] == M.ptSphere) & (sc.prims["materialId"] == M.PLAIN) &
                             (np.abs(sc.prims["p0"][:, axis]) < 0.9 * sc.prims["size"][:, 0]))
    k = int(rng.choice(spheres))
    c, r = sc.prims["p0"][k].astype(np.float64), float(sc.prims["size"][k][0])
    v = rng.normal(size=3)
    v[axis] = 0.0
    p = c + v / np.linalg.norm(v) * np.sqrt(r * r - c[axis] ** 2) * inside
    p[axis] = 0.0
    return p, k


def _octant_direction(rng, signs):
    """a direction of the octant `signs` with one component left to a tiny value (axis a1) and, where the octant allows a
    +0 there, sometimes a second one that is exactly zero (a2, else -1)"""
    a1 = int(rng.integers(0, 3))
    others = [a for a in range(3) if a != a1 and signs[a] > 0]
    a2 = int(rng.choice(others)) if others and rng.random() < 0.4 else -1
    u = rng.uniform(0.15, 1.0, 3) * signs
    u[a1] = 0.0
    if a2 >= 0:
        u[a2] = 0.0
    return u / np.linalg.norm(u), a1, a2


def tiny_octant_block(sc, rng, waves=8):
    """closest-hit rays, every wave of one octant, every direction with one or two components of +0, -0, +-1e-30, +-1e-38:
    the origin is 0 on that axis (target - origin is then the target's component, sign and all; an exact zero on a second
    axis comes from equal coordinates).  The octant a wave's list is picked by is (d < 0) per axis, the reciprocal of a
    zero component is 1: the copy with sorted bounds is walked by rays whose sign and reciprocal say different things"""
    origins, targets = [], []
    for w in range(waves):
        signs = np.array([1.0 if (w >> b) & 1 else -1.0 for b in range(3)])
        for _ in range(WAVE):
            u, a1, a2 = _octant_direction(rng, signs)
            if rng.random() < 0.3:
                aim, _ = _at_zero(sc, rng, a1, rng.uniform(0.0, 0.9))
            else:
                aim = rng.uniform(-9000, 9000, 3)
                aim[a1] = 0.0
            o = (aim - u * rng.uniform(300, 4000)).astype(f4)
            t = (o.astype(np.float64) + (aim - o) * rng.uniform(0.5, 1.5)).astype(f4)
            o[a1], t[a1] = 0.0, _tiny(rng, signs[a1] < 0)
            if a2 >= 0:
                t[a2] = o[a2]
            origins.append(o), targets.append(t)
    return Block("one_octant_tiny_components", "long", origins, targets, rng.choice(ITERATIONS, len(origins)))


def tiny_octant_shadows(sc, rng, n):
    """the same for shadow rays: points on spheres with a coordinate of exactly 0, every wave's lamps in one octant, the
    lamp's coordinate on that axis +0, -0, +-1e-30 or +-1e-38 (the reversed loop over the sorted copy)"""
    pts, prim, lamps = np.zeros((n, 3), f4), np.zeros(n, i4), np.zeros((n, 3), f4)
    for j in range(n):
        if j % WAVE == 0:
            signs = rng.choice([-1.0, 1.0], 3)
        u, a1, a2 = _octant_direction(rng, signs)
        p, prim[j] = _at_zero(sc, rng, a1, 1.0)
        pts[j] = p
        lamps[j] = (pts[j].astype(np.float64) + u * rng.uniform(3000, 16000)).astype(f4)
        pts[j, a1], lamps[j, a1] = 0.0, _tiny(rng, signs[a1] < 0)
        if a2 >= 0:
            lamps[j, a2] = pts[j, a2]
    return pts, prim, lamps


# ---- closest-hit classes on the deep list ------------------------------------------------------------------------------
def deep_cases(solr, seed=37):
    """waves of one octant (the copy with sorted bounds), of two octants (the generic loop), waves of one octant whose
    directions carry components of +-0 and denormals, and short rays with a rival hit within D / L (the checked form of the order-free walk and its second walk)"""
    sc = scene(solr, "deep")
    rng = np.random.default_rng(seed)
    centres = sc.prims["p0"][:-1].astype(np.float64)
    blocks = []

    def towards(n, signs):
        u = np.abs(_unit(rng, n)) * signs
        aim = centres[rng.integers(0, len(centres), n)] + rng.normal(size=(n, 3)) * 150.0
        o = aim - u * rng.uniform(300, 14000, (n, 1))
        return o, o + (aim - o) * rng.uniform(0.5, 1.5, (n, 1))

    one_o, one_t, two_o, two_t = [], [], [], []
    for w in range(16):
        signs = np.array([1 if (w >> b) & 1 else -1 for b in range(3)], float)
        o, t = towards(WAVE, signs)
        one_o.append(o), one_t.append(t)
        o, t = towards(WAVE, signs)
        flip = rng.random(WAVE) < 0.5
        flip[0] = False
        o2, t2 = towards(WAVE, -signs)
        two_o.append(np.where(flip[:, None], o2, o)), two_t.append(np.where(flip[:, None], t2, t))
    n = 16 * WAVE
    blocks.append(Block("one_octant", "long", np.concatenate(one_o), np.concatenate(one_t), rng.choice(ITERATIONS, n)))
    blocks.append(Block("two_octants", "long", np.concatenate(two_o), np.concatenate(two_t), rng.choice(ITERATIONS, n)))
    blocks.append(tiny_octant_block(sc, rng))
    # short rays: from a little in front of one primitive towards it, with a neighbour's surface about as far away
    for length in (0.5001, 0.95, 1.0, 1.5, 1.9):
        n = 192
        u = _unit(rng, n)
        aim = centres[rng.integers(0, len(centres), n)] + rng.normal(size=(n, 3)) * 60.0
        o = aim - u * rng.uniform(20, 1500, (n, 1))
        blocks.append(Block("short_%g" % length, "short", o, o + u * length, rng.choice(ITERATIONS, n)))
    strays = _stray_pools_deep(sc, rng)
    return {"pure": compose("deep", sc, blocks, strays, rng), "one_stray": compose("deep", sc, blocks, strays, rng, stray=True),
            "ragged_1": compose("deep", sc, blocks[:1] + blocks[2:3] + blocks[4:5], strays, rng, ragged=1),
            "ragged_63": compose("deep", sc, blocks[:1] + blocks[2:3] + blocks[4:5], strays, rng, ragged=63)}


def _stray_pools_deep(sc, rng, n=64):
    centres = sc.prims["p0"][:-1].astype(np.float64)
    u = _unit(rng, n)
    aim = centres[rng.integers(0, len(centres), n)]
    o = aim - u * rng.uniform(300, 3000, (n, 1))
    return {"long": Block("stray", None, o, o + u * 0.95), "short": Block("stray", None, o, o + (aim - o) * 1.3)}


def same_octant_waves(case):
    """per wave of a case: do all its rays share one octant?"""
    oc = octant(direction(case))
    n = len(oc)
    return np.array([len(set(oc[w:w + WAVE].tolist())) == 1 for w in range(0, n, WAVE)])


# ---- shadow cases ------------------------------------------------------------------------------------------------------
def _surface_points(sc, rng, n):
    """points on the scene's surfaces with the primitive they lie on, found with the oracle's own closest-hit walk"""
    from oracle import loader
    L = loader.lib()
    lo, hi = -7000.0, 7000.0
    m = 4 * n
    origins = rng.uniform(lo, hi, (m, 3)).astype(f4)
    targets = rng.uniform(lo, hi, (m, 3)).astype(f4)
    hit, prim = np.zeros(m, i4), np.zeros(m, i4)
    inter, normal, areas = np.zeros((m, 3), f4), np.zeros((m, 3), f4), np.zeros((m, 3), f4)
    osc = sc.oracle_scene()
    zero, nobody = np.zeros(m, i4), np.full(m, -2, i4)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    L.oracle_probe_closest(m, C.byref(osc), C.byref(sc.si), p(origins), p(targets), p(zero), p(nobody), p(hit), p(prim),
                           p(inter), p(normal), p(areas))
    keep = np.flatnonzero((hit != 0) & (prim != sc.made.lamp) & np.isfinite(inter).all(axis=1))[:n]
    assert len(keep) == n, (len(keep), n)
    return inter[keep], prim[keep]


FACE_PARAMETERS = [1 - 1e-3, 1 - 1e-4, 1.0, 1 + 1e-4, 1.0002, 1 + 3e-4, 1.01]


SURFACE_PARAMETERS = [0.981, 0.999, 0.9999, 1.0, 1.0001, 1.001, 1.02, 1.1]


def shadow_cases(solr, scene_name, seed=41, per_class=256):
    """shadow rays point -> lamp with the lamp placed against the walk's cut-off: {composition: case}.  Every case names the
    primitive its point lies on (`shaded`): the engine is probed the way the renderer calls the walk."""
    sc = scene(solr, scene_name)
    rng = np.random.default_rng(seed + len(scene_name))
    leaves = np.flatnonzero(sc.boxes["nbPrimitives"] > 0)
    leaves = leaves[(leaves != sc.names["lamp"]) & np.isfinite(sc.boxes["min"][leaves]).all(axis=1) &
                    np.isfinite(sc.boxes["max"][leaves]).all(axis=1)]
    blocks = {}

    def points(n):
        return _surface_points(sc, rng, n)

    # a leaf's box face at parameter p along point -> lamp: the lamp a hair before and behind the face
    n = per_class * 2
    pts, prim = points(n)
    lamps = np.empty((n, 3))
    for j in range(n):
        for _ in range(50):
            leaf = rng.choice(leaves)
            lo, hi = sc.boxes["min"][leaf].astype(np.float64), sc.boxes["max"][leaf].astype(np.float64)
            through = lo + (hi - lo) * rng.uniform(0.05, 0.95, 3)
            d = through - pts[j]
            with np.errstate(divide="ignore", invalid="ignore"):
                t0, t1 = (lo - pts[j]) / d, (hi - pts[j]) / d
            near = np.minimum(t0, t1).max()          # the ray enters the box at pts + near * d
            if near > 0.05 and np.linalg.norm(d) * near > 4.0:
                break
        lamps[j] = pts[j] + d * near / FACE_PARAMETERS[j % len(FACE_PARAMETERS)]
    blocks["face_at_the_cut_off"] = (pts, prim, lamps)
    solid = np.flatnonzero(sc.prims["type"] == M.ptSphere)
    solid = solid[(solid != sc.made.lamp) & (sc.prims["materialId"][solid] != M.GLASS)]

    def on_spheres(n, above):
        """points `above` the surface of opaque spheres (negative: below it), the sphere, the outward direction"""
        k = rng.choice(solid, n)
        u = _unit(rng, n)
        c, r = sc.prims["p0"][k].astype(np.float64), sc.prims["size"][k][:, :1].astype(np.float64)
        return c + u * (r + above), k, u, c

    # the lamp a hair behind a surface, and a hair in front of it: a hit at parameter p along point -> lamp, in a leaf that is
    # entered just before it
    n = per_class * 2
    pts, prim = points(n)
    candidates = points(n)[0].astype(np.float64)
    pick = rng.integers(0, n, (n, 8))           # of eight other surface points the nearest: short rays, little else in between
    far = np.linalg.norm(candidates[pick] - pts[:, None, :].astype(np.float64), axis=2)
    far[far < 10.0] = np.inf
    surface = candidates[pick[np.arange(n), far.argmin(axis=1)]]
    behind = np.array([SURFACE_PARAMETERS[j % len(SURFACE_PARAMETERS)] for j in range(n)])[:, None]
    blocks["lamp_behind_a_surface"] = (pts, prim, pts + (surface - pts) / behind)
    # lamps less than 2 away from the point (the order-free path is refused, the lane keeps the reference's cut-off alone):
    # around points on surfaces, and across the surface of a sphere from points half a unit above it
    half = per_class // 2
    pts, prim = points(half)
    lamps = pts + _unit(rng, half) * rng.choice([0.3, 0.95, 1.5, 1.99, 2.01], (half, 1))
    above, k, u, c = on_spheres(per_class - half, 0.5)
    below = above - u * rng.choice([0.8, 0.95, 1.5, 1.99], (per_class - half, 1))
    blocks["lamp_within_2"] = (np.concatenate([pts, above]), np.concatenate([prim, np.full(len(k), sc.made.lamp)]),
                               np.concatenate([lamps, below]))
    # every wave's lamps in the octant opposite to its first lane's and in its own (the reversed sorted loop, or not)
    pts, prim = points(per_class)
    lamps = np.empty((per_class, 3))
    for w in range(0, per_class, WAVE):
        signs = rng.choice([-1.0, 1.0], 3)
        lamps[w:w + WAVE] = pts[w:w + WAVE] + np.abs(_unit(rng, len(pts[w:w + WAVE]))) * signs * rng.uniform(2000, 16000, (len(pts[w:w + WAVE]), 1))
    blocks["one_octant"] = (pts, prim, lamps)
    if scene_name == "deep":
        blocks["one_octant_tiny_components"] = tiny_octant_shadows(sc, rng, per_class)
    # lamps inside an occluder: seen from points elsewhere, and from points on that very occluder (which the walk leaves out)
    pts, prim = points(half)
    own, k, u, c = on_spheres(per_class - half, 0.0)
    inside = np.concatenate([on_spheres(half, 0.0)[3], c]) + rng.normal(size=(per_class, 3)) * 20.0
    blocks["lamp_inside_an_occluder"] = (np.concatenate([pts, own]), np.concatenate([prim, k]), inside)
    # a zero component in point -> lamp (the lamp takes the point's coordinate)
    pts, prim = points(per_class)
    lamps = pts + _unit(rng, per_class) * rng.uniform(2000, 16000, (per_class, 1))
    axes = rng.integers(0, 3, per_class)
    lamps = lamps.astype(f4)
    lamps[np.arange(per_class), axes] = pts[np.arange(per_class), axes]
    blocks["zero_component"] = (pts, prim, lamps)
    # the scene's own lamp and lamps around it, far lamps: the ordinary shadow rays
    pts, prim = points(per_class)
    lamp = sc.lights["location"][0].astype(np.float64) + rng.normal(size=(per_class, 3)) * 40.0
    far = rng.random(per_class) < 0.3
    lamp[far] = rng.uniform(-9000, 9000, (int(far.sum()), 3))
    blocks["around_the_lamp"] = (pts, prim, lamp)

    def case_of(names, stray=False, ragged=0):
        o = np.concatenate([blocks[k][0] for k in names]).astype(f4)
        shaded = np.concatenate([blocks[k][1] for k in names]).astype(i4)
        lamps = np.concatenate([blocks[k][2] for k in names]).astype(f4)
        cls = np.concatenate([[k] * len(blocks[k][0]) for k in names])
        n = len(o)
        if stray:       # one lane a wave with a lamp less than 2 away: fails `longRay && minDistance >= 2`
            for w in range(0, n - WAVE + 1, WAVE):
                lane = w + int(rng.integers(0, WAVE))
                lamps[lane] = o[lane] + (_unit(rng, 1)[0] * 0.95).astype(f4)
        if ragged:
            n = (n // WAVE - 1) * WAVE + ragged
        iteration = rng.choice([0, 1, 2, 3], len(o)).astype(i4)
        return dict(name="shadow", scene_name=scene_name, scene=sc, si=sc.si, lamps=np.ascontiguousarray(lamps[:n]),
                    origins=np.ascontiguousarray(o[:n]), object_id=np.full(n, int(sc.prims["index"][sc.made.lamp]), i4),
                    iteration=np.ascontiguousarray(iteration[:n]), shaded=np.ascontiguousarray(shaded[:n]), cls=cls[:n])

    names = list(blocks)
    return {"pure": case_of(names), "one_stray": case_of(names, stray=True), "ragged_1": case_of(names[:2], ragged=1),
            "ragged_63": case_of(names[:2], stray=True, ragged=63)}
