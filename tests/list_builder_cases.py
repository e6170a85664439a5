"""Synthetic node lists for the builders of the order-free lists and for pruneInnerNodes (test infrastructure).

Pure numpy, fixed seeds, no engine.  `FREE_CASES` / `PRUNE_CASES` are the names, `free_case(name)` / `prune_case(name)` build
(rows (n, 2, 4) float32, start (n) int32, prims (p, 8, 4) float32 or None, margin, share, threshold) - the arguments of
engine_probes.free_lists / prune_list.  Each family is the smallest list that steers one branch of
sol-r_amd/csrc/solr_lists.hip; DESIGN.md section 4 says which.

Every list is LEGAL and shaped like the reference's (`_wrap`): node 0 is the lamp cell, a leaf with bounds +- viewDistance;
then inner nodes (count 0, skip = children + 1, bounds the exact union of the children) over runs of 1 to 7 leaves - so a
leaf's index is not its node's, about one node in seven is no leaf, and the device's second input route has something to
scan out.  flat=True: every leaf top-level with skip 1 - nearly every node a leaf, where the builder's scratch estimate
("a quarter of the nodes are leaves") is too small.  "L" in a name counts the leaves besides the lamp cell.
"""
import functools

import numpy as np

f32, i32 = np.float32, np.int32
VIEW = 1.0e6                                   # viewDistance: the lamp cell's half extent
PT_SPHERE, PT_XY, PT_YZ, PT_XZ = 0, 5, 6, 7    # include/solr_types.h PrimitiveType


def _bits(a):
    return np.asarray(a, i32).view(f32)


def _wrap(lo, hi, counts=None, flat=False, seed=1, starts=None):
    """the leaves lo / hi (L, 3) behind the lamp cell, under inner nodes over runs of 1 to 7 (or flat)"""
    lo, hi = np.asarray(lo, f32).reshape(-1, 3), np.asarray(hi, f32).reshape(-1, 3)
    L = len(lo)
    counts = 1 + np.arange(L) % 3 if counts is None else np.asarray(counts)
    starts = 1 + np.concatenate([[0], np.cumsum(counts)[:-1]]) if starts is None else np.asarray(starts)
    rng = np.random.RandomState(seed)
    nodes = [(np.full(3, -VIEW, f32), np.full(3, VIEW, f32), 1, 1, 0)]       # lo, hi, count, skip, start
    at = 0
    while at < L:
        run = 1 if flat else int(rng.randint(1, 8))
        run = min(run, L - at)
        if not flat:
            nodes.append((lo[at:at + run].min(axis=0), hi[at:at + run].max(axis=0), 0, run + 1, 0))
        for q in range(at, at + run):
            nodes.append((lo[q], hi[q], int(counts[q]), 1, int(starts[q])))
        at += run
    rows = np.zeros((len(nodes), 2, 4), f32)
    start = np.zeros(len(nodes), i32)
    for i, (a, b, count, skip, first) in enumerate(nodes):
        rows[i, 0, :3], rows[i, 0, 3] = a, b[2]
        rows[i, 1, :2] = b[:2]
        rows[i, 1, 2:] = _bits([count, skip])
        start[i] = first
    return rows, start


def _boxes(centres, half):
    centres, half = np.asarray(centres, f32), np.asarray(half, f32)
    return (centres - half).astype(f32), (centres + half).astype(f32)


def _random(L, seed, spread=1.0e4, size=300.0):
    rng = np.random.RandomState(seed)
    return _boxes(rng.uniform(-spread, spread, (L, 3)), rng.uniform(1.0, size, (L, 3)))


def _clusters(a, b, seed):
    """two clusters far apart on x, sorted by x: after the root's split a child begins where the first cluster ends"""
    rng = np.random.RandomState(seed)
    c = np.concatenate([rng.uniform([2.0e4, -500, -500], [2.1e4, 500, 500], (a, 3)),
                        rng.uniform([8.0e4, -500, -500], [8.1e4, 500, 500], (b, 3))])
    c = c[np.argsort(c[:, 0], kind="stable")]
    return _boxes(c, rng.uniform(1.0, 20.0, (a + b, 3)))


def _coincide(L, centre):
    """all centres the same, exactly (dyadic halves), every box another size: only the order tells the leaves apart"""
    half = (np.arange(L)[::-1, None] % 97 + 1 + np.arange(L)[:, None] // 97 * 100) * np.array([0.25, 0.5, 0.125])
    return _boxes(np.tile(np.asarray(centre, np.float64), (L, 1)), half)


def _lattice(k, offset, mirror=None):
    g = np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) * 4.0 + offset
    if mirror is not None:
        g[:, mirror] = -g[:, mirror]
    return _boxes(g, 1.0)


def _bin_edges(clo, extent):
    c = [f32(clo + k * extent / 16.0) for k in range(17)]
    c = sorted(set([x for v in c for x in (v, np.nextafter(v, f32(-np.inf)), np.nextafter(v, f32(np.inf)))
                    if f32(clo) <= x <= f32(clo + extent)]))
    rng = np.random.RandomState(5)
    centres = np.stack([np.array(c, f32), rng.uniform(-30, 30, len(c)).astype(f32), rng.uniform(-30, 30, len(c)).astype(f32)], axis=1)
    lo, hi = _boxes(centres, 0.5)
    order = rng.permutation(len(c))
    return lo[order], hi[order]


def _dynamic_range():
    rng = np.random.RandomState(9)
    small = _boxes(rng.uniform(-1e-3, 1e-3, (50, 3)), rng.uniform(1e-5, 1e-4, (50, 3)))
    large = _boxes(rng.uniform(8.5e5, 9.5e5, (50, 3)) * rng.choice([-1.0, 1.0], (50, 3)), rng.uniform(1e3, 5e4, (50, 3)))
    lo, hi = np.concatenate([small[0], large[0]]), np.concatenate([small[1], large[1]])
    lo[60:64, 0], hi[60:64, 0] = -VIEW, VIEW        # boxes that reach the view distance on an axis
    lo[64:68, 1], hi[68:72, 2] = -VIEW, VIEW
    order = rng.permutation(100)
    return lo[order], hi[order]


def _tiny_extents(step, L, axis):
    """centres `step` apart on one axis (1e-39 ... : 16 / extent is infinite in binary32), ordinary on the other two"""
    rng = np.random.RandomState(11)
    centres = rng.uniform(-50, 50, (L, 3))
    half = rng.uniform(0.5, 2.0, (L, 3))
    lo, hi = _boxes(centres, half)
    k = rng.permutation(L).astype(np.float64)
    lo[:, axis] = (k * step - step / 8).astype(f32)
    hi[:, axis] = (k * step + step / 8).astype(f32)
    return lo, hi


def _deep():
    c = np.zeros((30, 3))
    c[:, 0] = 1e-6 * 17.0 ** np.arange(30)
    half = np.ones((30, 3))
    half[:, 0] = 0.01 * c[:, 0]
    return _boxes(c, half)


# ---- build bounds: leaves with primitive records --------------------------------------------------------------------
def _record(kind, p0, size):
    r = np.zeros((8, 4), f32)
    r[0, :3], r[0, 3] = p0, _bits(kind)
    r[1, :3] = size
    return r


def _scene(leaves, flat=False, seed=3):
    """leaves: lists of (type, p0, size); the box of a leaf as uploaded is the union of p0 +- |size| (a sphere: its radius
    on every axis), as the reference boxes them.  Primitive 0 is the lamp, a sphere in the lamp cell."""
    prims = [_record(PT_SPHERE, (0, 0, 0), (10, 0, 0))]
    lo, hi, counts, starts = [], [], [], []
    for leaf in leaves:
        starts.append(len(prims))
        counts.append(len(leaf))
        los, his = [], []
        for kind, p0, size in leaf:
            prims.append(_record(kind, p0, size))
            reach = np.full(3, abs(size[0])) if kind == PT_SPHERE else np.abs(np.asarray(size, np.float64))
            los.append(np.asarray(p0, np.float64) - reach)
            his.append(np.asarray(p0, np.float64) + reach)
        lo.append(np.min(los, axis=0))
        hi.append(np.max(his, axis=0))
    rows, start = _wrap(lo, hi, counts, flat=flat, seed=seed, starts=starts)
    return rows, start, np.array(prims, f32)


def _walls(x, y, z, sign=1.0):
    s = (sign * x, sign * y, sign * z)
    return [[(PT_XZ, (0, -y, 0), s)], [(PT_XZ, (0, y, 0), s)], [(PT_YZ, (-x, 0, 0), s)], [(PT_YZ, (x, 0, 0), s)],
            [(PT_XY, (0, 0, -z), s)], [(PT_XY, (0, 0, z), s)]]


def _spheres(nb, reach, seed=21):
    rng = np.random.RandomState(seed)
    return [[(PT_SPHERE, tuple(rng.uniform(-reach, reach, 3)), (float(rng.uniform(20, 60)), 0, 0))] for _ in range(nb)]


def _room(spheres, dims=(1000.0, 1000.0, 1000.0), order=None, sign=1.0, **kw):
    walls = _walls(*dims, sign=sign)
    if order is not None:
        walls = [walls[q] for q in order]
    rows, start, prims = _scene(walls + _spheres(spheres, 0.8 * min(dims)), **kw)
    return rows, start, prims, f32(2.0 * max(dims) / 1024.0)


def _build_cases():
    cases = {}

    def add(name, made, share=0.25, threshold=1.0, prims=True):
        rows, start, records, margin = made
        cases[name] = (rows, start, records if prims else None, float(margin), share, threshold)

    for nb in (1, 10, 300):
        add("room-%d-spheres" % nb, _room(nb))
    add("room-300-spheres-flat", _room(300, flat=True))
    # the two largest walls (floor and ceiling of a room that is not cubic) tie in area: the first in the list is set apart
    add("room-tie-floor-first", _room(10, dims=(1500.0, 1000.0, 1200.0)))
    add("room-tie-ceiling-first", _room(10, dims=(1500.0, 1000.0, 1200.0), order=(1, 0, 2, 3, 4, 5)))
    # a wall whose centre is the union's on every axis (cl <= cu on all three: the low side, axis 0)
    middle = [[(PT_XZ, (0, 0, 0), (1000.0, 1000.0, 1000.0))]] + \
        [[(PT_SPHERE, (sx * 400.0, sy * 300.0, sz * 200.0), (50.0, 0, 0))] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    add("wall-at-the-centre", _scene(middle) + (f32(2.0),))
    # exactly three leaves with the lamp cell, which dominates; and three under it, a wall dominant
    add("three-leaves-lamp-dominant", _scene([[(PT_XZ, (0, -500.0, 0), (500.0, 500.0, 500.0))], [(PT_SPHERE, (100.0, 0, 50.0), (40.0, 0, 0))]]) + (f32(1.0),))
    add("three-leaves-wall-dominant", _scene([[(PT_XZ, (0, -500.0, 0), (500.0, 500.0, 500.0))], [(PT_SPHERE, (100.0, 0, 50.0), (40.0, 0, 0))],
                                              [(PT_SPHERE, (-200.0, 100.0, -50.0), (30.0, 0, 0))]]) + (f32(1.0),))
    walls = _walls(1000.0, 1000.0, 1000.0)
    add("leaf-of-two-rectangles", _scene([walls[0] + walls[2]] + walls[3:] + _spheres(12, 800.0)) + (f32(2.0),))
    add("leaf-of-rectangle-and-sphere", _scene([walls[0] + [(PT_SPHERE, (0, -900.0, 0), (50.0, 0, 0))]] + walls[1:] + _spheres(12, 800.0)) + (f32(2.0),))
    add("room-negative-sizes", _room(10, sign=-1.0))
    add("room-share-0", _room(10), share=0.0)
    add("room-no-records", _room(10), prims=False)
    for t in (0.25, 4.0):
        add("room-300-spheres-threshold-%g" % t, _room(300), threshold=t)
    return cases


def _plain_cases():
    cases = {}

    def add(name, boxes, threshold=1.0, **kw):
        rows, start = _wrap(boxes[0], boxes[1], **kw)
        cases[name] = (rows, start, None, 0.0, 0.25, threshold)

    # the decline rule, the first split, the smallest n >= 3
    for L in (0, 1, 2, 3):
        add("minimum-L%d" % L, _random(L, 40 + L))
    # wave and workgroup edges: with the lamp cell the leaf counts straddle 64, 128, 256, 512 and 1024
    for L in (62, 63, 64, 126, 127, 128, 254, 255, 256, 510, 511, 512, 1023, 1024):
        add("edge-L%d" % L, _random(L, L))
    for L in (63, 255, 1023):
        add("edge-L%d-flat" % L, _random(L, L), flat=True)
    for L in (64, 256, 1024):
        for t in (0.25, 4.0):
            add("edge-L%d-threshold-%g" % (L, t), _random(L, L), threshold=t)
    # a node's edge on a wave's or a workgroup's (flat: a leaf's place in the order is its place in the list, less none)
    for a, b in ((63, 64), (64, 64), (64, 65), (255, 256), (256, 256), (256, 257), (255, 2)):
        add("clusters-%d-%d-flat" % (a, b), _clusters(a, b, a + b), flat=True)
    add("clusters-64-65", _clusters(64, 65, 129))
    # signs and zeros
    rng = np.random.RandomState(70)
    add("all-negative", _boxes(rng.uniform(-9000, -100, (100, 3)), rng.uniform(1, 50, (100, 3))))
    add("all-positive", _boxes(rng.uniform(100, 9000, (100, 3)), rng.uniform(1, 50, (100, 3))))
    a = rng.uniform(1, 500, (40, 3)).astype(f32)
    add("centred-on-zero", (-a, a))
    lo, hi = _boxes(rng.uniform(-100, 100, (70, 3)), rng.uniform(1, 10, (70, 3)))
    lo[:, 0], hi[:, 0] = -0.0, -0.0                                  # flat on x, at minus zero
    add("minus-zero-slabs", (lo, hi))
    lo, hi = _boxes(rng.uniform(20, 100, (70, 3)), rng.uniform(1, 10, (70, 3)))
    lo[:, 0] = np.where(np.arange(70) % 2 == 0, -0.0, 0.0)           # the union's minimum is a zero: whose?
    lo[:, 1] = np.where(np.arange(70) % 3 == 0, 0.0, -0.0)
    add("zeros-of-both-signs-below", (lo, hi))
    lo, hi = _boxes(rng.uniform(-100, -20, (70, 3)), rng.uniform(1, 10, (70, 3)))
    hi[:, 0] = np.where(np.arange(70) % 2 == 0, 0.0, -0.0)
    hi[:, 2] = np.where(np.arange(70) % 5 == 0, -0.0, 0.0)
    add("zeros-of-both-signs-above", (lo, hi))
    # degenerate extents
    for L in (2, 3, 5, 64, 65, 257):
        add("coincide-L%d" % L, _coincide(L, (3.0, -5.0, 7.0)))
        add("coincide-at-zero-L%d" % L, _coincide(L, (0.0, 0.0, 0.0)))       # ... with the lamp cell's
    add("coincide-L257-flat", _coincide(257, (3.0, -5.0, 7.0)), flat=True)
    c = np.zeros((100, 3))
    c[:, 0] = rng.uniform(-4000, 4000, 100)
    add("on-a-line-through-zero", _boxes(c, [0.5, 0.25, 2.0]))
    add("on-a-line", _boxes(c + [0.0, 2.0, -3.0], [0.5, 0.25, 2.0]))
    c[:, 1] = rng.uniform(-4000, 4000, 100)
    add("on-a-plane", _boxes(c + [0.0, 0.0, 4.0], [0.5, 0.25, 2.0]))
    # cost ties
    add("lattice-4", _lattice(4, 8.0))
    add("lattice-8", _lattice(8, 8.0))
    add("lattice-4-about-zero", _lattice(4, -6.0))
    for axis in range(3):
        add("lattice-4-mirrored-%s" % "xyz"[axis], _lattice(4, 8.0, mirror=axis))
    # bin edges
    add("bin-edges-extent-1024", _bin_edges(-512.0, 1024.0))
    add("bin-edges-extent-1000", _bin_edges(-300.0, 1000.0))
    add("dynamic-range", _dynamic_range())
    # tiny extents
    for step, L, axis in ((1.0e-39, 2, 0), (1.0e-39, 17, 0), (1.0e-39, 40, 1), (2.0e-39, 20, 2), (1.0e-40, 33, 0), (4.0e-38, 2, 1)):
        add("tiny-extent-%g-L%d-%s" % (step, L, "xyz"[axis]), _tiny_extents(step, L, axis))
    add("deep-tree", _deep())
    # the sampling stride of the prune decisions: 2, 3 and 4
    for L in (8197, 12289, 16385):
        add("stride-L%d" % L, _random(L, L, spread=1.0e5))
        add("stride-L%d-flat" % L, _random(L, L, spread=1.0e5), flat=True)
    return cases


@functools.lru_cache(maxsize=None)
def _free():
    cases = _plain_cases()
    cases.update(_build_cases())
    return cases


# lists of fewer than two leaves: every builder declines them
DECLINED = ("minimum-L0",)


def _chain(depth):
    """the lamp cell, then `depth` inner nodes nested in each other over two leaves"""
    n = depth + 3
    rows = np.zeros((n, 2, 4), f32)
    start = np.zeros(n, i32)
    rows[0, 0], rows[0, 1] = (-VIEW, -VIEW, -VIEW, VIEW), (VIEW, VIEW, _bits(1), _bits(1))
    for d in range(depth):
        r = f32(1000.0 - d)
        rows[1 + d, 0], rows[1 + d, 1] = (-r, -r, -r, r), (r, r, _bits(0), _bits(depth + 2 - d))
    rows[n - 2, 0], rows[n - 2, 1] = (-5, -5, -5, 1), (-1, -1, _bits(1), _bits(1))
    rows[n - 1, 0], rows[n - 1, 1] = (1, 1, 1, 5), (5, 5, _bits(2), _bits(1))
    start[n - 2:] = 1, 2
    return rows, start


def _stray(out):
    """a node over three leaves that holds every leaf centre of the scene, the lamp cell's too (it hardly culls: it goes,
    whatever the threshold); out: one child reaches beyond it, and it has to stay"""
    lo = np.array([[-40, -40, -40], [10, -40, -40], [-40, 10, -40]], f32)
    hi = lo + np.array([30, 30, 80], f32)
    rows, start = _wrap(lo, hi, flat=True)
    group = np.zeros((1, 2, 4), f32)
    group[0, 0], group[0, 1] = (-40, -40, -40, 40), (40, 40, _bits(0), _bits(4))
    rows = np.concatenate([rows[:1], group, rows[1:]])
    start = np.concatenate([start[:1], [0], start[1:]]).astype(i32)
    if out:
        rows[3, 1, 0] = 40.5         # the second child's upper x
    return rows, start


@functools.lru_cache(maxsize=None)
def _prune():
    cases = {}
    free = _free()
    # the lists of the order-free cases as they are - inner nodes over runs of 1 to 7 leaves - at the case's own threshold,
    # and some of them on either side of it
    for name, case in free.items():
        cases["%s-threshold-%g" % (name, case[5])] = case[:2] + (case[5],)
    for name in ("minimum-L0", "minimum-L1", "minimum-L3", "edge-L63", "edge-L256", "edge-L1024", "clusters-64-65",
                 "coincide-L65", "lattice-4", "dynamic-range", "deep-tree", "room-300-spheres", "stride-L8197", "stride-L16385"):
        for t in (0.25, 4.0):
            cases["%s-threshold-%g" % (name, t)] = free[name][:2] + (t,)
    for t in (1.0, 0.25, 4.0):
        cases["child-sticks-out-threshold-%g" % t] = _stray(True) + (t,)
        cases["child-within-threshold-%g" % t] = _stray(False) + (t,)
        cases["chain-300-deep-threshold-%g" % t] = _chain(300) + (t,)
        cases["chain-200-deep-threshold-%g" % t] = _chain(200) + (t,)
    return cases


# the lists the device's decider leaves to the host: nested deeper than it launches levels for
PRUNE_DECLINED = tuple("chain-300-deep-threshold-%g" % t for t in (1.0, 0.25, 4.0))

FREE_CASES = tuple(_free())
PRUNE_CASES = tuple(_prune())


def free_case(name):
    return _free()[name]


def prune_case(name):
    return _prune()[name]


def scene_file(name, path):
    """a case in the format tests/list_builders_check.cpp reads: int32 n, p | rows | start | primitive records"""
    rows, start, prims = free_case(name)[:3]
    words = rows.view(i32)
    if prims is None:            # a sphere per primitive the leaves name, each in the middle of its leaf
        last = int((start + words[:, 1, 2]).max())
        prims = np.zeros((last, 8, 4), f32)
        for i in np.flatnonzero(words[:, 1, 2] > 0):
            prims[start[i]:start[i] + words[i, 1, 2], 0, :3] = 0.5 * (rows[i, 0, :3] + [rows[i, 1, 0], rows[i, 1, 1], rows[i, 0, 3]])
    with open(path, "wb") as f:
        np.array([len(start), len(prims)], i32).tofile(f)
        np.ascontiguousarray(rows, f32).tofile(f)
        np.ascontiguousarray(start, i32).tofile(f)
        np.ascontiguousarray(prims, f32).tofile(f)
