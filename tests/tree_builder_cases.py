"""Synthetic scenes for the box-grid builder (test infrastructure, no test functions).

GPUKernel::compactBoxes(true) is built three times in this repository: by the host (sol-r_amd/host/GPUKernel.cpp), on the
device (sol-r_amd/csrc/solr_tree.hip) and, statement by statement after the reference, by the Python model of
tests/test_builder_reference_model.py.  The scenes of that file are random; each scene here is the smallest one that steers
ONE of the places where the device builder's header says the tree is decided - the float divisions and truncations of the
keys, their unsigned and signed wrap, the order of the maps, the first of two equal values and the sign of a zero in the
bounds, the cases it declines.

`CASES` maps a name to a `Case`: `spec(solr)` gives the primitives in the format of test_builder_reference_model.SCENES,
(type, p0, p1, p2, size, emissive); `view_distance`; `move`, a translation applied after a first build and before the one
that is compared (the scene extent stays the one from before it: only setPrimitive grows it); `movable`, which primitives
that translation may move (None: all); `capacity`, the room for nodes the raw device entry point is given (None: plenty);
`declined`, the reasons - in the words of test_builder_reference_model.declines() - for which the device builder must
leave the scene to the host, empty when it must build it; and `check(solr, spec, model)`, the case's self-check: it raises
unless the model, fed this scene, really went where the case is named after.  A case that misses its target fails on the
CPU (tests/test_tree_builder_cases.py); it never passes quietly.

`ENGINE_CASES` are the ones tests/test_tree_build_gpu.py also takes through GPUKernel::buildTreeOnDevice.
"""
from fractions import Fraction

import numpy as np

import test_builder_reference_model as M

F = np.float32
PZ, NZ = 0.0, -0.0
ZERO_BITS = {0x00000000: "+0", 0x80000000: "-0"}

ALIAS = "a lamp's index is a key of the level below the top"
KEY0 = "a top-level child hashes to key 0"
NO_LAMP = "no emissive primitive"
ROOM = "more boxes than the caller has room for"
FEW = "one or two primitives"
NO_INT = "a cell number no int holds"


class Case:
    def __init__(self, spec, check, steers, view_distance=50000.0, move=None, movable=None, capacity=None, declined=()):
        self.spec, self.check, self.steers = spec, check, steers
        self.view_distance, self.move, self.movable, self.capacity = view_distance, move, movable, capacity
        self.declined = list(declined)


CASES = {}


def case(name, steers, **kw):
    def add(check):
        spec = kw.pop("spec")
        assert name not in CASES
        CASES[name] = Case(spec, check, steers, **kw)
        return check
    return add


def bits(v):
    return int(np.asarray(v, F).view(np.uint32))


def sph(p0, r=10.0, lamp=False):
    return (0, tuple(p0), 0, 0, (r, 0, 0), lamp)             # ptSphere = 0 (include/solr_types.h)


FAR_LAMP = sph((8000.0, 8000.0, -8000.0), 10.0, True)        # the lamp of the model's tiny scene


def leaves(model):
    return [n for n in model.nodes[1:] if n["nb"] > 0]


def inner(model):
    return [n for n in model.nodes[1:] if n["nb"] == 0]


def zero_signs(nodes, side, axis):
    return {ZERO_BITS[bits(n[side][axis])] for n in nodes if bits(n[side][axis]) in ZERO_BITS}


def cells(model):
    """the level-0 cells the primitives hashed to (stream() has inserted an empty box per lamp index besides)"""
    return {k: model.level(0)[k] for k in model.hashed[0]}


def members(model):
    """non-emissive members per level-0 cell, largest first"""
    return sorted((len(b.entries) for b in cells(model).values()), reverse=True)


def spread(n, seed, scale=9000.0, lamps=(), r=20.0):
    """n spheres at random places, the ones at the positions `lamps` emissive"""
    def make(solr):
        rng = np.random.default_rng(seed)
        return [sph(tuple(float(v) for v in rng.uniform(-scale, scale, 3)), r, i in lamps) for i in range(n)]
    return make


# ---- ties and zeros ----------------------------------------------------------------------------------------------------------
def _zero_triangles_and_cylinders(solr):
    """on each axis in turn: every way to give +0 or -0 to p0, p1 and p2 of a triangle (p0, p1 of a cylinder) - all equal
    as values, so std::min / std::max keep their FIRST argument - with a size of +0 (the box's lower bound keeps the sign:
    x - 0) and of -0 (the upper bound keeps it: x + -0).  One primitive per cell, 100 apart on the next axis"""
    out = [FAR_LAMP]                        # (index 0 is no box's key)
    at = 1
    for axis in range(3):
        b, c = (axis + 1) % 3, (axis + 2) % 3
        for size in (PZ, NZ):
            for signs in np.ndindex(2, 2, 2):
                pts = []
                for k, s in enumerate(signs):
                    p = [0.0] * 3
                    p[axis], p[b], p[c] = (NZ if s else PZ), 100.0 * at + 3.0 * k, 50.0 + 7.0 * k
                    pts.append(tuple(p))
                out.append((solr.ptTriangle, pts[0], pts[1], pts[2], (size, size, size), False))
                at += 1
            for signs in np.ndindex(2, 2):
                pts = []
                for k, s in enumerate(signs):
                    p = [0.0] * 3
                    p[axis], p[b], p[c] = (NZ if s else PZ), 100.0 * at + 3.0 * k, 50.0 - 7.0 * k
                    pts.append(tuple(p))
                out.append((solr.ptCylinder, pts[0], pts[1], 0, (size, 0, 0), False))
                at += 1
    return out + [sph((-700.0, -700.0, -700.0))]


@case("zeros: triangles and cylinders, +0 against -0 in every argument position", spec=_zero_triangles_and_cylinders,
      steers="minStd / maxStd: the first argument's zero; the sign survives into the leaves and their parents")
def _(solr, spec, model):
    assert not model.declined and max(members(model)) == 1
    for axis in range(3):
        for side in ("lo", "hi"):
            assert zero_signs(leaves(model), side, axis) == {"+0", "-0"}, (side, axis)
            assert zero_signs(inner(model), side, axis) == {"+0", "-0"}, (side, axis)
    # ... and a min / max that kept its SECOND argument would show: among the primitives are pairs that differ in nothing
    # but which of two equal arguments carries the sign
    tri = [s for s in spec if s[0] == solr.ptTriangle]
    assert any(bits(a[1][0]) != bits(a[2][0]) for a in tri) and any(bits(a[2][0]) != bits(a[3][0]) for a in tri)


def _tied_members(solr):
    E = solr.ptEllipsoid
    out = []
    for k, (first, second) in enumerate([((PZ, PZ), (NZ, NZ)), ((NZ, NZ), (PZ, PZ)), ((PZ, NZ), (NZ, PZ)), ((NZ, PZ), (PZ, NZ))]):
        for x, size in (first, second):                 # two members of one cell, equal bounds but for the zero's sign
            out.append((E, (x, 500.0 * (k + 1), 40.0), 0, 0, (size, 30.0, 20.0), False))
    return out + [sph((-900.0, -900.0, -900.0)), sph((900.0, 100.0, 100.0)), FAR_LAMP]


@case("ties: two members of one cell whose bounds tie", spec=_tied_members,
      steers="k_level0Bounds: `<` and `>` keep the first member's bound, and with it the sign of its zero")
def _(solr, spec, model):
    assert not model.declined
    pairs = [n for n in leaves(model) if n["nb"] == 2]
    assert len(pairs) == 4
    assert {ZERO_BITS[bits(n["lo"][0])] for n in pairs} == {"+0", "-0"}
    assert {ZERO_BITS[bits(n["hi"][0])] for n in pairs} == {"+0", "-0"}
    for n in pairs:                                      # the first member decided both
        first = model.prims[model.order[n["start"]]]
        assert bits(n["lo"][0]) == bits(F(first["p0"][0]) - F(first["size"][0]))
        assert bits(n["hi"][0]) == bits(F(first["p0"][0]) + F(first["size"][0]))


def _tied_children(solr):
    E = solr.ptEllipsoid
    out = []
    for k, (first, second) in enumerate([(PZ, NZ), (NZ, PZ)]):
        # two level-0 cells 2 apart on y (a cell is 9000 / 6400 wide, a cell of the level above 9000 / 7): one parent
        for j, x in enumerate((first, second)):
            out.append((E, (x, 600.0 + 2400.0 * k + 2.0 * j, 40.0), 0, 0, (PZ, 30.0, 20.0), False))
    return out + [sph((-1000.0, -1000.0, -1000.0)), sph((1000.0, 100.0, 100.0)), FAR_LAMP]


@case("ties: children of one outer box whose bounds tie", spec=_tied_children,
      steers="k_outerBounds: the first child in key order gives the parent its zero")
def _(solr, spec, model):
    assert not model.declined and model.tree_depth == 1 and max(members(model)) == 1
    parents = [b for b in model.level(1).values() if len([k for k in b.entries if model.level(0)[k].entries]) == 2]
    assert len(parents) == 2
    assert {ZERO_BITS[bits(b.lo[0])] for b in parents} == {"+0", "-0"}
    for b in parents:
        assert bits(b.lo[0]) == bits(model.level(0)[b.entries[0]].lo[0]) != bits(model.level(0)[b.entries[1]].lo[0])


# ---- many members per level-0 cell ----------------------------------------------------------------------------------------
def _one_p0(count):
    def make(solr):
        rng = np.random.default_rng(count)
        here = (1234.5, -678.25, 91.0)
        out = []
        for i in range(count):
            lamp = i % 7 == 3
            kind = i % 5
            if kind == 0:
                out.append(sph(here, float(rng.uniform(1, 400)), lamp))
            elif kind == 1:
                out.append((solr.ptEllipsoid, here, 0, 0, tuple(float(v) for v in rng.uniform(1, 400, 3)), lamp))
            elif kind == 2:
                out.append((solr.ptCylinder, here, tuple(float(v) for v in rng.uniform(-900, 900, 3)), 0,
                            (float(rng.uniform(1, 90)), 0, 0), lamp))
            elif kind == 3:
                out.append((solr.ptTriangle, here, tuple(float(v) for v in rng.uniform(-900, 900, 3)),
                            tuple(float(v) for v in rng.uniform(-900, 900, 3)), (0, 0, 0), lamp))
            else:
                out.append((solr.ptXZPlane, here, 0, 0, (float(rng.uniform(1, 900)), 0, float(rng.uniform(1, 900))), lamp))
        return out + [sph((-3000.0, -3000.0, -3000.0)), sph((3000.0, 2000.0, 1000.0), 30.0)] + \
            ([] if count > 3 else [FAR_LAMP])
    return make


def _check_one_p0(count):
    def check(solr, spec, model):
        assert not model.declined
        lamps = sum(1 for s in spec[:count] if s[5])
        assert members(model)[:2] == [count - lamps, 1]
        if count > 3:
            assert lamps >= 1 and model.nodes[0]["nb"] == lamps
        cell = [n for n in leaves(model) if n["nb"] == count - lamps][0]
        got = model.order[cell["start"]:cell["start"] + cell["nb"]]
        assert got == [i for i in range(count) if not spec[i][5]]           # in id order, the lamps between them left out
    return check


for _count in (2, 64, 257, 1500):
    case("members: %d primitives with one p0, five types, every seventh a lamp" % _count, spec=_one_p0(_count),
         steers="one thread walks a cell's members in id order: bounds, counts and the streamed order")(_check_one_p0(_count))


@case("rebuild: 257 primitives with one p0 and two more, built a second time", spec=_one_p0(257), move=(0.0, 0.0, 0.0),
      steers="the box the reference resets before it builds (GPUKernel.cpp:1049) is box 0 of the level that was the top one "
             "before: of level 2 on a fresh kernel, where this scene's tree of depth 4 hashes it into an empty cell of "
             "level 3 - one node more - and the lamp box itself on a kernel that has built the scene before")
def _(solr, spec, model):
    assert not model.declined and model.tree_depth == 4 and model.depth_before == 4
    fresh = M.ReferenceBuilder(solr, model.vd, model.prims, model.emissive, extent=(model.min, model.max))
    fresh.compact_boxes()
    fresh.stream()
    assert len(fresh.nodes) == len(model.nodes) + 1
    extra = [n for n in inner(fresh) if n["skip"] == 1 and bits(n["lo"][0]) == bits(model.vd)]
    assert len(extra) == 1 and not [n for n in inner(model) if n["skip"] == 1]


def _only_lamps_in_a_cell(solr):
    here = (100.0, 100.0, 100.0)
    return [sph((-500.0, -500.0, -500.0)), sph((100.5, 100.0, 100.0)), sph(here, 5.0, True), sph((100.0, 100.5, 100.0)),
            sph(here, 6.0, True), sph((100.0, 100.0, 100.5)), sph(here, 7.0, True), sph((600.0, 700.0, 800.0))]


@case("members: a cell with only emissive members, next to occupied cells", spec=_only_lamps_in_a_cell,
      steers="a cell is made for lamps too and stays empty: no node, bounds at the seed, centre 0 for the level above")
def _(solr, spec, model):
    assert not model.declined
    empty = [k for k, b in cells(model).items() if not b.entries]
    assert len(empty) == 1 and len(model.lamps) == 3
    keys = sorted(cells(model))
    at = keys.index(empty[0])
    assert 0 < at < len(keys) - 1, "the empty cell is meant to lie between occupied ones in key order"
    assert bits(model.level(0)[empty[0]].lo[0]) == bits(1000000.0)


def _interleaved(solr):
    """the members of three cells given turn by turn, the cells in descending key order: a sort that is not stable, or
    one by (key, anything but the position), changes the order within a cell"""
    places = [(900.0, 900.0, 900.0), (0.0, 10.0, 20.0), (-900.0, -900.0, -900.0)]
    out = []
    for i in range(300):
        out.append((solr.ptEllipsoid, places[i % 3], 0, 0, (1.0 + (i * 37) % 101, 1.0 + (i * 53) % 89, 1.0 + (i * 71) % 97),
                    i % 50 == 49))
    return out


@case("members: three cells' members interleaved, against the key order", spec=_interleaved,
      steers="the radix sort by key must keep the ids ascending within a key")
def _(solr, spec, model):
    assert not model.declined
    assert members(model)[:3] == [98, 98, 98]
    for n in leaves(model):
        got = model.order[n["start"]:n["start"] + n["nb"]]
        assert got == sorted(got) and len({g % 3 for g in got}) == 1
    first = model.order[len(model.lamps)]
    assert first % 3 == 2, "the cell given last comes first in key order"


# ---- degenerate extent ---------------------------------------------------------------------------------------------------------
def _flat(axes, n=23):
    def make(solr):
        rng = np.random.default_rng(40 + len(axes))
        out = []
        for i in range(n):
            p = [float(v) for v in rng.uniform(-5000, 5000, 3)]
            for a in axes:
                p[a] = 0.0
            out.append(sph(p, float(rng.uniform(5, 200)), i == 0))        # (index 0 is no box's key)
        return out
    return make


def _check_flat(axes):
    def check(solr, spec, model):
        assert not model.declined
        for a in range(3):
            assert (model.min[a] == model.max[a]) == (a in axes), a
            assert (model.steps(6400)[a] == 1) == (a in axes)
            assert ({c[a] for c in model.cells[0].values()} == {0}) == (a in axes)
    return check


case("extent: no extent on z, its step becomes 1", spec=_flat([2]), steers="steps == 0 -> 1 on one axis")(_check_flat([2]))
case("extent: no extent on x and y", spec=_flat([0, 1]), steers="steps == 0 -> 1 on two axes")(_check_flat([0, 1]))


def _same_p0(at):
    def make(solr):
        return [sph(at, 10.0 + 3 * i, i == 2) for i in range(9)]
    return make


@case("extent: every p0 at the origin", spec=_same_p0((0.0, 0.0, 0.0)), steers="no extent at all: one cell, every step 1")
def _(solr, spec, model):
    assert not model.declined and model.steps(6400) == [1, 1, 1] and members(model) == [8]


@case("extent: every p0 the same, away from the origin", spec=_same_p0((5.0, -7.0, 0.125)),
      steers="the extent is the origin and one point: cells 0 and 6400 only")
def _(solr, spec, model):
    assert not model.declined and members(model) == [8], members(model)
    assert set(map(tuple, model.cells[0].values())) == {(6400, 0, 6400)}


# ---- edges of the grid ------------------------------------------------------------------------------------------------------------
def _corners(solr):
    lo, hi = (-4096.0, -1000.0, -333.0), (4096.0, 3000.0, 777.0)
    out = [sph(lo, 10.0), sph(hi, 20.0)]
    for k in range(1, 7):                                  # every mix of the two corners' coordinates
        out.append(sph(tuple(hi[a] if k >> a & 1 else lo[a] for a in range(3)), 5.0 * k))
    return out + [sph((1.0, 2.0, 3.0), 1.0, True)]


@case("edges: p0 at minPos and at maxPos", spec=_corners, steers="cells 0 and 6400 (one past the grid) on every axis")
def _(solr, spec, model):
    assert not model.declined
    assert set(map(tuple, list(model.cells[0].values())[:8])) == \
        {tuple(6400 if k >> a & 1 else 0 for a in range(3)) for k in range(8)}


def _on_cell_borders(solr):
    """x from 0 to 10: a cell is float(10 / 6400) wide, which no binary32 holds exactly, and the primitives sit at
    float(k * 10 / 6400): the exact quotient of the two float values lies a little to one side of k, the rounded one
    often ON k.  y, z: the same on extents of 3 and 7"""
    out = []
    for k in list(range(1, 120)) + list(range(6280, 6400)):
        out.append(sph((float(F(k * 10.0 / 6400.0)), float(F(k * 3.0 / 6400.0)), float(F(k * 7.0 / 6400.0))), 0.001))
    return out + [sph((10.0, 3.0, 7.0), 0.001), sph((5.0, 1.0, 1.0), 0.001, True)]


@case("edges: quotients that land on an integer only after rounding", spec=_on_cell_borders,
      steers="(c - min) / step must be ONE correctly rounded float division, then a truncation")
def _(solr, spec, model):
    assert not model.declined
    step = model.steps(6400)
    decided = [0, 0, 0]
    for p, cell in model.cells[0].items():
        for a in range(3):
            c = F(model.prims[p]["p0"][a]) - model.min[a]
            exact = Fraction(float(c)) / Fraction(float(step[a]))
            if int(exact) != cell[a]:                      # the cell is not the one the exact quotient lies in
                decided[a] += 1
                assert abs(exact - cell[a]) < Fraction(1, 1000)
    assert min(decided) >= 5, decided


# ---- types -----------------------------------------------------------------------------------------------------------------------------
def _types(solr):
    return [(solr.ptEllipsoid, (-2000.0, 100.0, 50.0), 0, 0, (300.0, 200.0, 100.0), False),
            (solr.ptEllipsoid, (-1500.0, 900.0, 50.0), 0, 0, (1.0, 800.0, 30.0), False),
            (solr.ptCone, (0.0, -2000.0, 40.0), (0.0, -1000.0, 40.0), 0, (150.0, 0, 0), False),
            (solr.ptCone, (700.0, -2000.0, 40.0), (300.0, -3000.0, 90.0), 0, (90.0, 0, 0), False),
            (solr.ptXYPlane, (1000.0, 1000.0, -500.0), 0, 0, (400.0, 300.0, 0.0), False),
            (solr.ptYZPlane, (-1000.0, 1000.0, 500.0), 0, 0, (0.0, 300.0, 200.0), False),
            (solr.ptXZPlane, (1000.0, -1000.0, 500.0), 0, 0, (400.0, 0.0, 200.0), False),
            (solr.ptCheckboard, (0.0, -2500.0, 0.0), 0, 0, (2000.0, 0.0, 2000.0), False),
            (solr.ptCamera, (2000.0, 2000.0, 2000.0), 0, 0, (50.0, 60.0, 70.0), False),
            (solr.ptCylinder, (1500.0, 500.0, -100.0), (1400.0, -600.0, -900.0), 0, (60.0, 0, 0), False),
            (solr.ptCylinder, (-1500.0, 500.0, -100.0), (-1400.0, 1600.0, 900.0), 0, (60.0, 0, 0), False),
            (solr.ptTriangle, (100.0, 100.0, 100.0), (-200.0, 300.0, 50.0), (150.0, -80.0, 400.0), (0, 0, 0), False),
            (solr.ptEllipsoid, (2500.0, -2500.0, 2500.0), 0, 0, (5.0, 6.0, 7.0), True)]


@case("types: ellipsoid, cone, the three planes, checkboard, camera, a cylinder with p1 below p0", spec=_types,
      steers="which size and which points each type brings to its cell's bounds")
def _(solr, spec, model):
    assert not model.declined and max(members(model)) == 1
    assert {s[0] for s in spec} >= {solr.ptEllipsoid, solr.ptCone, solr.ptXYPlane, solr.ptYZPlane, solr.ptXZPlane,
                                    solr.ptCheckboard, solr.ptCamera, solr.ptCylinder, solr.ptTriangle}
    by_first = {model.order[n["start"]]: n for n in leaves(model)}
    assert [float(v) for v in by_first[1]["hi"]] == [-1499.0, 1700.0, 80.0]          # an ellipsoid: three sizes
    assert [float(v) for v in by_first[3]["lo"]] == [610.0, -2090.0, -50.0]          # a cone: p0 and the radius, not p1
    assert [float(v) for v in by_first[9]["lo"]] == [1340.0, -660.0, -960.0]         # the cylinder: p1 is the lower end


# ---- counts ----------------------------------------------------------------------------------------------------------------------------
def _few(n, lamp):
    def make(solr):
        places = [(-300.0, 200.0, 100.0), (400.0, -500.0, 600.0), (50.0, 60.0, -700.0)]
        return [sph(places[i], 20.0 + i, lamp and i == n - 1) for i in range(n)]
    return make


def _check_few(n, lamp):
    def check(solr, spec, model):
        want = ([FEW] if n <= 2 else []) + ([] if lamp else [NO_LAMP])
        assert sorted(model.declined) == sorted(want), model.declined
        assert model.tree_depth == 1
    return check


for _n in (1, 2, 3):
    for _lamp in (True, False):
        case("counts: n = %d, %s" % (_n, "the last one a lamp" if _lamp else "no lamp"), spec=_few(_n, _lamp),
             declined=([FEW] if _n <= 2 else []) + ([] if _lamp else [NO_LAMP]),
             steers="`while (nb > 2)` gives depth 0 to processBoxes for n <= 2, `do ... while` one outer level")(
                 _check_few(_n, _lamp))


def _check_depth(depth, cells=None):
    def check(solr, spec, model):
        assert not model.declined and model.tree_depth == depth
        if cells is not None:
            assert model.boxes_per_level[0] == cells
    return check


case("counts: n = 11, one outer level", spec=spread(11, 111, lamps=(4,)), steers="11 / 4 = 2 ends the loop")(_check_depth(1))
case("counts: n = 12, two outer levels", spec=spread(12, 112, lamps=(4,)), steers="12 / 4 = 3 goes on")(_check_depth(2))
case("counts: n = 255", spec=spread(255, 255, lamps=(0,)), steers="one short of a block of 256 threads")(_check_depth(4, 255))
case("counts: n = 256, 256 level-0 cells", spec=spread(256, 256, lamps=(0,)),
     steers="exactly one block of threads per primitive and per cell")(_check_depth(4, 256))
case("counts: n = 257, 257 level-0 cells", spec=spread(257, 257, lamps=(0,)),
     steers="one thread in a second block, for primitives and for cells")(_check_depth(4, 257))


@case("counts: every primitive a lamp", spec=spread(5, 5, lamps=range(5)), steers="level 0 holds empty cells only")
def _(solr, spec, model):
    assert not model.declined and len(model.lamps) == 5 and not leaves(model)


@case("counts: no lamp", spec=spread(6, 6), declined=[NO_LAMP], steers="the first ordinary top-level box streamed as the lamp box")
def _(solr, spec, model):
    assert model.declined == [NO_LAMP]
    assert sorted(model.order) != list(range(6)), "box keys are streamed in the primitives' place"


# ---- view distance ---------------------------------------------------------------------------------------------------------------------
@case("view distance smaller than the scene", spec=spread(40, 40, lamps=(7,)), view_distance=1000.0,
      steers="k_outerBounds starts from +-viewDistance: a child beyond it does not move the parent's bound")
def _(solr, spec, model):
    assert not model.declined
    clipped = [n for n in inner(model) if any(bits(n["lo"][a]) == bits(1000.0) or bits(n["hi"][a]) == bits(-1000.0)
                                              for a in range(3))]
    assert len(clipped) >= 10


# ---- outside the extent: move, then rebuild -------------------------------------------------------------------------------------------
@case("outside: negative cell numbers on every axis", spec=spread(30, 30, lamps=(29,)), move=(-4000.0, -3000.0, -5000.0),
      steers="(unsigned)(int) of a negative quotient at level 0, signed key arithmetic above")
def _(solr, spec, model):
    assert not model.declined and model.negative_cells == {0, 1, 2}
    for d in range(model.tree_depth + 1):
        assert any(min(c) < 0 for c in model.cells[d].values()), d


def _one_movable(solr):
    return [sph((-1000.0, -1000.0, -1000.0), 10.0), sph((1000.0, 0.0, 0.0), 20.0), sph((0.0, 1000.0, 1000.0), 30.0),
            sph((500.0, 500.0, 500.0), 5.0, True)]


@case("outside: a box centre one top-level cell below minPos", spec=_one_movable, move=(0.0, 0.0, -750.0),
      movable=[True, False, False, False], declined=[KEY0],
      steers="X n^2 + Y n + Z + 1 = 0 for cell (0, 0, -1): the child lands in the lamp box's key")
def _(solr, spec, model):
    assert model.declined == [KEY0] and model.tree_depth == 1
    assert [0, 0, -1] in [list(c) for c in model.cells[1].values()]


def _narrow(solr):
    return [sph((0.25 * i, 100.0 * i, -50.0 * i), 0.01, i == 2) for i in range(5)]


@case("outside: a quotient of 2^31 and more", spec=_narrow, move=(1.0e6, 0.0, 0.0), declined=[NO_INT],
      steers="(int) of a float no int holds: 0x80000000 on the host, saturation on the device")
def _(solr, spec, model):
    assert model.declined == [NO_INT] and model.outside_int
    assert any(c[0] == M.INT_INDEFINITE for c in model.cells[0].values())


@case("movable: two primitives in three stay where they are", spec=spread(40, 41, lamps=(13,)), move=(300.0, -200.0, 100.0),
      movable=[i % 3 == 0 for i in range(40)], steers="translatePrimitives asks the movable flag; so does a rotation")
def _(solr, spec, model):
    assert not model.declined
    moved = [i for i in range(40) if bits(model.prims[i]["p0"][0]) != bits(spec[i][1][0])]
    assert moved == [i for i in range(0, 40, 3)]


# ---- declines ------------------------------------------------------------------------------------------------------------------------------
def _alias_one_level(solr):
    return [sph((1000.0, 0.0, 0.0), 20.0), sph((500.0, 500.0, 500.0), 5.0, True), sph((-1000.0, -1000.0, -1000.0), 10.0),
            sph((0.0, 1000.0, 1000.0), 30.0)]


@case("declines: lamp alias, one outer level", spec=_alias_one_level, declined=[ALIAS],
      steers="the lamp at index 1 and the cell of the minimum corner, key 1: that cell is streamed twice")
def _(solr, spec, model):
    assert model.declined == [ALIAS] and model.tree_depth == 1
    assert len(model.order) == 5 and model.order.count(2) == 2


def _alias_two_levels(solr):
    """13 primitives: two outer levels, the lower one a grid of 13^3.  The box of the sphere at the minimum corner hashes
    to cell (0, 0, 0) there, key 1, and primitive 1 is a lamp"""
    out = spread(13, 1313, scale=4000.0)(solr)
    out[0] = sph((-5000.0, -5000.0, -5000.0), 10.0)
    out[1] = sph(out[1][1], 5.0, True)
    return out


@case("declines: lamp alias, two outer levels", spec=_alias_two_levels, declined=[ALIAS],
      steers="the lamp's index among the keys of level 1, not of level 0")
def _(solr, spec, model):
    assert model.declined == [ALIAS] and model.tree_depth == 2
    assert 1 in model.hashed[1]
    assert len(model.order) > 13


def _triangle_below(solr):
    """the extent grows from p0 alone: a triangle with p0 at the minimum corner and p1, p2 far below it on z has its
    box's centre a cell and a half of the top level (a grid of 4: 500 a cell) below minPos"""
    return [(solr.ptTriangle, (-1000.0, -1000.0, -1000.0), (-990.0, -995.0, -2500.0), (-995.0, -990.0, -2000.0), (0, 0, 0), False),
            sph((1000.0, 0.0, 0.0), 20.0), sph((0.0, 1000.0, 1000.0), 30.0), sph((500.0, 500.0, 500.0), 5.0, True)]


@case("declines: top-level key 0, a triangle hanging below the extent", spec=_triangle_below, declined=[KEY0],
      steers="a top-level child in the lamp box's key without any move")
def _(solr, spec, model):
    assert model.declined == [KEY0] and model.tree_depth == 1
    assert [0, 0, -1] in [list(c) for c in model.cells[1].values()]


def _tiny(solr):
    return M.SCENES["tiny: 3 spheres + a lamp, one outer level"](solr)


@case("declines: room for 7 nodes, the tree has 8", spec=_tiny, capacity=7, declined=[ROOM],
      steers="the NB_MAX_BOXES branch, without 2.5 M boxes")
def _(solr, spec, model):
    assert model.declined == [ROOM] and len(model.nodes) == 8


@case("builds: room for exactly the tree's 8 nodes", spec=_tiny, capacity=8, steers="... and the other side of that branch")
def _(solr, spec, model):
    assert not model.declined and len(model.nodes) == 8


def _alias_empty_cell(solr):
    return [sph((1000.0, 0.0, 0.0), 20.0), sph((-1000.0, -1000.0, -1000.0), 5.0, True), sph((0.0, 1000.0, 1000.0), 30.0),
            sph((500.0, -500.0, 500.0), 10.0)]


@case("declines: the lamp's index is the key of an EMPTY level-0 cell", spec=_alias_empty_cell, declined=[ALIAS],
      steers="lamp 1 sits at the minimum corner itself: cell key 1 exists and is empty.  The reference's recursion finds "
             "nothing there and the host's tree is an ordinary one; the device declines all the same, as its header says: "
             "it compares the lamp indices with every key of the level, occupied or not")
def _(solr, spec, model):
    assert model.declined == [ALIAS] and model.tree_depth == 1
    assert 1 in model.levels[0] and not model.levels[0][1].entries
    assert sorted(model.order) == [0, 1, 2, 3], "nothing is streamed twice"


ENGINE_CASES = [
    "declines: lamp alias, one outer level",
    "counts: n = 2, the last one a lamp",
    "counts: n = 3, the last one a lamp",
    "members: 257 primitives with one p0, five types, every seventh a lamp",
    "zeros: triangles and cylinders, +0 against -0 in every argument position",
    "types: ellipsoid, cone, the three planes, checkboard, camera, a cylinder with p1 below p0",
    "movable: two primitives in three stay where they are",
    "counts: n = 257, 257 level-0 cells",
]
