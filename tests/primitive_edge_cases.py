"""Rays aimed at the decisions of the six primitive tests (test infrastructure: a generator, deterministic, no GPU).

GI:159-659 - ellipsoid, sphere, cylinder / cone, the planes, the triangle - decide every hit.  The engine holds each test in
several forms (rt_device.h: sphereHit + sphereNormal beside sphereIntersection, triangleHit + triangleNormal beside
triangleIntersection, planePlain beside planeIntersection, a leaf's first primitive from the leaf's packed record and the
later ones row by row), and a walk chooses one per primitive from a bit of its tag.  The cases built here put rays ON the
comparisons of those tests, in the two layouts oracle.probes and tests/engine_probes.py take unchanged:

  per element      oracle.probes.case_primitive's layout; every ray twice, as the closest-hit walk and as the shadow walk
                   dispatch it (`shadows` 0 and 1); records written by hand, so that degenerate ones exist;
  through a walk   case_closest's / case_shadow's layout over a lattice of at most 64 leaves of 16 x 16 x 16 under one root,
                   32 apart; a leaf holds one case record, or two: the case record behind a tiny sphere the rays pass by
                   (the packed fetch, k == 0, and the row-by-row one, k > 0).

A case is made of FAMILIES: one record (or a few that differ in one field) and rays that differ in ONE binary32 input, which
steps through the floats around the analytically placed decision: +-k ulp for k = 0 ... 16, then +-2^j ulp.  A family is
built in the frame of the leaf it lies in - the stepping is done on the translated coordinate - so the walk is handed the
very numbers the family was made of; the per-element cases hold the families in the frame of the origin (the finest steps).
Directions are 16 long where nothing else is wanted: a power of two (what the text does to a unit direction it does to this
one, exactly), and the far point - the lamp of the shadow cases - lies behind the record.

Groups (one SceneInfo each): `dyadic` - geometryEpsilon 2^-10, transparentColor 0.5, rayEpsilon 0: the equalities;
`decimal` - geometryEpsilon 0.001, double-sided triangles, rayEpsilon 0.05; `flat` - extendedGeometry 0: sphere and plane
records tested as triangles; `camera` - ptCamera records with a 0 x 0 mapped material, per element only.  The consecutive
floats (OFFSETS) are for the families placed ON an equality; the others step geometrically (COARSE, SPARSE): the per-element
cases stay below 20 000 elements in all.

Nothing here judges a result: a family names the decision it is aimed at and, where an equality is wanted, the mutant
of the text model that can only differ from the model ON that equality (tests/test_primitive_edge_cases.py holds it to that).
"""
import numpy as np

import cuda_text_model as M

f4, i4 = np.float32, np.int32
WAVE = 64
E2 = 2.0 ** -10                      # the dyadic geometryEpsilon
VIEW_DISTANCE = 50000.0
PLAIN, GLASS, PROC, FAST, KEY_BELOW, KEY_EQUAL, KEY_ABOVE, EMISSIVE, WIRE0, WIRE1, WIRE255, LAMP, CAMERA = range(13)
GROUPS = {
    "dyadic": dict(geometryEpsilon=E2, transparentColor=0.5, rayEpsilon=0.0, doubleSidedTriangles=0, extendedGeometry=1),
    "decimal": dict(geometryEpsilon=0.001, transparentColor=2.0, rayEpsilon=0.05, doubleSidedTriangles=1, extendedGeometry=1),
    "flat": dict(geometryEpsilon=E2, transparentColor=0.5, rayEpsilon=0.0, doubleSidedTriangles=0, extendedGeometry=0),
    # ptCamera: its plane test maps a texture whatever the material (GI:551); per element, all-features instantiation only
    "camera": dict(geometryEpsilon=E2, transparentColor=0.5, rayEpsilon=0.0, doubleSidedTriangles=0, extendedGeometry=1),
}
OFFSETS = np.array([0] + [s * k for k in range(1, 17) for s in (-1, 1)] + [s * 2 ** j for j in (6, 12, 18) for s in (-1, 1)],
                   np.int64)
COARSE = np.array([0] + [s * k for k in (1, 16, 2 ** 8, 2 ** 11, 2 ** 14, 2 ** 17, 2 ** 20) for s in (-1, 1)], np.int64)
SPARSE = np.array([0] + [s * k for k in (16, 2 ** 11, 2 ** 20) for s in (-1, 1)], np.int64)
LATTICE = [(x, y, z) for x in (0.0, 32.0, -32.0, 64.0) for y in (0.0, 32.0, -32.0, 64.0) for z in (0.0, 32.0, -32.0, 64.0)]
LAMP_AT = (1024.0, 1024.0, 1024.0)


def materials(dtype):
    m = np.zeros(65506 + 30 + 1, dtype)
    for key in ("textureIds", "advancedTextureIds", "textureOffset", "advancedTextureOffset"):
        m[key][:16] = -1
    m["color"][:16] = (0.25, 0.25, 0.25, 0.0)
    m["specular"][:16] = (0.1, 200.0, 0.0, 0.0)
    m["color"][GLASS] = (0.5, 0.25, 0.125, 0.0)
    m["transparency"][GLASS], m["refraction"][GLASS], m["reflection"][GLASS], m["opacity"][GLASS] = 0.5, 1.1, 0.5, 0.2
    m["attributes"][PROC, 1] = 1
    m["attributes"][FAST, 0] = 1
    m["color"][KEY_BELOW] = (0.5, 0.5, 0.5 - 2.0 ** -22, 0.0)      # (r + g + b) / 3 against transparentColor 0.5
    m["color"][KEY_EQUAL] = (0.5, 0.5, 0.5, 0.0)
    m["color"][KEY_ABOVE] = (0.5, 0.5, 0.5 + 2.0 ** -22, 0.0)
    m["innerIllumination"][EMISSIVE, 0] = 0.5
    for k, w in ((WIRE0, 0), (WIRE1, 1), (WIRE255, 255)):
        m["attributes"][k, 2], m["attributes"][k, 3] = 2, w
    m["innerIllumination"][LAMP, 0] = 2.0
    m["color"][LAMP] = (1.0, 1.0, 1.0, 0.0)
    m["color"][CAMERA] = (0.25, 0.375, 0.5, 0.75)       # a 0 x 0 mapping: cubeMapping returns this, the shadow intensity its w
    return m


def step(x, offsets=OFFSETS):
    """the binary32 numbers `offsets` places from x in the order of the floats (through +-0 and the denormals)"""
    b = np.array([x], f4).view(i4).astype(np.int64)[0]
    key = b if b >= 0 else -(b & 0x7fffffff)
    k = key + offsets
    bits = np.where(k >= 0, k, (-k) | 0x80000000).astype(np.uint32)
    return bits.view(f4)


def stack(records):
    """records -> one array in the C layout (numpy re-packs padded record types when it concatenates)"""
    out = np.zeros(len(records), _P)
    for i, r in enumerate(records):
        out[i] = r
    return out


class Family:
    """decision: what it is aimed at; equality: the mutant (tests/test_primitive_edge_cases.py MUTANTS) that differs from
    the model only where the compared numbers are equal - None where no equality is claimed; recs: one record or one per
    ray, in the frame of the origin; rays: see realize; walk: goes into the lattice"""

    def __init__(self, decision, recs, o, t, mode=None, axis=0, equality=None, walk=True, directions=None, current=-2):
        self.decision, self.equality, self.walk, self.current = decision, equality, walk, current
        self.recs = recs if isinstance(recs, list) else [recs]
        self.o, self.t = np.atleast_2d(np.asarray(o, f4)), np.atleast_2d(np.asarray(t, f4))
        self.mode, self.axis, self.directions = mode, axis, directions

    offsets = OFFSETS

    def realize(self, c):
        """-> records, origins, targets (directions, where the family states them) in the frame of a leaf at c"""
        c = np.asarray(c, f4)
        o, t = (self.o + c).astype(f4), (self.t + c).astype(f4)
        a = self.axis
        if self.mode is not None:
            vals = step(o[0, a] if self.mode != "t" else t[0, a], self.offsets)
            o, t = np.repeat(o, len(vals), 0), np.repeat(t, len(vals), 0)
            if self.mode in ("o", "ot", "shift"):
                o[:, a] = vals
            if self.mode in ("t", "ot"):
                t[:, a] = vals
            if self.mode == "shift":                 # the far point moves with the origin: the direction stays
                t[:, a] = (vals + f4(self.t[0, a] - self.o[0, a])).astype(f4)
        k = len(self.recs)                           # every ray with every record, ray by ray
        o, t = np.repeat(o, k, 0), np.repeat(t, k, 0)
        recs = stack(self.recs * (len(o) // k))
        for key in ("p0", "p1", "p2"):
            recs[key] = (recs[key] + c).astype(f4)
        return recs, np.ascontiguousarray(o), np.ascontiguousarray(t)


# ---- records --------------------------------------------------------------------------------------------------------------
_P = None


def rec(ptype, p0=(0, 0, 0), size=(0, 0, 0), mat=PLAIN, p1=(0, 0, 0), p2=(0, 0, 0), n0=(0, 0, 0), n1=(0, 0, 0), n2=(0, 0, 0)):
    p = np.zeros(1, _P)[0]
    p["type"], p["p0"], p["p1"], p["p2"], p["size"], p["materialId"] = ptype, p0, p1, p2, size, mat
    p["n0"], p["n1"], p["n2"] = n0, n1, n2
    p["vt1"], p["vt2"] = (1.0, 0.0), (0.0, 1.0)
    return p


def sphere(r=1.0, mat=PLAIN, ptype=M.ptSphere, p0=(0, 0, 0)):
    return rec(ptype, p0, (r, r, r) if mat == PROC else (r, 0, 0), mat)


def cylinder(ptype=M.ptCylinder, r=1.0, length=4.0, size_y=None, mat=PLAIN, n1=(0, 1, 0)):
    return rec(ptype, (0, 0, 0), (r, r if size_y is None else size_y, r), mat, p1=(0, length, 0), p2=(0, length / 2, 0), n1=n1)


def plane(ptype, half=2.0, mat=PLAIN):
    across = {M.ptXYPlane: 2, M.ptCamera: 2, M.ptYZPlane: 0}.get(ptype, 1)
    size, n = [half] * 3, [0.0] * 3
    size[across], n[across] = 0.0, 1.0
    return rec(ptype, (0, 0, 0), size, mat, n0=n, n1=n, n2=n)


def triangle(p1=(4, 0, 0), p2=(0, 4, 0), mat=PLAIN, n=((0, 0, 1),) * 3, p0=(0, 0, 0)):
    return rec(M.ptTriangle, p0, (0, 0, 0), mat, p1=p1, p2=p2, n0=n[0], n1=n[1], n2=n[2])


def along(o, d, length=16.0):
    o = np.asarray(o, np.float64)
    return o, o + np.asarray(d, np.float64) * length


def fan(centre, reach, n=12, seed=1, distance=6.0):
    """n rays from around `centre` at `distance` towards points within `reach` of it: some hit, some pass by"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = np.asarray(centre) + np.round(u * distance * 64) / 64
    aim = np.asarray(centre) + np.round(rng.uniform(-reach, reach, (n, 3)) * 64) / 64
    return o, o + (aim - o) * 4.0


# ---- the families -----------------------------------------------------------------------------------------------------------
def sphere_families(eps, eq):
    """eq: the equalities are claimed (the dyadic epsilon)"""
    F, out = Family, []
    E = lambda name: name if eq else None     # noqa: E731
    for ptype, tag in ((M.ptSphere, "sphere"), (M.ptEnvironment, "environment")):
        S = sphere(ptype=ptype)
        out += [
            F(tag + ": d <= 0", S, *along((-5, 1, 0), (1, 0, 0)), "ot", 1, E("sphere d <= 0")),
            # t1 == epsilon: the origin epsilon before the near point - the back face from there on
            F(tag + ": t1 <= eps (the back flag)", S, *along((-1 - eps, 0, 0), (1, 0, 0)), "shift", 0, E("sphere t1 <= eps")),
            # t2 == epsilon: the origin epsilon before the far point, inside
            F(tag + ": t2 <= eps (going out)", S, *along((1 - eps, 0, 0), (1, 0, 0)), "shift", 0, E("sphere both: t2 <= eps")),
            # both roots behind: the origin beyond the far point
            F(tag + ": both roots behind", S, *along((1, 0, 0), (1, 0, 0)), "shift", 0),
            F(tag + ": origin on the surface going in", S, *along((-1, 0, 0), (1, 0, 0)), "shift", 0),
            F(tag + ": origin at the centre", S, *fan((0, 0, 0), 1.2, 12, 14, distance=0.0)),
            F(tag + ": radius 0", [sphere(0.0, ptype=ptype), S], *along((-5, 0, 0), (1, 0, 0)), None),
        ]
    S = sphere()
    out += [
        F("sphere: radius 0.5 at 1e4 (cancellation in c)", sphere(0.5, p0=(1.0e4, 1.0e4, 1.0e4)),
          *along((1.0e4 - 8, 1.0e4 + 0.5, 1.0e4), (1, 0, 0)), "ot", 1, walk=False),
        F("sphere: transparent (1 - |r|)", sphere(mat=GLASS), *fan((0, 0, 0), 1.2, 16, 2)),
        F("sphere: transparent, d <= 0", sphere(mat=GLASS), *along((-5, 1, 0), (1, 0, 0)), "ot", 1, E("sphere d <= 0")),
        F("sphere: procedural", sphere(mat=PROC), *fan((0, 0, 0), 1.2, 16, 3)),
        F("sphere: procedural, t1 <= eps", sphere(mat=PROC), *along((-1 - eps, 0, 0), (1, 0, 0)), "shift", 0, E("sphere t1 <= eps")),
        F("sphere: fast transparency, another material current", [sphere(mat=FAST), S], *fan((0, 0, 0), 1.2, 16, 4), current=PLAIN),
        F("sphere: fast transparency, its own material current", [sphere(mat=FAST), S], *fan((0, 0, 0), 1.2, 16, 4), current=FAST),
    ]
    return out


def ellipsoid_families(eps, eq):
    F, out = Family, []
    E = lambda name: name if eq else None     # noqa: E731
    L = rec(M.ptEllipsoid, (0, 0, 0), (2, 1, 4))
    out += [
        F("ellipsoid: d < 0", L, *along((-5, 1, 0), (1, 0, 0)), "ot", 1, E("ellipsoid d < 0")),
        F("ellipsoid: b == 0", L, *along((0, 0.5, 0), (1, 0, 0)), "shift", 0, E("ellipsoid b == 0")),
        F("ellipsoid: c == 0", L, *along((-2, 0, 0), (1, 0, 0)), "shift", 0, E("ellipsoid c == 0")),
        F("ellipsoid: c == 0 going out", L, *along((2, 0, 0), (1, 0, 0)), "shift", 0),
        # the near root (t2) at epsilon: from there on the far one is chosen
        F("ellipsoid: t2 <= eps (near root)", L, *along((-2 - eps, 0, 0), (1, 0, 0)), "shift", 0, E("ellipsoid elif t2 <= eps")),
        # the far root (t1) at epsilon, from inside
        F("ellipsoid: t1 <= eps (far root)", L, *along((2 - eps, 0, 0), (1, 0, 0)), "shift", 0),
        F("ellipsoid: from outside, both roots ahead", L, *fan((0, 0, 0), 3.0, 16, 5)),
        F("ellipsoid: a size component of 0", [rec(M.ptEllipsoid, (0, 0, 0), (2, 0, 4)), L], *fan((0, 0, 0), 2.0, 16, 6)),
    ]
    return out


def cylinder_families(eps, eq):
    F, out = Family, []
    E = lambda name: name if eq else None     # noqa: E731
    for ptype, tag in ((M.ptCylinder, "cylinder"), (M.ptCone, "cone")):
        C = cylinder(ptype)
        thin = cylinder(ptype, r=2.0 ** -12, length=8.0)
        half = cylinder(ptype, size_y=0.5)
        out += [
            # |cross(dir, n1)| == epsilon: from on the axis of a thin one, leaving through its wall at height 5
            F(tag + ": |cross(dir, n1)| against eps", thin, (0, 1, 0), (eps, 17, 0), "t", 0, E("cylinder ln < eps")),
            F(tag + ": along the axis, and at 1e-7, 1e-4, 1e-3 of it", thin, [(0, 1, 0)] * 8,
              [(x, 17, 0) for x in (0.0, -0.0, 1.6e-6, -1.6e-6, 1.6e-3, -1.6e-3, 1.6e-2, -1.6e-2)]),
            F(tag + ": d > size.y", C, *along((-5, 2, 1), (1, 0, 0)), "ot", 2, E("cylinder d > size.y")),
            F(tag + ": d > size.y, size.y != size.x", half, *along((-5, 2, 0.5), (1, 0, 0)), "ot", 2, E("cylinder d > size.y")),
            F(tag + ": size.y != size.x, between the two", [half, C], *along((-5, 2, 0.75), (1, 0, 0)), "ot", 2),
            F(tag + ": t < 0 (closest approach at the origin)", C, *along((0, 2, 0.5), (1, 0, 0)), "shift", 0, E("cylinder t < 0")),
            F(tag + ": scale1 < eps at the near root", C, *along((-5, eps, 0), (1, 0, 0)), "ot", 1, E("cylinder scale1 < eps (near)")),
            F(tag + ": scale2 > eps at the near root", C, *along((-5, 4 + eps, 0), (1, 0, 0)), "ot", 1, E("cylinder scale2 > eps (near)")),
            # slanted: the near root cut by an end, the far root on the decision
            F(tag + ": scale1 < eps at the far root", C, (-5, eps - 3, 0), (11, eps + 5, 0), "shift", 1, E("cylinder scale1 < eps (far)")),
            F(tag + ": scale2 > eps at the far root", C, (-5, 7 + eps, 0), (11, eps - 1, 0), "shift", 1, E("cylinder scale2 > eps (far)")),
            F(tag + ": from inside", C, *fan((0, 2, 0), 2.5, 12, 7, distance=0.5)),
            F(tag + ": p0 == p1 (n1 = 0)", [rec(ptype, (0, 0, 0), (1, 1, 1), p2=(0, 0, 0)), C], *fan((0, 2, 0), 2.0, 12, 8)),
            F(tag + ": n1 is not normalize(p1 - p0)", cylinder(ptype, n1=(0.75, 0.5, 0)), *fan((0, 2, 0), 2.5, 24, 9)),
            # dot(dir, O) == 0: an n1 so long that |cross(n, n1)|^2 is infinite (O = cross * (1 / inf) = 0) while |cross(dir, n1)|^2
            # of a direction 0.25 long is not: s is infinite, the point no number, and no comparison with it refuses
            F(tag + ": dot(dir, O) == 0", cylinder(ptype, n1=(0, 3.0e19, 0)), (-5, 2, 1), (-4.75, 2, 1), "ot", 2, walk=False),
        ]
    return out


def plane_families(eps, eq):
    F, out = Family, []
    E = lambda name: name if eq else None     # noqa: E731
    kinds = ((M.ptXYPlane, "XY", 0, 1, 2), (M.ptYZPlane, "YZ", 1, 2, 0), (M.ptXZPlane, "XZ", 0, 2, 1),
             (M.ptCheckboard, "checkerboard", 0, 2, 1), (M.ptMagicCarpet, "carpet", 0, 2, 1))
    for ptype, tag, u, v, w in kinds:
        R = plane(ptype)
        for face, side in (("front", 1.0), ("rear", -1.0)):
            d = [0.0, 0.0, 0.0]
            d[w] = -side
            single = ptype in (M.ptCheckboard, M.ptMagicCarpet) and face == "rear"      # nothing is hit from behind
            for axis, other in ((u, v), (v, u)):
                for sign in (1.0, -1.0):
                    o = [0.0, 0.0, 0.0]
                    o[w], o[axis], o[other] = 3.0 * side, 2.0 * sign, 0.5
                    name = "plane %s %s: |I.%s - p0.%s| < size.%s" % (tag, face, "xyz"[axis], "xyz"[axis], "xyz"[axis])
                    out.append(F(name, [plane(M.ptXZPlane, 4.0), R] if single else R, *along(o, d), "ot", axis,
                                 None if single else E("plane %s %s edge %s" % (tag, face, "xyz"[axis]))))
            o = [0.0, 0.0, 0.0]
            o[w], o[u], o[v] = 3.0 * side, 2.0, 2.0
            # (beside a larger rectangle - or, behind a single-sided one, a two-sided one - that the same rays hit)
            out.append(F("plane %s %s: a corner" % (tag, face), [plane(M.ptXZPlane, 4.0) if single else plane(ptype, 4.0), R], *along(o, d), "ot", u))
            o[u], o[v], o[w] = 0.5, 0.25, 0.0
            out.append(F("plane %s %s: o.W against p0.W" % (tag, face), [plane(M.ptXZPlane, 4.0), R] if single else R, *along(o, d), "shift", w,
                         None if single else E("plane %s %s o.W" % (tag, face))))
        o, t = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        o[w], o[u], o[v] = 3.0, 0.5, 0.25
        t[w], t[u], t[v] = 3.0, 0.5 + 2.0 ** -24, 0.25      # (nearly along the normal: the point stays inside)
        out.append(F("plane %s: d.W through 0" % tag, R, o, t, "t", w))
    for ptype in (M.ptXYPlane, M.ptCheckboard):
        keyed = [plane(ptype, mat=KEY_BELOW), plane(ptype, mat=KEY_EQUAL), plane(ptype, mat=KEY_ABOVE)]
        out.append(F("plane: averageColor >= transparentColor", keyed, *fan((0, 0, 0), 1.5, 4, 10 + ptype),
                     equality=E("plane colour key")))
    # the chessboard of an emissive YZ plane: (int)|I| % 4000 < 2000 on both axes (GI:486-490)
    big = rec(M.ptYZPlane, (0, 0, 0), (0, 8192, 8192), EMISSIVE, n0=(1, 0, 0), n1=(1, 0, 0), n2=(1, 0, 0))
    for axis, other in ((1, 2), (2, 1)):
        for at in (2000.0, 4000.0, -2000.0):
            o = [3.0, 0.0, 0.0]
            o[axis], o[other] = at, 100.0
            out.append(F("plane YZ emissive: (int)|I.%s| %% 4000 < 2000" % "xyz"[axis], big, *along(o, (-1, 0, 0)), "ot", axis,
                         E("plane YZ chessboard " + "xyz"[axis]) if abs(at) == 2000.0 else None, walk=False))
    out.append(F("plane YZ emissive: small", plane(M.ptYZPlane, mat=EMISSIVE), *along((3, 2, 0.5), (-1, 0, 0)), "ot", 1))
    # wireframe mode 2: (int)|x| % 100 <= width or (int)|y| % 100 <= width
    for mat, width, at in ((WIRE0, 0, 1.0), (WIRE1, 1, 2.0), (WIRE255, 255, 3.0)):
        for ptype, tag, u, v, w in kinds[:3]:
            o = [0.0, 0.0, 0.0]
            o[w], o[u], o[v] = 3.0, at, at + 0.5
            d = [0.0, 0.0, 0.0]
            d[w] = -1.0
            out.append(F("plane %s: wireframe width %d" % (tag, width), [plane(ptype, 4.0, mat), plane(ptype, 4.0)], *along(o, d), "ot", u,
                         E("wireframe X <= width") if width < 255 else None))
            o[u], o[v] = at + 0.5, at
            out.append(F("plane %s: wireframe width %d, the other axis" % (tag, width), [plane(ptype, 4.0, mat), plane(ptype, 4.0)],
                         *along(o, d), "ot", v, E("wireframe Y <= width") if width < 255 else None))
    return out


def _at_the_edge(p1=(5.5, 3, 1.25), p2=(1, 6.75, 7.5), n=96, seed=15):
    rng = np.random.default_rng(seed)
    s = rng.uniform(0, 1, (n, 1))
    at = np.asarray(p1) * s + np.asarray(p2) * (1 - s)
    o = at + np.round(rng.uniform(-3, 3, (n, 3)) * 8) / 8 + [0, 0, 5]
    return o, o + (at - o) * 2


def camera_families():
    """a ptCamera record with a 0 x 0 mapped material, from both sides: the XY plane's branch (GI:514-541)"""
    F, out = Family, []
    R = plane(M.ptCamera, mat=CAMERA)
    for face, side in (("front", 1.0), ("rear", -1.0)):
        d = (0, 0, -side)
        for axis, other in ((0, 1), (1, 0)):
            for sign in (1.0, -1.0):
                o = [0.0, 0.0, 3.0 * side]
                o[axis], o[other] = 2.0 * sign, 0.5
                out.append(F("camera %s: |I.%s - p0.%s| < size.%s" % (face, "xy"[axis], "xy"[axis], "xy"[axis]), R, *along(o, d), "ot", axis,
                             "plane XY %s edge %s" % (face, "xy"[axis])))
        out.append(F("camera %s: o.W against p0.W" % face, R, *along((0.5, 0.25, 0.0), d), "shift", 2, "plane XY %s o.W" % face))
    keyed = plane(M.ptCamera, mat=KEY_EQUAL)
    out.append(F("camera: the colour key", [keyed, R], *fan((0, 0, 0), 1.5, 8, 16), equality="plane colour key"))
    return out


def triangle_families(eps, eq, flat=False):
    F, out = Family, []
    E = lambda name: name if eq else None     # noqa: E731
    T = triangle()
    down, up = (0, 0, -1), (0, 0, 1)
    out += [
        F("triangle: a < 0", T, *along((0, 1, 3), down), "ot", 0, E("triangle a < 0")),
        F("triangle: a > 1 (the vertex p1)", T, *along((4, 0, 3), down), "ot", 0, E("triangle a > 1")),
        F("triangle: b < 0", T, *along((1, 0, 3), down), "ot", 1, E("triangle b < 0")),
        F("triangle: b > 1 (the vertex p2)", T, *along((0, 4, 3), down), "ot", 1, E("triangle b > 1")),
        F("triangle: the vertex p0", T, *along((0, 0, 3), down), "ot", 0),
        F("triangle: a + b > 1", T, *along((2, 2, 3), down), "ot", 0, E("triangle a + b > 1")),
        F("triangle: a + b > 1, from below", T, *along((1, 3, -3), up), "ot", 1, E("triangle a + b > 1")),
        # det = 16 d.z: +-epsilon at d.z = -+epsilon / 16
        F("triangle: |det| < eps, det > 0", T, (1, 1, eps / 16), (1, 1, 0), "o", 2, E("triangle |det| < eps")),
        F("triangle: |det| < eps, det < 0", T, (1, 1, -eps / 16), (1, 1, 0), "o", 2, E("triangle |det| < eps")),
        F("triangle: t < 0 at +0", T, *along((1, 1, 0), down), "shift", 2, E("triangle t < 0")),
        F("triangle: t < 0 at -0", T, *along((1, 1, 0), up), "shift", 2, E("triangle t < 0")),
        F("triangle: r > 0 (the flip of the normal)", triangle(n=((1, 0, 0),) * 3), (1, 1, 3), (1, 1, -13), "t", 0, E("triangle r > 0")),
        F("triangle: vertex normals whose weighted sum is 0", triangle(n=((0, 0, 1), (0, 0, -1), (0, 0, 0))), *along((1, 1, 3), down), "ot", 0),
        F("triangle: three collinear points", [triangle((2, 0, 0), (4, 0, 0)), T], *along((1, 0, 3), down), "ot", 1),
        F("triangle: two equal points", [triangle((4, 0, 0), (4, 0, 0)), T], *along((1, 0, 3), down), "ot", 1),
        F("triangle: transparent", triangle(mat=GLASS), *fan((1, 1, 0), 2.5, 16, 11)),
        # points along the hypotenuse of triangles whose quotients are not dyadic: a + b lands on either side of 1
        F("triangle: along the hypotenuse", triangle((3, 0, 0), (0, 3, 0)),
          *[np.array(x) for x in zip(*[along((3 * k / 48.0, 3 - 3 * k / 48.0, 3), down) for k in range(49)])]),
        F("triangle: along the hypotenuse, slanted", triangle((5, 0, 0), (0, 7, 0)),
          *[np.array(x) for x in zip(*[((5 * k / 48.0 + 1, 7 - 7 * k / 48.0 + 0.5, 4), (5 * k / 48.0 - 3, 7 - 7 * k / 48.0 - 1.5, -12))
                                       for k in range(49)])]),
        # a triangle in general position, rays from all around aimed at its edge p1 - p2: behind a + b > 1 lies the
        # reference's second test with E21 = p1 - p1, which refuses what a test with the edge p1 - p2 would let through
        F("triangle: along the edge p1 - p2, in general position", triangle((5.5, 3, 1.25), (1, 6.75, 7.5)), *_at_the_edge()),
    ]
    if flat:
        # without extended geometry every record is tested as a triangle: a sphere's and a plane's p1 / p2 are what the
        # record holds there (zeros: a degenerate triangle) - beside records of those types that carry a triangle
        as_sphere, as_plane = triangle(), triangle()
        as_sphere["type"], as_sphere["size"] = M.ptSphere, (1, 0, 0)
        as_plane["type"], as_plane["size"], as_plane["n0"] = M.ptXZPlane, (2, 0, 2), (0, 1, 0)
        out += [
            F("flat: a sphere record tested as a triangle", [as_sphere, sphere()], *along((1, 0, 3), down), "ot", 1, E("triangle b < 0")),
            F("flat: a plane record tested as a triangle", [as_plane, plane(M.ptXZPlane)], *along((0, 1, 3), down), "ot", 0, E("triangle a < 0")),
        ]
    return out


def every_type_families(eps):
    """a zero direction, denormal components, origins at +-viewDistance, directions of length 1e-12 and 1e12, per type"""
    F, out = Family, []
    records = (("sphere", sphere()), ("ellipsoid", rec(M.ptEllipsoid, (0, 0, 0), (2, 1, 4))), ("cylinder", cylinder()),
               ("cone", cylinder(M.ptCone)), ("XY plane", plane(M.ptXYPlane)), ("triangle", triangle()))
    for tag, R in records:
        o, t = fan((0.5, 0.5, 0), 2.0, 8, 12)
        d = (t - o).astype(f4)
        tiny = f4(1.0e-45)
        den = np.array([d * [0, 1, 1] + [tiny, 0, 0], d * [0, 0, 1] + [tiny, -tiny, 0], np.broadcast_to([tiny, tiny, -tiny], d.shape)], f4).reshape(-1, 3)
        out += [
            F("%s: a zero direction" % tag, R, np.concatenate([o, o]), np.concatenate([t, o])),
            F("%s: denormal direction components" % tag, R, np.concatenate([o] * 4), np.concatenate([t] * 4),
              directions=np.concatenate([d, den]), walk=False),
            F("%s: a direction of length 1e-12" % tag, R, np.concatenate([o, o]), np.concatenate([t, t]),
              directions=np.concatenate([d, d * f4(1.0e-12) / np.linalg.norm(d, axis=1, keepdims=True).astype(f4)]), walk=False),
            F("%s: a direction of length 1e12" % tag, R, np.concatenate([o, o]),
              np.concatenate([t, o + (t - o) * 1.0e12 / np.linalg.norm(t - o, axis=1, keepdims=True)])),
        ]
        ys = np.arange(-3.0, 5.25, 0.5)
        for sign in (1.0, -1.0):
            far = np.stack([np.full(len(ys), sign * VIEW_DISTANCE), ys, np.full(len(ys), 0.25)], 1)
            out.append(F("%s: an origin at %+d" % (tag, sign * VIEW_DISTANCE), [R, sphere(64.0)] if tag == "sphere" else R, far, far * [-1, 1, -1]))
    return out


def tie_families():
    """two identical records in one leaf, and in two leaves; two triangles of opposite winding that share an edge"""
    out = []
    for tag, R, centre in (("sphere", sphere(), (0, 0, 0)), ("triangle", triangle(), (1, 1, 0)), ("XZ plane", plane(M.ptXZPlane), (0, 0, 0))):
        o, t = fan(centre, 1.5, 16, 13)
        out.append(("tie: two identical %ss in one leaf" % tag, [R, R], False, o, t))
        out.append(("tie: two identical %ss in two leaves" % tag, [R, R], True, o, t))
    shared = [triangle((4, 0, 0), (0, 4, 0)), triangle((0, 4, 0), (4, 0, 0), p0=(4, 4, 0))]
    o = np.array([[k / 8.0, 4 - k / 8.0, 3] for k in range(33)] + [[k / 8.0 + 2.0 ** -20, 4 - k / 8.0, 3] for k in range(33)])
    out.append(("tie: an edge shared by two triangles of opposite winding", shared, False, o, o + [[0, 0, -16]]))
    return out


def families(solr, group):
    global _P
    _P = solr.PRIMITIVE_DTYPE
    g = GROUPS[group]
    eps, eq = g["geometryEpsilon"], group != "decimal"
    if group == "flat":
        return triangle_families(eps, eq, flat=True)
    if group == "camera":
        return camera_families()
    out = (sphere_families(eps, eq) + ellipsoid_families(eps, eq) + cylinder_families(eps, eq) + plane_families(eps, eq) +
           triangle_families(eps, eq))
    if group == "dyadic":
        out += every_type_families(eps)
    # the consecutive floats around a decision are for the families placed ON an equality; where none is placed (a
    # decimal epsilon; the unusual rays, which do not read it) the geometric steps say as much
    for f in out:
        if not f.equality:
            f.offsets = SPARSE if group == "decimal" else COARSE
    return out


def scene_info(group):
    from oracle import probes
    return probes._scene_info(viewDistance=VIEW_DISTANCE, **GROUPS[group])


# ---- per element ------------------------------------------------------------------------------------------------------------
_ELEMENT = {}


def element_case(solr, group):
    """-> the case (oracle.probes.case_primitive's layout; `family`: the family of every element) and its families"""
    if group not in _ELEMENT:
        fams = families(solr, group)
        parts = []
        for j, fam in enumerate(fams):
            recs, o, t = fam.realize((0, 0, 0))
            d = (t - o).astype(f4) if fam.directions is None else np.repeat(np.asarray(fam.directions, f4), len(fam.recs), 0)
            assert len(d) == len(o), fam.decision
            for shadows in (0, 1):
                parts.append((recs, o, d, np.full(len(o), shadows, i4), np.full(len(o), j, i4)))
        prims = stack([r for p in parts for r in p[0]])
        prims["index"] = np.arange(len(prims))
        n = len(prims)
        case = dict(name="primitive", si=scene_info(group), prims=prims, materials=materials(solr.MATERIAL_DTYPE),
                    textures=np.zeros(16, np.uint8), origins=np.ascontiguousarray(np.concatenate([p[1] for p in parts])),
                    directions=np.ascontiguousarray(np.concatenate([p[2] for p in parts])), shadows=np.concatenate([p[3] for p in parts]),
                    initial=np.zeros((n, 2, 3), f4), family=np.concatenate([p[4] for p in parts]))
        _ELEMENT[group] = (case, fams)
    return _ELEMENT[group]


# ---- through the walks ------------------------------------------------------------------------------------------------------
class Scene:
    """hand-made arrays in the shape of oracle.probes.SceneData (as tests/walk_margin_cases.py Scene)"""

    def __init__(self, solr, group, boxes, prims, lamp):
        from oracle import loader
        self._loader = loader
        self.boxes, self.prims, self.lamp = boxes, prims, lamp
        self.materials = materials(solr.MATERIAL_DTYPE)
        self.textures = np.zeros(16, np.uint8)
        self.lights = np.zeros(1, solr.LIGHT_DTYPE)
        self.lights["primitiveId"], self.lights["materialId"] = lamp, LAMP
        self.lights["location"], self.lights["color"] = prims["p0"][lamp], (1.0, 1.0, 1.0, 2.0)
        self.nb_lamps = 1
        self.randoms = np.zeros(0, f4)
        self.si = scene_info(group)
        self.ppi = solr.PostProcessingInfo()

    def oracle_scene(self):
        rnd = np.zeros(1, f4)
        self._keep = rnd          # (the oracle's scene holds its address: it must outlive the call)
        return self._loader.OracleScene(self.boxes.ctypes.data, len(self.boxes), self.prims.ctypes.data, len(self.prims),
                                        self.lights.ctypes.data, len(self.lights), self.nb_lamps, self.materials.ctypes.data,
                                        self.textures.ctypes.data, rnd.ctypes.data, len(rnd))


def _leaf_bounds(c, recs):
    """the leaf's cell, 16 wide - grown to what its records reach (a leaf holds what it names)"""
    lo, hi = np.asarray(c, f4) - f4(8), np.asarray(c, f4) + f4(8)
    for r in recs:
        reach = np.full(3, r["size"][0], f4) if int(r["type"]) in (M.ptSphere, M.ptEnvironment) else np.abs(r["size"])
        pts = [r["p0"] - reach, r["p0"] + reach]
        if int(r["type"]) in (M.ptTriangle, M.ptCylinder, M.ptCone):
            pts += [r["p1"] - reach, r["p1"] + reach, r["p2"]]
        lo, hi = np.minimum(lo, np.min(pts, axis=0)), np.maximum(hi, np.max(pts, axis=0))
    return lo, hi


_WALK = {}


PARTS = ("kinds", "general")
WALKS = (("dyadic", "kinds"), ("dyadic", "general"), ("decimal", "kinds"), ("decimal", "general"), ("flat", "kinds"))


def _contained(r):
    """engine.h primitiveContained: the types whose leaves hold them by the reference's builder.  A scene of nothing else is
    offered the order-free lists and the lamp's cut-off - the types with a short path of their own, all of them"""
    return int(r["type"]) in (M.ptTriangle, M.ptCylinder, M.ptXYPlane, M.ptYZPlane, M.ptXZPlane) or \
        (int(r["type"]) == M.ptSphere and int(r["materialId"]) != PROC)


def lattice(solr, group, part, thin=1):
    """-> Scene, rays: the families of the group that go into a walk, each in a leaf of its own (one leaf per distinct set
    of records, at most 64), and the ties.  part: `kinds` - the families whose records are all of the types the engine takes
    for contained (above); `general` - the others (cones, ellipsoids, procedural spheres, the environment, checkerboard and
    carpet): two lattices, because one such record keeps the order-free lists from the whole scene.  rays: dict(origins, targets, current, family, own (the primitive a ray is aimed
    at), decisions).  thin: every thin-th stepped ray is kept (the Python model walks these rays too)"""
    if (group, part, thin) in _WALK:
        return _WALK[(group, part, thin)]
    B = solr.BOX_DTYPE
    fams = [f for f in families(solr, group) if f.walk and all(_contained(r) for r in f.recs) == (part == "kinds")]
    leaves, prims, rays, decisions = [], [], [], []
    where = {}

    def leaf(c, recs, tiny_first):
        recs = list(recs)
        if tiny_first:
            t = sphere(2.0 ** -6)
            t["p0"] = np.asarray(c, f4) + f4(7)
            recs = [t] + recs
        lo, hi = _leaf_bounds(c, recs)
        leaves.append((lo, hi, len(recs), len(prims)))
        first = len(prims) + (1 if tiny_first else 0)
        prims.extend(recs)
        return first

    def add(decision, fam_index, first, n_recs, o, t, current):
        per = np.arange(len(o)) % n_recs
        rays.append((o, t, np.full(len(o), current, i4), np.full(len(o), fam_index, i4), (first + per).astype(i4)))

    for j, fam in enumerate(fams):
        key = b"".join(r.tobytes() for r in fam.recs)
        if key not in where:
            assert len(where) + 10 < len(LATTICE), "no leaf left for " + fam.decision      # (ten leaves are the ties')
            c = LATTICE[len(where)]
            recs, _, _ = fam.realize(c)
            where[key] = (c, leaf(c, recs[: len(fam.recs)], len(where) % 2 == 1))
        c, first = where[key]
        _, o, t = fam.realize(c)
        keep = np.arange(len(o)) if fam.mode is None else np.flatnonzero((np.arange(len(o)) % thin == 0) | (np.arange(len(o)) < 9))
        decisions.append(fam.decision)
        add(fam.decision, len(decisions) - 1, first, len(fam.recs), o[keep], t[keep], fam.current)
    if group == "dyadic" and part == "kinds":
        at = len(where)
        for decision, recs, two_leaves, o, t in tie_families():
            c = np.asarray(LATTICE[at], f4)
            at += 1
            moved = []
            for r in recs:
                r = r.copy()
                for k in ("p0", "p1", "p2"):
                    r[k] = r[k] + c
                moved.append(r)
            first = leaf(c, moved[:1] if two_leaves else moved, False)
            if two_leaves:
                leaf(c, moved[1:], False)
            decisions.append(decision)
            add(decision, len(decisions) - 1, first, 1, (o + c).astype(f4), (t + c).astype(f4), -2)
    lamp = sphere(1.0, LAMP, p0=LAMP_AT)
    leaf(LAMP_AT, [lamp], False)
    boxes = np.zeros(len(leaves) + 1, B)
    for k, (lo, hi, count, start) in enumerate(leaves):
        boxes[k + 1]["min"], boxes[k + 1]["max"] = lo, hi
        boxes[k + 1]["nbPrimitives"], boxes[k + 1]["startIndex"], boxes[k + 1]["indexForNextBox"] = count, start, (1, 0)
    boxes[0]["min"], boxes[0]["max"] = boxes["min"][1:].min(axis=0), boxes["max"][1:].max(axis=0)
    boxes[0]["indexForNextBox"] = (len(boxes), 0)
    records = stack(prims)
    records["index"] = np.arange(len(records))
    sc = Scene(solr, group, boxes, records, len(records) - 1)
    out = dict(origins=np.ascontiguousarray(np.concatenate([r[0] for r in rays]).astype(f4)),
               targets=np.ascontiguousarray(np.concatenate([r[1] for r in rays]).astype(f4)),
               current=np.concatenate([r[2] for r in rays]), family=np.concatenate([r[3] for r in rays]),
               own=np.concatenate([r[4] for r in rays]), decisions=decisions)
    _WALK[(group, part, thin)] = (sc, out)
    return sc, out


def walk_case(kind, sc, rays, order=None, ragged=None):
    """a closest-hit or shadow case of the lattice's rays in the given order; ragged: its first rays once more at the end,
    until the case is that many rays beyond a multiple of 64 (no ray is left out)"""
    order = np.arange(len(rays["origins"])) if order is None else np.asarray(order)
    if ragged is not None:
        order = np.concatenate([order, order[: (ragged - len(order)) % WAVE]])
    n = len(order)
    o, t = np.ascontiguousarray(rays["origins"][order]), np.ascontiguousarray(rays["targets"][order])
    extra = dict(family=rays["family"][order].copy(), own=rays["own"][order].copy(), order=order.astype(i4))
    if kind == "closest":
        return dict(name="closest", scene=sc, si=sc.si, origins=o, targets=t, iteration=np.zeros(n, i4),
                    current=np.ascontiguousarray(rays["current"][order]), **extra)
    return dict(name="shadow", scene=sc, si=sc.si, lamps=t, origins=o, object_id=np.full(n, sc.lamp, i4),
                iteration=np.zeros(n, i4), **extra)


def interleaved(hits):
    """an order in which every wave of 64 holds exactly one ray that hits, for as long as the rays that miss last (63 a
    wave); the rest follows as it came.  hits: per ray, from the oracle - used to compose waves, nothing else"""
    hit, miss = list(np.flatnonzero(hits)), list(np.flatnonzero(~np.asarray(hits, bool)))
    waves = min(len(hit), len(miss) // (WAVE - 1))
    order = []
    for w in range(waves):
        lane = (17 * w) % WAVE
        block = miss[w * (WAVE - 1): (w + 1) * (WAVE - 1)]
        order += block[:lane] + [hit[w]] + block[lane:]
    return np.array(order + hit[waves:] + miss[waves * (WAVE - 1):], np.int64), waves


def one_hit_waves(hits, family, most=90):
    """waves of exactly one ray that hits among 63 that miss, the rays that miss taken again and again: one wave per
    family that has a hit, then a second one, ... up to `most` waves.  -> the order (rays repeat), the number of waves"""
    hits = np.asarray(hits, bool)
    miss = np.flatnonzero(~hits)
    per_family = [list(np.flatnonzero(hits & (family == f))) for f in range(int(family.max()) + 1)]
    chosen, depth = [], 0
    while len(chosen) < most and any(len(x) > depth for x in per_family):
        chosen += [x[(7 * depth) % len(x)] for x in per_family if len(x) > depth]
        depth += 1
    chosen = chosen[:most]
    order = []
    for w, h in enumerate(chosen):
        lane = (17 * w) % WAVE
        block = [int(miss[(w * (WAVE - 1) + k) % len(miss)]) for k in range(WAVE - 1)]
        order += block[:lane] + [int(h)] + block[lane:]
    return np.array(order, np.int64), len(chosen)


def count_by_decision(fams):
    """decision -> [families built, equalities claimed]"""
    table = {}
    for f in fams:
        row = table.setdefault(f.decision, [0, 0])
        row[0] += 1
        row[1] += 1 if f.equality else 0
    return table
