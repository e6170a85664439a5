"""The cases of tests/primitive_edge_cases.py are worth comparing (CPU): on every element and every ray of them

  * the oracle in dialect 0 gives the bits of the independent reading of the CUDA text (tests/cuda_text_model.py) - per
    element hit flag, hit point, normal, areas and shadow intensity; through the walks every output of
    intersection_with_primitives and process_shadows.  What a miss leaves in the outputs is nobody's business
    (tests/test_engine_probes_gpu.py); no element is left out for any other reason;
  * every family holds both outcomes by the model, and a family aimed at an equality holds an element ON it: the mutant of
    the model that differs only in the strictness of that comparison (`<` for `<=`, an `== 0` dropped) can differ from the
    model nowhere else, so it is the model's own arithmetic that says the compared numbers were equal;
  * every wrong restatement in MUTANTS is told apart from the model by some element; the pinned tables say which decisions
    are held by how many families and equalities;
  * the generator is deterministic (the digests are checked again on the GPU, tests/test_primitive_edges_gpu.py).
"""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cuda_text_model as M  # noqa: E402
import primitive_edge_cases as G  # noqa: E402
import text_mutants  # noqa: E402

F = np.float32
GROUP_NAMES = ("dyadic", "decimal", "flat", "camera")
THIN = {"dyadic": 1, "decimal": 1, "flat": 1}      # every n-th stepped ray goes through the walks (the Python model walks them)


# ---- the model over the cases -------------------------------------------------------------------------------------------------
def _model_scene(case_or_scene, boxes=None, lights=None):
    prims = case_or_scene["prims"] if isinstance(case_or_scene, dict) else case_or_scene.prims
    mats = case_or_scene["materials"] if isinstance(case_or_scene, dict) else case_or_scene.materials
    flat = types.SimpleNamespace(boxes=np.zeros(0, [("min", F, 3), ("max", F, 3), ("nbPrimitives", "i4"), ("startIndex", "i4"),
                                                     ("indexForNextBox", "i4", 2)]) if boxes is None else boxes,
                                 primitives=prims, lights=np.zeros(0, [("primitiveId", "i4"), ("materialId", "i4"), ("location", F, 3),
                                                                       ("color", F, 4)]) if lights is None else lights,
                                 materials=mats[:16], randoms=np.zeros(1, F))
    return M.Scene(flat)


def model_elements(case, only=None):
    """per element: None (a miss) or (intersection, normal, areas, shadow intensity) by the text model"""
    if case.get("_model") is None:
        case["_model"] = _model_scene(case)          # (not an array: no part of the digest)
    s = case["_model"]
    si = case["si"]
    out = {}
    with np.errstate(all="ignore"):
        for e in (range(len(case["origins"])) if only is None else only):
            r = M.compute_ray_attributes(M.v(*case["origins"][e]), M.v(*case["directions"][e]))
            p = s.P[e]
            if case["shadows"][e]:
                h = M._dispatch_shadow(si, s, p, r)
                out[e] = None if not h else (h[0], h[1], h[3] if len(h) > 3 else M.v(0, 0, 0), h[2])
            else:
                hit, inter, normal, areas = M._dispatch_closest(si, s, p, r)
                if not hit:
                    out[e] = None
                else:   # the shadow intensity a closest-hit test leaves: the test's own
                    t = p["type"] if si.extendedGeometry else M.ptTriangle
                    if t in (M.ptSphere, M.ptEnvironment):
                        shadow = M.sphere_intersection(si, s, p, r)[2]
                    elif t in (M.ptCylinder, M.ptCone, M.ptEllipsoid, M.ptTriangle):
                        shadow = F(1)
                    else:
                        shadow = M.plane_intersection(si, s, p, r)[0][2]
                    out[e] = (inter, normal, areas, shadow)
    return out


def _same(a, b):
    from oracle import probes
    return bool(np.all(probes.same_bits(np.array(a, F), np.array(b, F))))


def outcomes_equal(x, y):
    if x is None or y is None:
        return x is None and y is None
    return all(_same(a, b) for a, b in zip(x, y))


def model_walk(kind, sc, rays):
    """per ray of the lattice: the model's closest hit (hit, primitive, point, normal, areas) or shadow (result, colour)"""
    s = _model_scene(sc, sc.boxes, sc.lights)
    out = []
    with np.errstate(all="ignore"):
        for e in range(len(rays["origins"])):
            o, t = M.v(*rays["origins"][e]), M.v(*rays["targets"][e])
            if kind == "closest":
                out.append(M.intersection_with_primitives(sc.si, s, o, t, 0, int(rays["current"][e]), [F(0)] * 3))
            else:
                out.append(M.process_shadows(sc.si, s, t, o, sc.lamp, 0, -12345))
    return out


# ---- mutants of the model ------------------------------------------------------------------------------------------------------
# name -> (function of cuda_text_model, text, replacement, which occurrence (None: the only one)).  Strictness mutants first.
def _plane_mutants():
    out = {}
    branches = {"carpet": ("t in (ptMagicCarpet, ptCheckboard)", 1, "ix", 0, "iz", 2), "XZ": ("t == ptXZPlane", 1, "ix", 0, "iz", 2),
                "YZ": ("t == ptYZPlane", 0, "iy", 1, "iz", 2), "XY": ("t in (ptXYPlane, ptCamera)", 2, "ix", 0, "iy", 1)}
    for tag, (_, w, iu, u, iv, v) in branches.items():
        for face, dcmp, ocmp in (("front", "<", ">"), ("rear", ">", "<")):
            if tag == "carpet" and face == "rear":
                continue
            nth = {("carpet", "front"): 0, ("XZ", "front"): 1}.get((tag, face))
            names = ["checkerboard", "carpet"] if tag == "carpet" else [tag]
            side = "rev * d[%d] %s F(0) and rev * o[%d] %s rev * p0[%d]" % (w, dcmp, w, ocmp, w)
            flipped = "rev * d[%d] %s F(0) and rev * o[%d] %s= rev * p0[%d]" % (w, dcmp, w, ocmp, w)
            for n in names:
                out["plane %s %s o.W" % (n, face)] = ("plane_intersection", side, flipped, nth)
            # the rectangle: front and rear of a branch are the 1st and 2nd occurrence of the same line within it
            line = "collision = abs(%s - p0[%d]) < size[%d] and abs(%s - p0[%d]) < size[%d]" % (iu, u, u, iv, v, v)
            if tag in ("carpet", "XZ"):
                k = 0 if tag == "carpet" else (1 if face == "front" else 2)
            else:
                k = 0 if face == "front" else 1
            for n in names:
                out["plane %s %s edge %s" % (n, face, "xyz"[u])] = ("plane_intersection", line, line.replace("< size[%d] and" % u, "<= size[%d] and" % u), k)
                out["plane %s %s edge %s" % (n, face, "xyz"[v])] = ("plane_intersection", line, line[:-len("< size[%d]" % v)] + "<= size[%d]" % v, k)
    return out


MUTANTS = {
    "sphere d <= 0": ("sphere_intersection", "if d <= F(0) or a == F(0):", "if d < F(0) or a == F(0):", None),
    "sphere both: t2 <= eps": ("sphere_intersection", "if t1 <= eps and t2 <= eps:", "if t1 <= eps and t2 < eps:", None),
    "sphere t1 <= eps": ("sphere_intersection", "    if t1 <= eps:\n        t = t2", "    if t1 < eps:\n        t = t2", None),
    "ellipsoid d < 0": ("ellipsoid_intersection", "if d < F(0) or a == F(0)", "if d <= F(0) or a == F(0)", None),
    "ellipsoid b == 0": ("ellipsoid_intersection", " or b == F(0)", "", None),
    "ellipsoid c == 0": ("ellipsoid_intersection", " or c == F(0)", "", None),
    "ellipsoid elif t2 <= eps": ("ellipsoid_intersection", "elif t2 <= eps:", "elif t2 < eps:", None),
    "cylinder ln < eps": ("cylinder_intersection", "if ln < eps and ln > -eps:", "if ln <= eps and ln > -eps:", None),
    "cylinder d > size.y": ("cylinder_intersection", 'if d > p["size"][1]:', 'if d >= p["size"][1]:', None),
    "cylinder t < 0": ("cylinder_intersection", "if t < F(0):", "if t <= F(0):", None),
    "cylinder scale1 < eps (near)": ("cylinder_intersection", "if scale1 < eps or scale2 > eps:", "if scale1 <= eps or scale2 > eps:", 0),
    "cylinder scale2 > eps (near)": ("cylinder_intersection", "if scale1 < eps or scale2 > eps:", "if scale1 < eps or scale2 >= eps:", 0),
    "cylinder scale1 < eps (far)": ("cylinder_intersection", "if scale1 < eps or scale2 > eps:", "if scale1 <= eps or scale2 > eps:", 1),
    "cylinder scale2 > eps (far)": ("cylinder_intersection", "if scale1 < eps or scale2 > eps:", "if scale1 < eps or scale2 >= eps:", 1),
    "plane colour key": ("plane_intersection", "/ F(3) >= F(si.transparentColor)", "/ F(3) > F(si.transparentColor)", None),
    "plane YZ chessboard z": ("plane_intersection", "to_int(abs(iz)) % 4000 < 2000", "to_int(abs(iz)) % 4000 <= 2000", 0),
    "plane YZ chessboard y": ("plane_intersection", "to_int(abs(iy)) % 4000 < 2000", "to_int(abs(iy)) % 4000 <= 2000", 0),
    "wireframe X <= width": ("wire_frame_mapping", "(X % 100 <= width)", "(X % 100 < width)", None),
    "wireframe Y <= width": ("wire_frame_mapping", "(Y % 100 <= width)", "(Y % 100 < width)", None),
    "triangle |det| < eps": ("triangle_intersection", "if abs(det) < eps:", "if abs(det) <= eps:", None),
    "triangle a < 0": ("triangle_intersection", "if a < F(0) or a > F(1):", "if a <= F(0) or a > F(1):", None),
    "triangle a > 1": ("triangle_intersection", "if a < F(0) or a > F(1):", "if a < F(0) or a >= F(1):", None),
    "triangle b < 0": ("triangle_intersection", "if b < F(0) or b > F(1):", "if b <= F(0) or b > F(1):", None),
    "triangle b > 1": ("triangle_intersection", "if b < F(0) or b > F(1):", "if b < F(0) or b >= F(1):", None),
    "triangle a + b > 1": ("triangle_intersection", "if (a + b) > F(1):", "if (a + b) >= F(1):", None),
    "triangle t < 0": ("triangle_intersection", "    if t < F(0):", "    if t <= F(0):", None),
    "triangle r > 0": ("triangle_intersection", "if rr > F(0):", "if rr >= F(0):", None),
    # ---- wrong restatements that are no change of strictness
    "sphere: the two roots exchanged": ("sphere_intersection", "t1 = (-b - rt) / a\n    t2 = (-b + rt) / a", "t1 = (-b + rt) / a\n    t2 = (-b - rt) / a", None),
    "sphere: the back flag dropped": ("sphere_intersection", "        back = True\n", "", None),
    "cylinder: size.y read as size.x": ("cylinder_intersection", 'if d > p["size"][1]:', 'if d > p["size"][0]:', None),
    "cylinder: ray.d read as the normalised direction": ("cylinder_intersection", "d_ = r.direction", "d_ = normalize(r.direction)", None),
    "triangle: ray.d read as the normalised direction": ("triangle_intersection", '    E01 = sub(p["p1"], p["p0"])',
                                                         '    r = _unit_ray(r)\n    E01 = sub(p["p1"], p["p0"])', None),
    "triangle: E21 corrected to p1 - p2": ("triangle_intersection", 'E21 = sub(p["p1"], p["p1"])', 'E21 = sub(p["p1"], p["p2"])', None),
    "plane: the rear face does not negate the normal": ("plane_intersection", "normal = neg(normal)", "normal = normal", "all"),
}
MUTANTS.update(_plane_mutants())

# Strictness mutants that no binary32 input can tell from the model, with the argument; not built, not counted above.
UNREACHABLE = {
    "sphere both: t1 <= eps": "t1 == eps with t2 <= eps needs t1 == t2, the root of d lost in b: rt < 2^-24 |b|.  But d = b * b - 2 a c "
                              "is a difference of two binary32 numbers no larger than b * b: not 0, it is at least 2^-25 b * b, rt > 2^-13 |b|",
    "sphere elif t2 <= eps": "reached with t1 > eps only, and t2 = (-b + rt) / a >= (-b - rt) / a = t1 for rt >= 0, a > 0: t2 > eps",
    "sphere final t < eps": "t is t2 > eps (t1 <= eps, not both), t1 > eps, or the smaller of two numbers > eps: never below eps",
    "ellipsoid if t1 <= eps": "t1 is the larger root ((-b + d) / 2a, d >= 0, a > 0): t1 <= eps implies t2 <= eps, refused the line before",
    "ellipsoid final t < eps": "as the sphere's",
    "plane d.W < 0 / > 0": "at d.W == 0 the point k * d.U / -0 is infinite or no number: inside no rectangle of finite size, whatever "
                           "the side predicate said",
    "cylinder ln > -eps": "ln is a length: never negative",
    "triangle b > 1 dropped": "no strictness, but the same kind: b > 1 with a >= 0 gives a + b > 1, and the test behind that, with "
                              "E21 = p1 - p1, has det_ = 0 and refuses everything (an engine without the clause passes every test)",
    "ellipsoid: the two roots exchanged": "the choice of t is symmetric in t1 and t2, and there is no back flag",
}


def _unit_ray(r):
    return M.compute_ray_attributes(r.origin, M.normalize(r.direction))


def mutant(name):
    return text_mutants.mutant(MUTANTS, name, dict(_unit_ray=_unit_ray))


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def elements(solr, oracle):
    """per group: the case, its families, the oracle's outputs (dialect 0) and the model's outcomes - computed once"""
    from oracle import probes
    L = oracle.lib()
    assert L.oracle_get_dialect() == 0
    out = {}
    L.oracle_set_rounded_transcendentals(1)      # the model's form of the procedural sphere's cos / sin
    try:
        for group in GROUP_NAMES:
            case, fams = G.element_case(solr, group)
            out[group] = (case, fams, probes._oracle_outputs(L, case), model_elements(case))
    finally:
        L.oracle_set_rounded_transcendentals(0)
    return out


@pytest.fixture(scope="module")
def walks(solr, oracle):
    from oracle import probes
    L = oracle.lib()
    assert L.oracle_get_dialect() == 0
    out = {}
    L.oracle_set_rounded_transcendentals(1)
    try:
        for group, part in G.WALKS:
            sc, rays = G.lattice(solr, group, part, THIN[group])
            for kind in ("closest", "shadow"):
                case = G.walk_case(kind, sc, rays)
                out[(group, part, kind)] = (sc, rays, case, probes._oracle_outputs(L, case), model_walk(kind, sc, rays))
    finally:
        L.oracle_set_rounded_transcendentals(0)
    return out


# ---- the tests -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUP_NAMES)
def test_the_oracle_equals_the_text_model_on_every_element(elements, group):
    case, fams, got, want = elements[group]
    bad = []
    for e in range(len(case["origins"])):
        w = want[e]
        if (w is not None) != bool(got["hit"][e]):
            bad.append((e, "hit"))
        elif w is not None:
            mine = (got["intersection"][e], got["normal"][e], got["areas"][e], got["shadow"][e])
            for key, a, b in zip(("intersection", "normal", "areas", "shadow"), mine, w):
                if not _same(a, b):
                    bad.append((e, key))
    hits = sum(1 for w in want.values() if w is not None)
    print("%s: %d elements, %d hits by the model, %d differ" % (group, len(want), hits, len(bad)))
    assert (0.15 if group == "camera" else 0.2) < hits / len(want) < 0.8      # (a ptCamera record shadows nothing, GI:861)
    assert not bad, [(e, key, fams[case["family"][e]].decision, int(case["shadows"][e])) for e, key in bad[:20]]


@pytest.mark.parametrize("group,part", G.WALKS)
@pytest.mark.parametrize("kind", ["closest", "shadow"])
def test_the_oracle_equals_the_text_model_on_every_ray_of_the_walks(walks, group, part, kind):
    sc, rays, case, got, want = walks[(group, part, kind)]
    bad = []
    for e, w in enumerate(want):
        if kind == "closest":
            if bool(w[0]) != bool(got["hit"][e]):
                bad.append((e, "hit"))
            elif w[0]:
                if int(got["primitive"][e]) != w[1]:
                    bad.append((e, "primitive"))
                for key, b in zip(("intersection", "normal", "areas"), w[2:]):
                    if not _same(got[key][e], b):
                        bad.append((e, key))
        else:
            if not _same(got["result"][e], w[0]) or not _same(got["color"][e], w[1]):
                bad.append((e, "shadow"))
    hit = [bool(w[0]) if kind == "closest" else bool(w[0] > 0) for w in want]
    print("%s %s %s: %d rays over %d leaves, %d hit, %d differ" % (group, part, kind, len(want), len(sc.boxes) - 1, sum(hit), len(bad)))
    assert len(want) <= 6200 and len(sc.boxes) - 2 <= 64
    assert sum(hit) > len(hit) // (20 if group == "decimal" and kind == "shadow" else 8)
    assert not bad, [(e, key, rays["decisions"][rays["family"][e]]) for e, key in bad[:20]]


def test_a_ray_meets_in_the_lattice_what_it_meets_alone(solr, walks):
    """the per-primitive outcome is unchanged by the walk around it: where the walk's closest hit is the record a ray was
    aimed at, it is the hit point and normal the model gives for that record and that ray alone, and where the ray alone hits
    its record farther than epsilon the walk finds that record or something nearer"""
    for group, part in G.WALKS:
        sc, rays, case, got, want = walks[(group, part, "closest")]
        s = _model_scene(sc, sc.boxes, sc.lights)
        own_hits = 0
        with np.errstate(all="ignore"):
            for e, w in enumerate(want):
                p = s.P[int(rays["own"][e])]
                m = s.material(p["mat"])
                if m["attributes"][0] == 1 and int(rays["current"][e]) == p["mat"]:
                    continue
                o, t = M.v(*rays["origins"][e]), M.v(*rays["targets"][e])
                r = M.compute_ray_attributes(o, M.sub(t, o))
                hit, inter, normal, areas = M._dispatch_closest(sc.si, s, p, r)
                if w[0] and w[1] == int(rays["own"][e]):
                    own_hits += 1
                    assert hit and _same(inter, w[2]) and _same(normal, w[3]), (group, e)
                elif hit:
                    distance = M.length(M.sub(inter, o))
                    if distance > F(sc.si.geometryEpsilon) and distance < F(sc.si.viewDistance):
                        assert w[0] and M.length(M.sub(w[2], o)) <= distance, (group, e, rays["decisions"][rays["family"][e]])
        assert own_hits > len(want) // 4, (group, own_hits)


def _family_elements(case, j):
    return np.flatnonzero(case["family"] == j)


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_every_family_holds_both_outcomes(elements, group):
    case, fams, got, want = elements[group]
    single = []
    for j, fam in enumerate(fams):
        es = _family_elements(case, j)
        es = es[case["shadows"][es] == 0]
        seen = []
        for e in es:
            if not any(outcomes_equal(want[e], x) for x in seen):
                seen.append(want[e])
        if len(seen) < 2:
            single.append(fam.decision)
    assert not single, single


EQUALITIES = {'dyadic': 97, 'flat': 13, 'camera': 11}


@pytest.mark.parametrize("group", ["dyadic", "flat", "camera"])
def test_a_family_aimed_at_an_equality_holds_an_element_on_it(elements, group):
    """... by the model's own arithmetic: its strictness mutant differs from it on an element of the family"""
    case, fams, got, want = elements[group]
    missing, found = [], 0
    for j, fam in enumerate(fams):
        if not fam.equality:
            continue
        es = _family_elements(case, j)
        with mutant(fam.equality):
            other = model_elements(case, es)
        if any(not outcomes_equal(other[e], want[e]) for e in es):
            found += 1
        else:
            missing.append((fam.decision, fam.equality))
    assert not missing, missing
    assert found == EQUALITIES[group], found


def test_every_mutant_is_told_apart(elements):
    """every wrong restatement gives another result on some element of the per-element cases"""
    unnoticed = []
    for name in MUTANTS:
        func = MUTANTS[name][0]
        noticed = False
        for group in ("dyadic", "flat", "decimal", "camera"):
            case, fams, got, want = elements[group]
            word = {"sphere_intersection": ("sphere", "environment"), "ellipsoid_intersection": ("ellipsoid",),
                    "cylinder_intersection": ("cylinder", "cone"), "triangle_intersection": ("triangle", "flat"),
                    "plane_intersection": ("plane", "camera"), "wire_frame_mapping": ("wireframe",)}[func]
            es = np.flatnonzero([any(w in fams[j].decision.split(":")[0] or w in fams[j].decision for w in word) for j in case["family"]])
            with mutant(name):
                other = model_elements(case, es)
            if any(not outcomes_equal(other[e], want[e]) for e in es):
                noticed = True
                break
        if not noticed:
            unnoticed.append(name)
    assert not unnoticed, unnoticed


MUTANT_NAMES = ['cylinder d > size.y', 'cylinder ln < eps', 'cylinder scale1 < eps (far)', 'cylinder scale1 < eps (near)',
 'cylinder scale2 > eps (far)', 'cylinder scale2 > eps (near)', 'cylinder t < 0',
 'cylinder: ray.d read as the normalised direction', 'cylinder: size.y read as size.x', 'ellipsoid b == 0', 'ellipsoid c == 0',
 'ellipsoid d < 0', 'ellipsoid elif t2 <= eps', 'plane XY front edge x', 'plane XY front edge y', 'plane XY front o.W',
 'plane XY rear edge x', 'plane XY rear edge y', 'plane XY rear o.W', 'plane XZ front edge x', 'plane XZ front edge z',
 'plane XZ front o.W', 'plane XZ rear edge x', 'plane XZ rear edge z', 'plane XZ rear o.W', 'plane YZ chessboard y',
 'plane YZ chessboard z', 'plane YZ front edge y', 'plane YZ front edge z', 'plane YZ front o.W', 'plane YZ rear edge y',
 'plane YZ rear edge z', 'plane YZ rear o.W', 'plane carpet front edge x', 'plane carpet front edge z',
 'plane carpet front o.W', 'plane checkerboard front edge x', 'plane checkerboard front edge z', 'plane checkerboard front o.W',
 'plane colour key', 'plane: the rear face does not negate the normal', 'sphere both: t2 <= eps', 'sphere d <= 0',
 'sphere t1 <= eps', 'sphere: the back flag dropped', 'sphere: the two roots exchanged', 'triangle a + b > 1', 'triangle a < 0',
 'triangle a > 1', 'triangle b < 0', 'triangle b > 1', 'triangle r > 0', 'triangle t < 0', 'triangle |det| < eps',
 'triangle: E21 corrected to p1 - p2', 'triangle: ray.d read as the normalised direction', 'wireframe X <= width',
 'wireframe Y <= width']


def test_the_list_of_mutants_is_pinned():
    assert sorted(MUTANTS) == sorted(MUTANT_NAMES), sorted(set(MUTANTS) ^ set(MUTANT_NAMES))
    assert not set(UNREACHABLE) & set(MUTANTS)


# group -> decision -> [families built, equalities claimed]
DECISIONS = {'dyadic': {'sphere: d <= 0': [1, 1],
            'sphere: t1 <= eps (the back flag)': [1, 1],
            'sphere: t2 <= eps (going out)': [1, 1],
            'sphere: both roots behind': [1, 0],
            'sphere: origin on the surface going in': [1, 0],
            'sphere: origin at the centre': [1, 0],
            'sphere: radius 0': [1, 0],
            'environment: d <= 0': [1, 1],
            'environment: t1 <= eps (the back flag)': [1, 1],
            'environment: t2 <= eps (going out)': [1, 1],
            'environment: both roots behind': [1, 0],
            'environment: origin on the surface going in': [1, 0],
            'environment: origin at the centre': [1, 0],
            'environment: radius 0': [1, 0],
            'sphere: radius 0.5 at 1e4 (cancellation in c)': [1, 0],
            'sphere: transparent (1 - |r|)': [1, 0],
            'sphere: transparent, d <= 0': [1, 1],
            'sphere: procedural': [1, 0],
            'sphere: procedural, t1 <= eps': [1, 1],
            'sphere: fast transparency, another material current': [1, 0],
            'sphere: fast transparency, its own material current': [1, 0],
            'ellipsoid: d < 0': [1, 1],
            'ellipsoid: b == 0': [1, 1],
            'ellipsoid: c == 0': [1, 1],
            'ellipsoid: c == 0 going out': [1, 0],
            'ellipsoid: t2 <= eps (near root)': [1, 1],
            'ellipsoid: t1 <= eps (far root)': [1, 0],
            'ellipsoid: from outside, both roots ahead': [1, 0],
            'ellipsoid: a size component of 0': [1, 0],
            'cylinder: |cross(dir, n1)| against eps': [1, 1],
            'cylinder: along the axis, and at 1e-7, 1e-4, 1e-3 of it': [1, 0],
            'cylinder: d > size.y': [1, 1],
            'cylinder: d > size.y, size.y != size.x': [1, 1],
            'cylinder: size.y != size.x, between the two': [1, 0],
            'cylinder: t < 0 (closest approach at the origin)': [1, 1],
            'cylinder: scale1 < eps at the near root': [1, 1],
            'cylinder: scale2 > eps at the near root': [1, 1],
            'cylinder: scale1 < eps at the far root': [1, 1],
            'cylinder: scale2 > eps at the far root': [1, 1],
            'cylinder: from inside': [1, 0],
            'cylinder: p0 == p1 (n1 = 0)': [1, 0],
            'cylinder: n1 is not normalize(p1 - p0)': [1, 0],
            'cylinder: dot(dir, O) == 0': [1, 0],
            'cone: |cross(dir, n1)| against eps': [1, 1],
            'cone: along the axis, and at 1e-7, 1e-4, 1e-3 of it': [1, 0],
            'cone: d > size.y': [1, 1],
            'cone: d > size.y, size.y != size.x': [1, 1],
            'cone: size.y != size.x, between the two': [1, 0],
            'cone: t < 0 (closest approach at the origin)': [1, 1],
            'cone: scale1 < eps at the near root': [1, 1],
            'cone: scale2 > eps at the near root': [1, 1],
            'cone: scale1 < eps at the far root': [1, 1],
            'cone: scale2 > eps at the far root': [1, 1],
            'cone: from inside': [1, 0],
            'cone: p0 == p1 (n1 = 0)': [1, 0],
            'cone: n1 is not normalize(p1 - p0)': [1, 0],
            'cone: dot(dir, O) == 0': [1, 0],
            'plane XY front: |I.x - p0.x| < size.x': [2, 2],
            'plane XY front: |I.y - p0.y| < size.y': [2, 2],
            'plane XY front: a corner': [1, 0],
            'plane XY front: o.W against p0.W': [1, 1],
            'plane XY rear: |I.x - p0.x| < size.x': [2, 2],
            'plane XY rear: |I.y - p0.y| < size.y': [2, 2],
            'plane XY rear: a corner': [1, 0],
            'plane XY rear: o.W against p0.W': [1, 1],
            'plane XY: d.W through 0': [1, 0],
            'plane YZ front: |I.y - p0.y| < size.y': [2, 2],
            'plane YZ front: |I.z - p0.z| < size.z': [2, 2],
            'plane YZ front: a corner': [1, 0],
            'plane YZ front: o.W against p0.W': [1, 1],
            'plane YZ rear: |I.y - p0.y| < size.y': [2, 2],
            'plane YZ rear: |I.z - p0.z| < size.z': [2, 2],
            'plane YZ rear: a corner': [1, 0],
            'plane YZ rear: o.W against p0.W': [1, 1],
            'plane YZ: d.W through 0': [1, 0],
            'plane XZ front: |I.x - p0.x| < size.x': [2, 2],
            'plane XZ front: |I.z - p0.z| < size.z': [2, 2],
            'plane XZ front: a corner': [1, 0],
            'plane XZ front: o.W against p0.W': [1, 1],
            'plane XZ rear: |I.x - p0.x| < size.x': [2, 2],
            'plane XZ rear: |I.z - p0.z| < size.z': [2, 2],
            'plane XZ rear: a corner': [1, 0],
            'plane XZ rear: o.W against p0.W': [1, 1],
            'plane XZ: d.W through 0': [1, 0],
            'plane checkerboard front: |I.x - p0.x| < size.x': [2, 2],
            'plane checkerboard front: |I.z - p0.z| < size.z': [2, 2],
            'plane checkerboard front: a corner': [1, 0],
            'plane checkerboard front: o.W against p0.W': [1, 1],
            'plane checkerboard rear: |I.x - p0.x| < size.x': [2, 0],
            'plane checkerboard rear: |I.z - p0.z| < size.z': [2, 0],
            'plane checkerboard rear: a corner': [1, 0],
            'plane checkerboard rear: o.W against p0.W': [1, 0],
            'plane checkerboard: d.W through 0': [1, 0],
            'plane carpet front: |I.x - p0.x| < size.x': [2, 2],
            'plane carpet front: |I.z - p0.z| < size.z': [2, 2],
            'plane carpet front: a corner': [1, 0],
            'plane carpet front: o.W against p0.W': [1, 1],
            'plane carpet rear: |I.x - p0.x| < size.x': [2, 0],
            'plane carpet rear: |I.z - p0.z| < size.z': [2, 0],
            'plane carpet rear: a corner': [1, 0],
            'plane carpet rear: o.W against p0.W': [1, 0],
            'plane carpet: d.W through 0': [1, 0],
            'plane: averageColor >= transparentColor': [2, 2],
            'plane YZ emissive: (int)|I.y| % 4000 < 2000': [3, 2],
            'plane YZ emissive: (int)|I.z| % 4000 < 2000': [3, 2],
            'plane YZ emissive: small': [1, 0],
            'plane XY: wireframe width 0': [1, 1],
            'plane XY: wireframe width 0, the other axis': [1, 1],
            'plane YZ: wireframe width 0': [1, 1],
            'plane YZ: wireframe width 0, the other axis': [1, 1],
            'plane XZ: wireframe width 0': [1, 1],
            'plane XZ: wireframe width 0, the other axis': [1, 1],
            'plane XY: wireframe width 1': [1, 1],
            'plane XY: wireframe width 1, the other axis': [1, 1],
            'plane YZ: wireframe width 1': [1, 1],
            'plane YZ: wireframe width 1, the other axis': [1, 1],
            'plane XZ: wireframe width 1': [1, 1],
            'plane XZ: wireframe width 1, the other axis': [1, 1],
            'plane XY: wireframe width 255': [1, 0],
            'plane XY: wireframe width 255, the other axis': [1, 0],
            'plane YZ: wireframe width 255': [1, 0],
            'plane YZ: wireframe width 255, the other axis': [1, 0],
            'plane XZ: wireframe width 255': [1, 0],
            'plane XZ: wireframe width 255, the other axis': [1, 0],
            'triangle: a < 0': [1, 1],
            'triangle: a > 1 (the vertex p1)': [1, 1],
            'triangle: b < 0': [1, 1],
            'triangle: b > 1 (the vertex p2)': [1, 1],
            'triangle: the vertex p0': [1, 0],
            'triangle: a + b > 1': [1, 1],
            'triangle: a + b > 1, from below': [1, 1],
            'triangle: |det| < eps, det > 0': [1, 1],
            'triangle: |det| < eps, det < 0': [1, 1],
            'triangle: t < 0 at +0': [1, 1],
            'triangle: t < 0 at -0': [1, 1],
            'triangle: r > 0 (the flip of the normal)': [1, 1],
            'triangle: vertex normals whose weighted sum is 0': [1, 0],
            'triangle: three collinear points': [1, 0],
            'triangle: two equal points': [1, 0],
            'triangle: transparent': [1, 0],
            'triangle: along the hypotenuse': [1, 0],
            'triangle: along the hypotenuse, slanted': [1, 0],
            'triangle: along the edge p1 - p2, in general position': [1, 0],
            'sphere: a zero direction': [1, 0],
            'sphere: denormal direction components': [1, 0],
            'sphere: a direction of length 1e-12': [1, 0],
            'sphere: a direction of length 1e12': [1, 0],
            'sphere: an origin at +50000': [1, 0],
            'sphere: an origin at -50000': [1, 0],
            'ellipsoid: a zero direction': [1, 0],
            'ellipsoid: denormal direction components': [1, 0],
            'ellipsoid: a direction of length 1e-12': [1, 0],
            'ellipsoid: a direction of length 1e12': [1, 0],
            'ellipsoid: an origin at +50000': [1, 0],
            'ellipsoid: an origin at -50000': [1, 0],
            'cylinder: a zero direction': [1, 0],
            'cylinder: denormal direction components': [1, 0],
            'cylinder: a direction of length 1e-12': [1, 0],
            'cylinder: a direction of length 1e12': [1, 0],
            'cylinder: an origin at +50000': [1, 0],
            'cylinder: an origin at -50000': [1, 0],
            'cone: a zero direction': [1, 0],
            'cone: denormal direction components': [1, 0],
            'cone: a direction of length 1e-12': [1, 0],
            'cone: a direction of length 1e12': [1, 0],
            'cone: an origin at +50000': [1, 0],
            'cone: an origin at -50000': [1, 0],
            'XY plane: a zero direction': [1, 0],
            'XY plane: denormal direction components': [1, 0],
            'XY plane: a direction of length 1e-12': [1, 0],
            'XY plane: a direction of length 1e12': [1, 0],
            'XY plane: an origin at +50000': [1, 0],
            'XY plane: an origin at -50000': [1, 0],
            'triangle: a zero direction': [1, 0],
            'triangle: denormal direction components': [1, 0],
            'triangle: a direction of length 1e-12': [1, 0],
            'triangle: a direction of length 1e12': [1, 0],
            'triangle: an origin at +50000': [1, 0],
            'triangle: an origin at -50000': [1, 0]},
 'decimal': {'sphere: d <= 0': [1, 0],
             'sphere: t1 <= eps (the back flag)': [1, 0],
             'sphere: t2 <= eps (going out)': [1, 0],
             'sphere: both roots behind': [1, 0],
             'sphere: origin on the surface going in': [1, 0],
             'sphere: origin at the centre': [1, 0],
             'sphere: radius 0': [1, 0],
             'environment: d <= 0': [1, 0],
             'environment: t1 <= eps (the back flag)': [1, 0],
             'environment: t2 <= eps (going out)': [1, 0],
             'environment: both roots behind': [1, 0],
             'environment: origin on the surface going in': [1, 0],
             'environment: origin at the centre': [1, 0],
             'environment: radius 0': [1, 0],
             'sphere: radius 0.5 at 1e4 (cancellation in c)': [1, 0],
             'sphere: transparent (1 - |r|)': [1, 0],
             'sphere: transparent, d <= 0': [1, 0],
             'sphere: procedural': [1, 0],
             'sphere: procedural, t1 <= eps': [1, 0],
             'sphere: fast transparency, another material current': [1, 0],
             'sphere: fast transparency, its own material current': [1, 0],
             'ellipsoid: d < 0': [1, 0],
             'ellipsoid: b == 0': [1, 0],
             'ellipsoid: c == 0': [1, 0],
             'ellipsoid: c == 0 going out': [1, 0],
             'ellipsoid: t2 <= eps (near root)': [1, 0],
             'ellipsoid: t1 <= eps (far root)': [1, 0],
             'ellipsoid: from outside, both roots ahead': [1, 0],
             'ellipsoid: a size component of 0': [1, 0],
             'cylinder: |cross(dir, n1)| against eps': [1, 0],
             'cylinder: along the axis, and at 1e-7, 1e-4, 1e-3 of it': [1, 0],
             'cylinder: d > size.y': [1, 0],
             'cylinder: d > size.y, size.y != size.x': [1, 0],
             'cylinder: size.y != size.x, between the two': [1, 0],
             'cylinder: t < 0 (closest approach at the origin)': [1, 0],
             'cylinder: scale1 < eps at the near root': [1, 0],
             'cylinder: scale2 > eps at the near root': [1, 0],
             'cylinder: scale1 < eps at the far root': [1, 0],
             'cylinder: scale2 > eps at the far root': [1, 0],
             'cylinder: from inside': [1, 0],
             'cylinder: p0 == p1 (n1 = 0)': [1, 0],
             'cylinder: n1 is not normalize(p1 - p0)': [1, 0],
             'cylinder: dot(dir, O) == 0': [1, 0],
             'cone: |cross(dir, n1)| against eps': [1, 0],
             'cone: along the axis, and at 1e-7, 1e-4, 1e-3 of it': [1, 0],
             'cone: d > size.y': [1, 0],
             'cone: d > size.y, size.y != size.x': [1, 0],
             'cone: size.y != size.x, between the two': [1, 0],
             'cone: t < 0 (closest approach at the origin)': [1, 0],
             'cone: scale1 < eps at the near root': [1, 0],
             'cone: scale2 > eps at the near root': [1, 0],
             'cone: scale1 < eps at the far root': [1, 0],
             'cone: scale2 > eps at the far root': [1, 0],
             'cone: from inside': [1, 0],
             'cone: p0 == p1 (n1 = 0)': [1, 0],
             'cone: n1 is not normalize(p1 - p0)': [1, 0],
             'cone: dot(dir, O) == 0': [1, 0],
             'plane XY front: |I.x - p0.x| < size.x': [2, 0],
             'plane XY front: |I.y - p0.y| < size.y': [2, 0],
             'plane XY front: a corner': [1, 0],
             'plane XY front: o.W against p0.W': [1, 0],
             'plane XY rear: |I.x - p0.x| < size.x': [2, 0],
             'plane XY rear: |I.y - p0.y| < size.y': [2, 0],
             'plane XY rear: a corner': [1, 0],
             'plane XY rear: o.W against p0.W': [1, 0],
             'plane XY: d.W through 0': [1, 0],
             'plane YZ front: |I.y - p0.y| < size.y': [2, 0],
             'plane YZ front: |I.z - p0.z| < size.z': [2, 0],
             'plane YZ front: a corner': [1, 0],
             'plane YZ front: o.W against p0.W': [1, 0],
             'plane YZ rear: |I.y - p0.y| < size.y': [2, 0],
             'plane YZ rear: |I.z - p0.z| < size.z': [2, 0],
             'plane YZ rear: a corner': [1, 0],
             'plane YZ rear: o.W against p0.W': [1, 0],
             'plane YZ: d.W through 0': [1, 0],
             'plane XZ front: |I.x - p0.x| < size.x': [2, 0],
             'plane XZ front: |I.z - p0.z| < size.z': [2, 0],
             'plane XZ front: a corner': [1, 0],
             'plane XZ front: o.W against p0.W': [1, 0],
             'plane XZ rear: |I.x - p0.x| < size.x': [2, 0],
             'plane XZ rear: |I.z - p0.z| < size.z': [2, 0],
             'plane XZ rear: a corner': [1, 0],
             'plane XZ rear: o.W against p0.W': [1, 0],
             'plane XZ: d.W through 0': [1, 0],
             'plane checkerboard front: |I.x - p0.x| < size.x': [2, 0],
             'plane checkerboard front: |I.z - p0.z| < size.z': [2, 0],
             'plane checkerboard front: a corner': [1, 0],
             'plane checkerboard front: o.W against p0.W': [1, 0],
             'plane checkerboard rear: |I.x - p0.x| < size.x': [2, 0],
             'plane checkerboard rear: |I.z - p0.z| < size.z': [2, 0],
             'plane checkerboard rear: a corner': [1, 0],
             'plane checkerboard rear: o.W against p0.W': [1, 0],
             'plane checkerboard: d.W through 0': [1, 0],
             'plane carpet front: |I.x - p0.x| < size.x': [2, 0],
             'plane carpet front: |I.z - p0.z| < size.z': [2, 0],
             'plane carpet front: a corner': [1, 0],
             'plane carpet front: o.W against p0.W': [1, 0],
             'plane carpet rear: |I.x - p0.x| < size.x': [2, 0],
             'plane carpet rear: |I.z - p0.z| < size.z': [2, 0],
             'plane carpet rear: a corner': [1, 0],
             'plane carpet rear: o.W against p0.W': [1, 0],
             'plane carpet: d.W through 0': [1, 0],
             'plane: averageColor >= transparentColor': [2, 0],
             'plane YZ emissive: (int)|I.y| % 4000 < 2000': [3, 0],
             'plane YZ emissive: (int)|I.z| % 4000 < 2000': [3, 0],
             'plane YZ emissive: small': [1, 0],
             'plane XY: wireframe width 0': [1, 0],
             'plane XY: wireframe width 0, the other axis': [1, 0],
             'plane YZ: wireframe width 0': [1, 0],
             'plane YZ: wireframe width 0, the other axis': [1, 0],
             'plane XZ: wireframe width 0': [1, 0],
             'plane XZ: wireframe width 0, the other axis': [1, 0],
             'plane XY: wireframe width 1': [1, 0],
             'plane XY: wireframe width 1, the other axis': [1, 0],
             'plane YZ: wireframe width 1': [1, 0],
             'plane YZ: wireframe width 1, the other axis': [1, 0],
             'plane XZ: wireframe width 1': [1, 0],
             'plane XZ: wireframe width 1, the other axis': [1, 0],
             'plane XY: wireframe width 255': [1, 0],
             'plane XY: wireframe width 255, the other axis': [1, 0],
             'plane YZ: wireframe width 255': [1, 0],
             'plane YZ: wireframe width 255, the other axis': [1, 0],
             'plane XZ: wireframe width 255': [1, 0],
             'plane XZ: wireframe width 255, the other axis': [1, 0],
             'triangle: a < 0': [1, 0],
             'triangle: a > 1 (the vertex p1)': [1, 0],
             'triangle: b < 0': [1, 0],
             'triangle: b > 1 (the vertex p2)': [1, 0],
             'triangle: the vertex p0': [1, 0],
             'triangle: a + b > 1': [1, 0],
             'triangle: a + b > 1, from below': [1, 0],
             'triangle: |det| < eps, det > 0': [1, 0],
             'triangle: |det| < eps, det < 0': [1, 0],
             'triangle: t < 0 at +0': [1, 0],
             'triangle: t < 0 at -0': [1, 0],
             'triangle: r > 0 (the flip of the normal)': [1, 0],
             'triangle: vertex normals whose weighted sum is 0': [1, 0],
             'triangle: three collinear points': [1, 0],
             'triangle: two equal points': [1, 0],
             'triangle: transparent': [1, 0],
             'triangle: along the hypotenuse': [1, 0],
             'triangle: along the hypotenuse, slanted': [1, 0],
             'triangle: along the edge p1 - p2, in general position': [1, 0]},
 'flat': {'triangle: a < 0': [1, 1],
          'triangle: a > 1 (the vertex p1)': [1, 1],
          'triangle: b < 0': [1, 1],
          'triangle: b > 1 (the vertex p2)': [1, 1],
          'triangle: the vertex p0': [1, 0],
          'triangle: a + b > 1': [1, 1],
          'triangle: a + b > 1, from below': [1, 1],
          'triangle: |det| < eps, det > 0': [1, 1],
          'triangle: |det| < eps, det < 0': [1, 1],
          'triangle: t < 0 at +0': [1, 1],
          'triangle: t < 0 at -0': [1, 1],
          'triangle: r > 0 (the flip of the normal)': [1, 1],
          'triangle: vertex normals whose weighted sum is 0': [1, 0],
          'triangle: three collinear points': [1, 0],
          'triangle: two equal points': [1, 0],
          'triangle: transparent': [1, 0],
          'triangle: along the hypotenuse': [1, 0],
          'triangle: along the hypotenuse, slanted': [1, 0],
          'triangle: along the edge p1 - p2, in general position': [1, 0],
          'flat: a sphere record tested as a triangle': [1, 1],
          'flat: a plane record tested as a triangle': [1, 1]},
 'camera': {'camera front: |I.x - p0.x| < size.x': [2, 2],
            'camera front: |I.y - p0.y| < size.y': [2, 2],
            'camera front: o.W against p0.W': [1, 1],
            'camera rear: |I.x - p0.x| < size.x': [2, 2],
            'camera rear: |I.y - p0.y| < size.y': [2, 2],
            'camera rear: o.W against p0.W': [1, 1],
            'camera: the colour key': [1, 1]}}

# oracle.probes.input_digest of every case
DIGESTS = {'element dyadic': '2dd1317966415dd03a85049d78a9361c68652fd5',
 'element decimal': 'c433afef12326cacc0e88b09f5aab9cf3ed43d3a',
 'element flat': '9f5b9d82d38b20e6fa41937e8cbefb995eb1b330',
 'element camera': '7f4e1753ef427737030159d7f8b3ff2fe7192b05',
 'closest dyadic kinds': '4746884e79158e637ecb76b3d1bd23ee29ad4a55',
 'shadow dyadic kinds': 'e693bfbe0128738101abb00a861312377229e72c',
 'closest dyadic general': '489c8cb8a3515bd48c8f01d97b3956a066a7d234',
 'shadow dyadic general': '28e2e9aeb656c7278583e9edeb6358fced16a7f8',
 'closest decimal kinds': 'fbbd3962783745c10afb767da421873d7a194771',
 'shadow decimal kinds': '545b8741d002b83b6fcdf81d750474c42a8ac8cb',
 'closest decimal general': 'e3c660a8da45028502494c1873612f6da88d7187',
 'shadow decimal general': '0ac71b0710a1434b727af73738073b73808193ac',
 'closest flat kinds': '7f9fa3fc820b958695a4f9a366ed64ac2b360938',
 'shadow flat kinds': 'f5e7f53d1f430e5ca95186eee4f86c31b451a4ed'}


def test_the_decisions_are_pinned(solr):
    for group in GROUP_NAMES:
        table = G.count_by_decision(G.families(solr, group))
        assert table == DECISIONS[group], {k: v for k, v in table.items() if DECISIONS[group].get(k) != v}


def digests(solr):
    from oracle import probes
    out = {}
    for group in GROUP_NAMES:
        out["element " + group] = probes.input_digest(G.element_case(solr, group)[0])
    for group, part in G.WALKS:
        sc, rays = G.lattice(solr, group, part, THIN[group])
        for kind in ("closest", "shadow"):
            out["%s %s %s" % (kind, group, part)] = probes.input_digest(G.walk_case(kind, sc, rays))
    return out


def test_the_generator_is_deterministic(solr):
    G._ELEMENT.clear()
    G._WALK.clear()
    assert digests(solr) == DIGESTS


def test_the_sizes(solr):
    total = sum(len(G.element_case(solr, group)[0]["origins"]) for group in GROUP_NAMES)
    print("elements:", {group: len(G.element_case(solr, group)[0]["origins"]) for group in GROUP_NAMES})
    assert total <= 20000
