"""Every route to a primitive test (rt_device.h) on the rays of tests/primitive_edge_cases.py - aimed at the comparisons of
the tests, at equality and a float to either side - held to the oracle's CUDA dialect bit for bit, with no element left out
and no tolerance (tests/test_primitive_edge_cases.py holds that oracle to the independent reading of the text on the same
arrays: the digests are checked here again).

  per element      testPrimitive as either walk dispatches it (solr_hip_probe_primitive: sphereIntersection,
                   triangleIntersection, planeIntersection with run-time material facts, the row-by-row fetch), in the
                   instantiation the engine chooses and in the one with everything;
  through a walk   closestHitWalk and shadowWalk over the lattice: the short paths of KIND_SPHERE / KIND_PLANE_* / KIND_TRIANGLE /
                   KIND_CYLINDER records (sphereHit + sphereNormal, triangleHit + triangleNormal, planePlain), the general
                   branches of the others, the first primitive of a leaf from the leaf's packed record and the second row by
                   row; on the engine's lists and on the reference's own (exact), family by family and interleaved so that
                   a wave holds one ray that hits among 63 that miss (the ballots' early-outs), in cases of 64 k + 1 and
                   64 k + 63 rays, reached by taking the first rays again: both orders hold every ray.  The misses last for
                   few such waves, so a third case repeats them: one hit in every wave, a wave per family.  A ray must
                   give the same bits wherever it stands, in every instantiation and on either list.

Compared: the hit flag of every element; hit point, normal, areas and shadow intensity wherever both sides have a hit (what a
miss leaves in the outputs is nobody's business, tests/test_engine_probes_gpu.py); through the walks also the primitive,
the shadow and its colour.

That the route ran is read back, not assumed: the kind in every resident record's tag (scene_layout.h PrimKind) against the
rule stated there, the feature mask the probe returns, and what the walks are offered (solr_hip_probe_walk_offer).  Each
group's families lie in two lattices.  `kinds`: the records of the types the engine takes for contained in their leaves
(engine.h primitiveContained: plain, transparent and fast-transparency spheres, cylinders, axis planes, triangles) - every
type with a short path; these lattices ARE offered the order-free lists with their sorted copies, the lamp's cut-off and
(with extended geometry) the thin copies; a transparent record keeps the shadow walks in the reference's order (no
SHADOWS_OPAQUE).  `general`: cones, ellipsoids, procedural spheres, the environment, checkerboard and carpet; ONE such record
keeps the order-free lists and the lamp's cut-off from a whole scene, so these lattices are walked in the reference's
order - recorded in the test, not forced.  A transparent sphere or triangle keeps its kind: the short paths read
PRIM_TRANSPARENT from the tag (rt_device.h shadowWalk); fast transparency, emission on a YZ plane and wireframe mode 2 make
a record KIND_GENERAL.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cuda_text_model as M  # noqa: E402
import engine_probes as E  # noqa: E402
import primitive_edge_cases as G  # noqa: E402
from test_primitive_edge_cases import DIGESTS, GROUP_NAMES, THIN  # noqa: E402

pytestmark = pytest.mark.gpu
i4 = np.int32
KIND_GENERAL, KIND_SPHERE, KIND_PLANE_XY, KIND_PLANE_YZ, KIND_PLANE_XZ, KIND_TRIANGLE, KIND_CYLINDER = range(7)
SHADOWS_OPAQUE, SHADOWS_LAMP_CUTOFF = 1, 2


def _oracle(oracle, case):
    from oracle import probes
    L = oracle.lib()
    assert L.oracle_get_dialect() == 0 and not L.oracle_get_rounded_transcendentals()
    return probes._oracle_outputs(L, case)


def _differ(a, b):
    from oracle import probes
    same = probes.same_bits(np.asarray(a), np.asarray(b))
    return ~same.reshape(len(same), -1).all(axis=1)


def expected_kinds(prims, materials):
    """scene_layout.h PrimKind: the short path a record's type and its material's facts allow"""
    out = np.zeros(len(prims), i4)
    for i, p in enumerate(prims):
        m = materials[int(p["materialId"])]
        t = int(p["type"])
        if int(m["attributes"][0]) != 0:
            continue
        if t == M.ptSphere and int(m["attributes"][1]) == 0:
            out[i] = KIND_SPHERE
        elif t in (M.ptXYPlane, M.ptYZPlane, M.ptXZPlane) and int(m["textureIds"][0]) == -1 and int(m["attributes"][2]) != 2 and \
                not (t == M.ptYZPlane and float(m["innerIllumination"][0]) != 0.0):
            out[i] = {M.ptXYPlane: KIND_PLANE_XY, M.ptYZPlane: KIND_PLANE_YZ, M.ptXZPlane: KIND_PLANE_XZ}[t]
        elif t == M.ptTriangle:
            out[i] = KIND_TRIANGLE
        elif t in (M.ptCylinder, M.ptCone):
            out[i] = KIND_CYLINDER
    return out


def resident_kinds(hip):
    return (E.primitive_records(hip)[:, 0, 3].view(i4) >> 24) & 15


@pytest.mark.parametrize("group,features", [(g, f) for g in GROUP_NAMES for f in (0, E.EVERYTHING) if f or g != "camera"],
                         ids=lambda v: {0: "the-engine-s-choice", E.EVERYTHING: "everything"}.get(v, v))
def test_every_element(solr, oracle, group, features):
    """(the ptCamera records, which map a texture whatever their material, in the all-features instantiation only)"""
    from oracle import probes
    case, fams = G.element_case(solr, group)
    assert probes.input_digest(case) == DIGESTS["element " + group]
    want = _oracle(oracle, case)
    got = E.engine_outputs(solr, case, features=features)
    print("%s: %d elements, instantiation %#x (asked %#x), %d hits by the oracle" % (group, len(want["hit"]), got["features"], features,
                                                                                      int((want["hit"] != 0).sum())))
    needed = {"flat": E.F_TRI, "camera": E.F_PLANE | E.F_TEX}.get(group, E.F_SPHERE | E.F_PROC | E.F_CYL | E.F_ELL | E.F_TRI | E.F_PLANE)
    assert got["features"] & needed == needed and (features == 0 or got["features"] == features)
    bad = _differ(got["hit"], want["hit"])
    hit = (got["hit"] != 0) & (want["hit"] != 0)
    per_key = {"hit": int(bad.sum())}
    for key in ("intersection", "normal", "areas", "shadow"):
        d = _differ(got[key], want[key]) & hit
        per_key[key] = int(d.sum())
        bad |= d
    first = [(int(e), fams[case["family"][e]].decision, int(case["shadows"][e])) for e in np.flatnonzero(bad)[:12]]
    assert not bad.any(), "%d of %d elements differ %s: %s" % (int(bad.sum()), len(bad), per_key, first)
    assert (0.15 if group == "camera" else 0.2) < hit.mean() < 0.8


def _walk_differ(kind, mine, theirs):
    if kind == "closest":
        bad = _differ(mine["hit"], theirs["hit"])
        found = (mine["hit"] != 0) & (theirs["hit"] != 0)
        per_key = {"hit": int(bad.sum())}
        for key in ("primitive", "intersection", "normal", "areas"):
            d = _differ(mine[key], theirs[key]) & found
            per_key[key] = int(d.sum())
            bad |= d
        return bad, per_key
    bad, per_key = np.zeros(len(mine["result"]), bool), {}
    for key in ("result", "color"):
        d = _differ(mine[key], theirs[key])
        per_key[key] = int(d.sum())
        bad |= d
    return bad, per_key


@pytest.mark.parametrize("group,part", G.WALKS)
def test_through_the_walks(solr, oracle, group, part):
    from oracle import probes
    hip = solr.hip_lib()
    sc, rays = G.lattice(solr, group, part, THIN[group])
    failures = []
    with E.Resident(solr, sc.si, sc.boxes, sc.prims, sc.materials, sc.textures, sc.lights, sc.nb_lamps):
        # ---- the route: what the walks are offered (the first question makes the scene resident)
        for exact in (0, 1):
            offer = E.walk_offer(hip, sc.si, exact)
            print("%s %s: offered (exact %d) %s" % (group, part, exact, offer))
            if exact:
                assert offer["nbBoxesFree"] == 0 and offer["tightLists"] == 0 and not (offer["opaqueShadows"] & SHADOWS_LAMP_CUTOFF)
            elif part == "kinds":
                # the order-free lists, their sorted copies and the lamp's cut-off; a transparent record keeps the
                # shadow walks in the reference's order
                assert offer["nbBoxesFree"] > 0 and offer["sortedLists"] == 1 and offer["opaqueShadows"] & SHADOWS_LAMP_CUTOFF
                assert not (offer["opaqueShadows"] & SHADOWS_OPAQUE)
                assert offer["tightLists"] == (0 if group == "flat" else 1)
            else:
                # recorded, not forced: a scene with one record the engine does not take for contained in its leaf (a cone,
                # an ellipsoid, a procedural sphere, the environment, a checkerboard) gets no list of the engine's own
                assert offer["nbBoxesFree"] == 0 and not (offer["opaqueShadows"] & SHADOWS_LAMP_CUTOFF)
        # ... and the kind in every resident record's tag
        kinds = resident_kinds(hip)
        assert kinds.tolist() == expected_kinds(sc.prims, sc.materials).tolist()
        found = sorted(set(kinds.tolist()))
        types = {k: sorted(set(sc.prims["type"][kinds == k].tolist())) for k in found}
        print("%s %s: kinds %s (types by kind %s)" % (group, part, found, types))
        general = sc.prims[kinds == KIND_GENERAL]
        if group != "flat" and part == "kinds":
            assert found == list(range(7))
            assert {G.FAST, G.EMISSIVE, G.WIRE0, G.WIRE1, G.WIRE255} == set(general["materialId"].tolist())
            glass = sc.prims["materialId"] == G.GLASS
            assert set(kinds[glass].tolist()) == {KIND_SPHERE, KIND_TRIANGLE}          # (see the module docstring)
        elif group != "flat":
            assert {M.ptEnvironment, M.ptCheckboard, M.ptMagicCarpet, M.ptEllipsoid, M.ptSphere} <= set(general["type"].tolist())
            assert G.PROC in general["materialId"].tolist() and KIND_CYLINDER in found          # (the cones)
        # ---- the rays
        for kind in ("closest", "shadow"):
            plain = G.walk_case(kind, sc, rays)
            assert probes.input_digest(plain) == DIGESTS["%s %s %s" % (kind, group, part)]
            want_plain = _oracle(oracle, plain)
            hits = (want_plain["hit"] != 0) if kind == "closest" else (want_plain["result"] > 0)
            plain_got = {}
            order, waves = G.interleaved(hits)
            assert waves >= 2 and all(int(hits[order[w * 64: (w + 1) * 64]].sum()) == 1 for w in range(waves))
            # the misses of a lattice last for few such waves: a third case takes them again and again, a wave for every
            # family that has a hit (90 waves at most: the case stays below 6 000 rays)
            single, single_waves = G.one_hit_waves(hits, rays["family"])
            families_with_a_hit = len(set(rays["family"][hits].tolist()))
            assert single_waves >= min(90, families_with_a_hit)
            assert all(int(hits[single[w * 64: (w + 1) * 64]].sum()) == 1 for w in range(single_waves))
            cases = {"family by family, 64 k + 1": G.walk_case(kind, sc, rays, None, 1),
                     "interleaved, 64 k + 63": G.walk_case(kind, sc, rays, order, 63),
                     "one hit in every wave": G.walk_case(kind, sc, rays, single)}
            keys = ("hit", "primitive", "intersection", "normal", "areas") if kind == "closest" else ("result", "color")
            for composition, case in cases.items():
                n = len(case["origins"])
                assert n % 64 == {"1": 1, "3": 63}.get(composition[-1], 0) and n <= 6200
                # no ray is left out: the two orders of the case hold every ray of the lattice
                assert composition.startswith("one hit") or set(case["order"].tolist()) == set(range(len(hits)))
                want = _oracle(oracle, case)
                first_of = {}
                for j, r in enumerate(case["order"].tolist()):
                    first_of.setdefault(r, j)
                back = np.array([first_of[r] for r in case["order"].tolist()])
                for features in (0, E.EVERYTHING):
                    for exact in (0, 1):
                        got = E.walk_outputs(hip, case, features, exact)
                        what = "%s %s %s, %s, instantiation %#x, %s" % (group, part, kind, composition, got["features"],
                                                                      "the reference's list" if exact else "the engine's lists")
                        assert features == 0 or got["features"] == features
                        chosen = got["features"] if features == 0 else chosen
                        bad, per_key = _walk_differ(kind, got, want)
                        if bad.any():
                            first = [(int(e), rays["decisions"][case["family"][e]]) for e in np.flatnonzero(bad)[:8]]
                            failures.append("%s: %d of %d rays differ %s: %s" % (what, int(bad.sum()), n, per_key, first))
                        # a ray gives the same bits wherever it stands: in this case (repeats) and in the plain order
                        here = {k: got[k] for k in keys}
                        for other, name in (({k: got[k][back] for k in keys}, "its first place in the case"),
                                            ({k: plain_got[(features, exact)][k][case["order"]] for k in keys} if composition != list(cases)[0]
                                             else None, "the family-by-family order")):
                            if other is None:
                                continue
                            bad, per_key = _walk_differ(kind, here, other)
                            if bad.any():
                                failures.append("%s: %d rays differ from %s %s" % (what, int(bad.sum()), name, per_key))
                        if composition == list(cases)[0]:
                            plain_got[(features, exact)] = {k: got[k][: len(hits)] for k in keys}
                print("%s %s %s, %s: %d rays, %d hit, instantiation %#x / %#x" % (group, part, kind, composition, n, int(hits[case["order"]].sum()),
                                                                              chosen, E.EVERYTHING))
    assert not failures, "\n".join(failures)
