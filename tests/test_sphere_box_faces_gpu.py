"""closestHitWalk (rt_device.h) on rays aimed at the THIN BOXES OF SPHERE LEAVES (sol-r_amd/csrc/build_bounds.h
sphereBuildExtent): a hand-made list (tests/sphere_leaves_model.py light_cell) whose lamp sits in a cell boxed
+-viewDistance and which holds one more sphere in a box of another host's, far larger than the sphere.  The rays are made
here, in the manner of tests/walk_margin_cases.py (its Scene, Block and compose are used, nothing of it is changed):

  faces   through points on the six faces of each thin box, moved along the face's normal by one ULP, half a margin, a
          margin and two margins to either side, and on it; along the face, leaning into the box or away from it
  edges   the same at the twelve edges, moved along both normals
  rim     at the sphere's rim as seen from the origin: a hair inside (1e-4, 1e-2 units), on it, a unit and a margin
          outside, and straight at the sphere - from 30 to 30 000 units away
  each as LONG rays (the thin copy: `tight`) and as SHORT ones of length 0.95 started up to a few hundred units in front
  of the point (the bounce rays: `tightShort`, whose every thin leaf is checked against the reference's own box,
  `fatCheck`), in pure waves and in waves with one stray lane that fails the wave's predicate.

Every ray, bit for bit and with no tolerance: the walk on the engine's lists against itself with sphere leaves as uploaded
(solr_hip_set_variant(18)), with no thin copies at all (8), on the reference's own node list, and against the oracle's
CUDA dialect - after asserting that the walk is offered the thin copy and that the copy's two loose leaves are the
model's boxes the rays were aimed at."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_probes as E  # noqa: E402
import list_copies_model as M  # noqa: E402
import sphere_leaves_model as S  # noqa: E402
import test_walk_margins_gpu as T  # noqa: E402
import walk_margin_cases as W  # noqa: E402

pytestmark = pytest.mark.gpu
f4, i4 = np.float32, np.int32
REFERENCE_LEAVES, UPLOADED_SPHERE_LEAVES = 8, 18
LOOSE = ((2000.0, 2000.0, 2000.0), 300.0, ([0.0] * 3, [9000.0] * 3))


def the_scene(solr):
    made = S.light_cell(solr, W.VIEW_DISTANCE, lamps=1, extra=[("loose", [(LOOSE[0], LOOSE[1])], LOOSE[2])])
    return W.Scene(solr, made, W.VIEW_DISTANCE)


def thin_boxes(sc):
    """{leaf name: (lo, hi, centre, radius)} of the two loose sphere leaves, by the model"""
    kinds = S.kinds(sc.prims, sc.materials)
    rows, start = M.rows_of(sc.boxes), sc.boxes["startIndex"].astype(i4)
    thin = S.thin_leaves(rows, start, M.records_of(sc.prims, kinds), kinds, sc.margin, S.reach_of(sc.extent, sc.si.viewDistance))
    out = {}
    for name in ("lamp", "loose"):
        leaf = sc.names[name]
        k = int(start[leaf])
        assert not np.array_equal(thin[leaf], rows[leaf])
        out[name] = (M.lo(thin)[leaf].astype(np.float64), M.hi(thin)[leaf].astype(np.float64),
                     sc.prims["p0"][k].astype(np.float64), float(sc.prims["size"][k][0]))
    return out


def _offsets(m):
    return [("ulp", -1), ("ulp", 1), 0.0, -m / 2, m / 2, -m, m, -2 * m, 2 * m]


def _moved(face, sign, off):
    """the coordinate of a face (at `face`, outward normal `sign`) moved outwards by `off`"""
    if isinstance(off, tuple):
        return float(np.nextafter(f4(face), f4(np.inf) * f4(sign * off[1])))
    return float(f4(face + sign * off))


def face_points(sc, rng, per_offset=6):
    """(points, outward normals) on the faces and edges of the two thin boxes, moved by every offset"""
    pts, normals = [], []
    for lo, hi, _, _ in thin_boxes(sc).values():
        for axis in range(3):
            for sign, face in ((-1, lo[axis]), (1, hi[axis])):
                for off in _offsets(float(sc.margin)):
                    for _ in range(per_offset):
                        p = lo + rng.uniform(0.05, 0.95, 3) * (hi - lo)
                        p[axis] = _moved(face, sign, off)
                        n = np.zeros(3)
                        n[axis] = sign
                        pts.append(p), normals.append(n)
        for a in range(3):          # edges: the two other axes at a face each
            b, c = [x for x in range(3) if x != a]
            for sb in (-1, 1):
                for sc_ in (-1, 1):
                    for off in _offsets(float(sc.margin)):
                        p = lo + rng.uniform(0.05, 0.95, 3) * (hi - lo)
                        p[b] = _moved(lo[b] if sb < 0 else hi[b], sb, off)
                        p[c] = _moved(lo[c] if sc_ < 0 else hi[c], sc_, off)
                        n = np.zeros(3)
                        n[b], n[c] = sb, sc_
                        pts.append(p), normals.append(n / np.sqrt(2.0))
    return np.array(pts), np.array(normals)


def _along(rng, normals):
    """unit directions along the face, leaning into the box or away from it by up to a tenth, no small component"""
    u = W._unit(rng, len(normals))
    u -= (u * normals).sum(axis=1, keepdims=True) * normals
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    u += normals * rng.uniform(-0.1, 0.1, (len(normals), 1))
    u += np.where(np.abs(u) < 0.02, 0.02 * rng.choice([-1.0, 1.0], u.shape), 0.0)
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def rim_points(sc, rng, per_offset=40):
    """(points, origins): points at the rim of each sphere as seen from origins 30 ... 30 000 units away"""
    pts, origins = [], []
    m = float(sc.margin)
    for _, _, centre, radius in thin_boxes(sc).values():
        for off in (-1.0e-4, -1.0e-2, 0.0, 1.0, m, None):
            for _ in range(per_offset):
                away = np.exp(rng.uniform(np.log(30.0 + radius), np.log(30000.0)))
                o = centre + W._unit(rng, 1)[0] * away
                to = centre - o
                u = rng.normal(size=3)
                u -= (u @ to) * to / (to @ to)
                u /= np.linalg.norm(u)
                pts.append(centre + u * (rng.uniform(0.0, 0.9) * radius if off is None else radius + off))
                origins.append(o)
    return np.array(pts), np.array(origins)


def blocks(sc, rng):
    pts, normals = face_points(sc, rng)
    u = _along(rng, normals)
    n = len(pts)
    back = np.exp(rng.uniform(np.log(30.0), np.log(9000.0), (n, 1)))
    o_long = np.clip(pts - u * back, -0.98 * W.VIEW_DISTANCE, 0.98 * W.VIEW_DISTANCE)
    near = np.exp(rng.uniform(np.log(0.05), np.log(400.0), (n, 1)))
    o_short = pts - u * near
    rim, o_rim = rim_points(sc, rng)
    d_rim = rim - o_rim
    d_rim /= np.linalg.norm(d_rim, axis=1, keepdims=True)
    # short rays towards the rim start up to 400 units in front of the sphere's nearest point, or inside its thin box
    gap = np.exp(rng.uniform(np.log(0.05), np.log(400.0), (len(rim), 1)))
    o_rim_short = rim - d_rim * gap
    it = lambda k: rng.choice(W.ITERATIONS, k)  # noqa: E731
    return [W.Block("faces_long", "tight", o_long, o_long + (pts - o_long) * rng.uniform(1.1, 3.0, (n, 1)), it(n)),
            W.Block("faces_short", "short_tight", o_short, o_short + u * 0.95, it(n)),
            W.Block("rim_long", "tight", o_rim, o_rim + (rim - o_rim) * rng.uniform(1.05, 2.0, (len(rim), 1)), it(len(rim))),
            W.Block("rim_short", "short_tight", o_rim_short, o_rim_short + d_rim * 0.95, it(len(rim)))]


def cases(solr, seed=53):
    sc = the_scene(solr)
    rng = np.random.default_rng(seed)
    made = blocks(sc, rng)
    strays = W._stray_pools(sc, rng)
    return sc, {"pure": W.compose("light_cell", sc, made, strays, rng),
                "one_stray": W.compose("light_cell", sc, made, strays, rng, stray=True)}


def test_rays_at_the_faces_of_a_thin_sphere_box(solr, oracle):
    hip = solr.hip_lib()
    sc, made = cases(solr)
    boxes = thin_boxes(sc)
    report = T.Report()
    with E.Resident(solr, sc.si, sc.boxes, sc.prims, sc.materials, sc.textures, sc.lights, sc.nb_lamps):
        try:
            offer = E.walk_offer(hip, sc.si)
            print("light_cell: %s" % offer)
            assert offer["tightLists"] == 1 and offer["nbBoxesFree"] > 0 and offer["nbBoxes"] <= 1024
            # the copy the walks take has the boxes the rays were aimed at
            rows, thin = E.list_copy(hip, E.WALK_LIST, E.NODE_ROWS), E.list_copy(hip, E.WALK_LIST, E.THIN_COPY)
            start = E.list_copy(hip, E.WALK_LIST, E.START_INDICES)
            for name, (lo, hi, _, _) in boxes.items():
                leaf = int(np.flatnonzero((M.counts(rows) > 0) & (start == sc.boxes["startIndex"][sc.names[name]]))[0])
                assert np.array_equal(M.lo(thin)[leaf], lo.astype(f4)) and np.array_equal(M.hi(thin)[leaf], hi.astype(f4)), name
            for composition, case in made.items():
                what = "light_cell closest %s (%d rays)" % (composition, len(case["origins"]))
                # the pure waves are what their class claims: every lane a long ray for the thin copy, or a bounce ray for it
                d = W.direction(case)
                for w, (cls, wants, lane) in enumerate(case["waves"]):
                    if wants:
                        ok = W.PREDICATES[wants](case["origins"][w * 64:w * 64 + 64], d[w * 64:w * 64 + 64], W.VIEW_DISTANCE)
                        assert ok.sum() == (64 if lane < 0 else 63), (what, w, cls)
                base = E.walk_outputs(hip, case)
                for variant in (UPLOADED_SPHERE_LEAVES, REFERENCE_LEAVES):
                    hip.solr_hip_set_variant(variant)
                    out = E.walk_outputs(hip, case)
                    hip.solr_hip_set_variant(0)
                    assert out["features"] == base["features"]
                    report.compare("%s, variant 0 against variant %d" % (what, variant), case, base, out)
                exact = E.walk_outputs(hip, case, exact=1)
                report.compare("%s, the engine's lists against the reference's list" % what, case, base, exact)
                want = T._oracle(oracle, case)
                assert not any(np.isnan(v).any() for v in want.values()), what
                report.compare("%s, the reference's list against the oracle" % what, case, exact, want)
                report.compare("%s, the engine's lists against the oracle" % what, case, base, want)
                # worth comparing: the spheres are hit and missed, in every class
                hit = want["hit"] != 0
                for name in ("lamp", "loose"):
                    index = int(sc.prims["index"][sc.boxes["startIndex"][sc.names[name]]])
                    on = hit & (want["primitive"] == index)
                    for cls in ("rim_long", "rim_short"):
                        mine = case["cls"] == cls
                        assert 20 <= on[mine].sum() < mine.sum() // 2, (what, name, cls, int(on[mine].sum()), int(mine.sum()))
                assert 0.1 < hit.mean() < 0.95, (what, hit.mean())
        finally:
            hip.solr_hip_set_variant(0)
    report.done()
