"""(CPU) The thin box of a leaf of spheres: sol-r_amd/csrc/build_bounds.h leafBuildBounds - compiled into a program of its
own (tests/sphere_leaf_bounds_check.cpp, under the address and undefined-behaviour sanitizers) and called as
solr_arena.hip k_tightenLeaves calls it - against the numpy model of tests/sphere_leaves_model.py, BIT FOR BIT, on lists of
a dozen nodes: a lamp boxed +-viewDistance, a leaf of two spheres, a leaf of a sphere and a plane, radii that are negative,
zero, infinite and no number, a centre that is no number, a box smaller than its sphere, a sphere boxed p0 -+ r as the
reference's builder boxes every sphere but the lamps (the same bits as without the clause), the reach 0 of
solr_hip_set_variant(18), the decision by type that the build box takes (no clause for spheres there).  And the hand-made lists of
tests/list_copies_model.py, whose sphere leaves are all boxed p0 -+ r: their thin copies are what they were."""
import os
import subprocess

import numpy as np
import pytest

import list_copies_model as M
import sphere_leaves_model as S

HERE = os.path.dirname(os.path.abspath(__file__))
f4, i4 = np.float32, np.int32
VIEW = 50000.0
EXTENT = f4(55000.0)
MARGIN = M.margin_of(EXTENT)
REACH = S.reach_of(EXTENT, VIEW)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sphere_leaves") / "sphere_leaf_bounds_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", exe,
                    os.path.join(HERE, "sphere_leaf_bounds_check.cpp")], check=True)
    return exe


def compiled(checker, tmp_path, rows, start, records, margin, reach, by_kind=True):
    """the leaves of the thin copy and leafBuildBounds' answers, from the compiled function"""
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        np.array([len(rows), len(records), 1 if by_kind else 0], i4).tofile(f)
        np.array([margin, reach], f4).tofile(f)
        np.ascontiguousarray(rows, f4).tofile(f)
        np.ascontiguousarray(start, i4).tofile(f)
        np.ascontiguousarray(records, f4).tofile(f)
    subprocess.run([checker, src, dst], check=True)
    out = np.fromfile(dst, f4, 8 * len(rows)).reshape(len(rows), 2, 4)
    answers = np.fromfile(dst, i4, len(rows), offset=32 * len(rows))
    return out, answers


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(i4), np.ascontiguousarray(b).view(i4))


class Lists:
    """a root over leaves made one by one: add(box or None, [(type, kind, p0, size) ...]) -> the leaf's node"""

    def __init__(self):
        self.rows, self.start, self.records = [np.zeros((2, 4), f4)], [0], []

    def add(self, box, members):
        with np.errstate(all="ignore"):
            if box is None:     # the reference's builder: p0 -+ r
                p = np.array([m[2] for m in members], f4)
                r = np.array([[m[3][0]] * 3 for m in members], f4)
                box = ((p - r).min(axis=0), (p + r).max(axis=0))
        row = np.zeros((2, 4), f4)
        row[0, :3], row[0, 3], row[1, :2] = box[0], box[1][2], box[1][:2]
        row[1, 2], row[1, 3] = i4(len(members)).view(f4), i4(1).view(f4)
        self.rows.append(row)
        self.start.append(len(self.records))
        for ptype, kind, p0, size in members:
            r = np.zeros((8, 4), f4)
            r[M.ROW_P0_TYPE, :3], r[M.ROW_SIZE_MAT, :3] = p0, size
            r[M.ROW_P0_TYPE, 3] = i4(ptype | (kind << M.KIND_SHIFT)).view(f4)
            self.records.append(r)
        return len(self.rows) - 1

    def done(self):
        rows = np.array(self.rows, f4)
        rows[0, 0, :3], rows[0, 0, 3], rows[0, 1, :2] = -VIEW, VIEW, VIEW
        rows[0, 1, 3] = i4(len(rows)).view(f4)
        records = np.array(self.records, f4)
        return rows, np.array(self.start, i4), records, M.kinds_of_records(records)


def sphere(p0, radius, kind=S.KIND_SPHERE):
    return (M.ptSphere, kind, p0, (radius, 0.0, 0.0))


def plane(p0, size, ptype=M.ptXYPlane, kind=M.KIND_PLANE_XY):
    return (ptype, kind, p0, size)


WIDE = ([-VIEW] * 3, [VIEW] * 3)
LAMP = (8000.0, 8000.0, -8000.0)


def the_cases():
    L = Lists()
    n = {}
    n["lamp"] = L.add(WIDE, [sphere(LAMP, 10.0)])
    n["two"] = L.add(([-20000.0] * 3, [30000.0] * 3), [sphere((1000.0, -2000.0, 3000.0), 500.0), sphere((-4000.0, 2500.0, 100.0), 2000.0)])
    n["sphere and plane"] = L.add(WIDE, [sphere((100.0, 200.0, 300.0), 50.0), plane((0.0, 0.0, 900.0), (400.0, 300.0, 200.0))])
    n["plane and sphere"] = L.add(WIDE, [plane((0.0, 0.0, 900.0), (400.0, 300.0, 200.0)), sphere((100.0, 200.0, 300.0), 50.0)])
    n["negative radius"] = L.add(WIDE, [sphere((-7000.0, 100.0, 2000.0), -300.0)])
    n["zero radius"] = L.add(WIDE, [sphere((-7000.0, 100.0, 2000.0), 0.0)])
    n["infinite radius"] = L.add(WIDE, [sphere((-7000.0, 100.0, 2000.0), np.inf)])
    n["radius no number"] = L.add(WIDE, [sphere((-7000.0, 100.0, 2000.0), np.nan)])
    n["centre no number"] = L.add(WIDE, [sphere((-7000.0, np.nan, 2000.0), 40.0)])
    n["no number beside a sphere"] = L.add(WIDE, [sphere((500.0, 600.0, 700.0), 40.0), sphere((-7000.0, np.nan, 2000.0), 40.0)])
    n["box smaller than its sphere"] = L.add(([2950.0, -40.0, 10.0], [3020.0, 35.0, 60.0]), [sphere((3000.0, 0.0, 0.0), 100.0)])
    n["as the builder boxes it"] = L.add(None, [sphere((3000.0, -6000.0, 250.0), 600.0)])
    n["two, as the builder boxes them"] = L.add(None, [sphere((3000.0, -6000.0, 250.0), 600.0), sphere((3500.0, -6100.0, 0.0), 2000.0)])
    n["procedural"] = L.add(WIDE, [sphere((3000.0, -6000.0, 250.0), 600.0, kind=0)])
    n["plain plane"] = L.add(WIDE, [plane((0.0, 0.0, 900.0), (400.0, 300.0, 200.0))])
    return L.done(), n


def test_the_compiled_clause_is_the_model_s(checker, tmp_path):
    (rows, start, records, kinds), n = the_cases()
    got, answers = compiled(checker, tmp_path, rows, start, records, MARGIN, REACH)
    want = S.thin_leaves(rows, start, records, kinds, MARGIN, REACH)
    differing = np.flatnonzero((got.view(i4) != want.view(i4)).reshape(len(rows), -1).any(axis=1))
    assert _same(got, want), [k for k, v in n.items() if v in differing]
    changed = {k for k, v in n.items() if not _same(got[v], rows[v])}
    print("leaves whose thin box differs from their rows:", sorted(changed))
    assert changed == {"lamp", "two", "negative radius", "plain plane"}
    # a leaf of spheres that is boxed as the builder boxes it takes the clause and comes out of the cut as it went in
    for name in ("as the builder boxes it", "two, as the builder boxes them", "box smaller than its sphere"):
        assert answers[n[name]] == 1 and _same(got[n[name]], rows[n[name]]), name
    for name in ("sphere and plane", "plane and sphere", "zero radius", "infinite radius", "radius no number", "centre no number",
                 "no number beside a sphere", "procedural"):
        assert answers[n[name]] == 0, name
    # the lamp: p0 -+ ((10 + margin) + 3 far^2 2^-21 / 10 + far 2^-9), far = 55 000 + 8 000 - written out in binary64
    far = float(REACH) + 8000.0
    e = 10.0 + float(MARGIN) + 3.0 * far * far * 2.0 ** -21 / 10.0 + far * 2.0 ** -9
    box = got[n["lamp"]]
    assert np.allclose(M.lo(box[None])[0], np.array(LAMP) - e, rtol=1e-6) and np.allclose(M.hi(box[None])[0], np.array(LAMP) + e, rtol=1e-6)
    assert 700.0 < e < 800.0
    # the negative radius counts as its size
    twin = S.sphere_extent((-7000.0, 100.0, 2000.0), 300.0, MARGIN, REACH)
    assert S.sphere_extent((-7000.0, 100.0, 2000.0), -300.0, MARGIN, REACH).view(i4) == twin.view(i4)


def test_without_a_reach_sphere_leaves_keep_their_boxes(checker, tmp_path):
    """solr_hip_set_variant(18), and every caller from before the clause: the model of tests/list_copies_model.py"""
    (rows, start, records, kinds), n = the_cases()
    got, answers = compiled(checker, tmp_path, rows, start, records, MARGIN, 0.0)
    planes_only = np.where(np.isin(kinds, S.PLANES), kinds, 0)
    assert _same(got, M.thin_leaves(rows, start, records, planes_only, MARGIN))
    assert _same(got, S.thin_leaves(rows, start, records, kinds, MARGIN, 0.0))
    assert [k for k, v in n.items() if answers[v]] == ["plain plane"]


def test_by_type_there_is_no_clause_for_spheres(checker, tmp_path):
    """byKind off - the box the order-free hierarchy is built on, materials unknown: the type does not say which spheres are
    procedural, so leaves of spheres keep their boxes whatever the reach; planes go by type as before"""
    (rows, start, records, kinds), n = the_cases()
    got, answers = compiled(checker, tmp_path, rows, start, records, MARGIN, REACH, by_kind=False)
    types = records[:, M.ROW_P0_TYPE, 3].view(i4) & 0xff
    by_type = np.where(types == M.ptXYPlane, M.KIND_PLANE_XY, 0).astype(i4)
    assert _same(got, M.thin_leaves(rows, start, records, by_type, MARGIN))
    assert [k for k, v in n.items() if answers[v]] == ["plain plane"]


def test_inner_nodes_follow_the_thin_lamp(checker, tmp_path):
    """k_tightenInner's model over the leaves: the root of a list whose every leaf is thin shrinks with them"""
    L = Lists()
    L.add(WIDE, [sphere(LAMP, 10.0)])
    L.add(None, [sphere((-2000.0, 100.0, 50.0), 700.0)])
    L.add(None, [plane((0.0, 0.0, 900.0), (400.0, 300.0, 200.0))])
    rows, start, records, kinds = L.done()
    got, _ = compiled(checker, tmp_path, rows, start, records, MARGIN, REACH)
    thin = S.thin_copy(rows, start, records, kinds, MARGIN, REACH)
    assert _same(thin[1:], got[1:])
    assert (M.hi(thin)[0] < 10000.0).all() and (M.lo(thin)[0] > -10000.0).all()
    assert _same(S.thin_copy(rows, start, records, kinds, MARGIN, 0.0)[0], rows[0])


@pytest.mark.parametrize("make", ["panels", "foreign"])
def test_the_hand_made_lists_keep_their_thin_copies(solr, checker, tmp_path, make):
    """every sphere leaf of tests/list_copies_model.py's lists, the lamp's included, is boxed p0 -+ r: with the clause their
    thin copies are the same bits, and none of their sphere leaves is loose"""
    scene = getattr(M, make)(solr, glass=True)
    materials = M.hand_made_materials(solr.MATERIAL_DTYPE)
    kinds = S.kinds(scene.prims, materials)
    assert (kinds == S.KIND_SPHERE).sum() >= 8
    records = M.records_of(scene.prims, kinds)
    rows, start = M.rows_of(scene.boxes), scene.boxes["startIndex"].astype(i4)
    margin = M.margin_of(M.extent(scene.prims))
    reach = S.reach_of(M.extent(scene.prims), VIEW)
    before = M.thin_copy(rows, start, records, M.plain_kinds(scene.prims, materials), margin)
    assert _same(S.thin_copy(rows, start, records, kinds, margin, reach), before)
    got, _ = compiled(checker, tmp_path, rows, start, records, margin, reach)
    assert _same(M.thin_inner(got, len(rows)), before)
    assert S.loose_sphere_leaves(rows, start, records, kinds) == []


def test_the_light_cell_of_a_hand_made_list(solr, checker, tmp_path):
    scene = S.light_cell(solr, VIEW, lamps=2, extra=[("loose", [((2000.0, 2000.0, 2000.0), 300.0)], ([0.0] * 3, [9000.0] * 3))])
    materials = M.hand_made_materials(solr.MATERIAL_DTYPE)
    kinds = S.kinds(scene.prims, materials)
    records = M.records_of(scene.prims, kinds)
    rows, start = M.rows_of(scene.boxes), scene.boxes["startIndex"].astype(i4)
    margin, reach = M.margin_of(M.extent(scene.prims)), S.reach_of(M.extent(scene.prims), VIEW)
    assert S.loose_sphere_leaves(rows, start, records, kinds) == [scene.names["loose"], scene.names["lamp"]]
    got, answers = compiled(checker, tmp_path, rows, start, records, margin, reach)
    want = S.thin_leaves(rows, start, records, kinds, margin, reach)
    assert _same(got, want)
    without = M.thin_leaves(rows, start, records, M.plain_kinds(scene.prims, materials), margin)
    changed = np.flatnonzero((want.view(i4) != without.view(i4)).reshape(len(rows), -1).any(axis=1)).tolist()
    assert changed == [scene.names["loose"], scene.names["lamp"]]
    # both lamps lie in the cell's thin box, which is far smaller than the cell
    lamp = scene.names["lamp"]
    for p in scene.prims[scene.lamp:]:
        assert (M.lo(want)[lamp] < p["p0"] - 10).all() and (M.hi(want)[lamp] > p["p0"] + 10).all()
    assert (M.hi(want)[lamp] - M.lo(want)[lamp] < 0.2 * 2 * VIEW).all()
