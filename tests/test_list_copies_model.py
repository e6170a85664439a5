"""(CPU) The model of the derived node-list copies (tests/list_copies_model.py) held to what those copies are FOR, on the
hand-made lists the engine's copies are compared on (tests/test_list_copies_gpu.py): a thin box never reaches outside the
box it was cut from, a plain leaf's thin box holds each of its rectangles as far as that box does, an inner node holds the
leaves below it, the sorted copy is a permutation of the rows.  And the theorem rt_device.h's tightRay states - a ray with
no zero direction component, |direction| >= 2 and its origin within viewDistance that crosses a plain rectangle passes the
binary32 slab test of the thin box at its crossing parameter wherever it passes that of the leaf's own box - by brute
force: a few thousand such rays against every plain rectangle of the list, the crossing worked out in binary64 and kept at
least two margins inside the rectangle's edge."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import list_copies_model as M  # noqa: E402

f4 = np.float32
PLANES = (M.KIND_PLANE_XY, M.KIND_PLANE_YZ, M.KIND_PLANE_XZ)


@pytest.fixture(scope="module")
def solr():
    return importlib.import_module("sol-r_amd")


def _lists(solr):
    yield "panels", M.panels(solr)
    yield "panels, odd bounds", M.panels(solr, odd=True)
    yield "panels, 257 nodes", M.panels(solr, nodes=257, odd=True)
    yield "foreign", M.foreign(solr)


def _copies(solr, scene):
    materials = M.hand_made_materials(solr.MATERIAL_DTYPE)
    kinds = M.plain_kinds(scene.prims, materials)
    records = M.records_of(scene.prims, kinds)
    rows, start = M.rows_of(scene.boxes), scene.boxes["startIndex"]
    margin = M.margin_of(M.extent(scene.prims))
    return rows, start, records, kinds, margin, M.thin_copy(rows, start, records, kinds, margin)


def _inside(lo_a, hi_a, lo_b, hi_b):
    """[lo_a, hi_a] inside [lo_b, hi_b] on every axis (a bound of b that is no number bounds nothing)"""
    with np.errstate(invalid="ignore"):
        return bool((~(lo_a < lo_b)).all() and (~(hi_a > hi_b)).all())


def test_the_plain_rule_and_the_extent(solr):
    scene = M.panels(solr, odd=True)
    kinds = M.plain_kinds(scene.prims, M.hand_made_materials(solr.MATERIAL_DTYPE))
    first = {name: int(scene.boxes["startIndex"][i]) for name, i in scene.names.items()}
    assert kinds[first["textured"]] == 0 and kinds[first["wireframe"]] == 0 and kinds[first["emissive_yz"]] == 0
    assert kinds[first["emissive_xy"]] == M.KIND_PLANE_XY            # (only a YZ plane's emission matters)
    assert kinds[first["plane_sphere"]] == M.KIND_PLANE_XY and kinds[first["plane_sphere"] + 1] == 0
    assert kinds[first["infinite_size"]] == M.KIND_PLANE_XY and kinds[first["nan_alone"]] == M.KIND_PLANE_XZ
    assert kinds[scene.lamp] == 0
    # an infinite size and a NaN coordinate do not make the extent infinite or no number
    honest = M.panels(solr)
    assert np.isfinite(M.extent(scene.prims)) and 1.0 <= M.extent(honest.prims) <= 2.0 * 8300.0
    lone = np.zeros(1, solr.PRIMITIVE_DTYPE)
    assert M.extent(lone) == 1.0 and M.margin_of(M.extent(lone)) == f4(2.0 ** -10)


def test_thin_boxes_stay_inside_their_boxes_and_hold_their_rectangles(solr):
    for label, scene in _lists(solr):
        rows, start, records, kinds, margin, thin = _copies(solr, scene)
        assert np.array_equal(thin[:, 1, 2:].view(np.int32), rows[:, 1, 2:].view(np.int32)), label   # counts, skips
        thinner = 0
        for i in range(len(rows)):
            assert _inside(M.lo(thin)[i], M.hi(thin)[i], M.lo(rows)[i], M.hi(rows)[i]), (label, i)
            nb = int(M.counts(rows)[i])
            mine = range(int(start[i]), int(start[i]) + nb)
            if nb <= 0 or not all(kinds[k] in PLANES for k in mine):
                if nb > 0:
                    assert np.array_equal(thin[i].view(np.int32), rows[i].view(np.int32)), (label, i)
                continue
            thinner += not np.array_equal(thin[i].view(np.int32), rows[i].view(np.int32))
            for k in mine:
                rl, rh = M.rectangle_box(records[k, 0, :3], records[k, 1, :3], kinds[k], f4(0.0))
                rl, rh = np.array(rl), np.array(rh)
                with np.errstate(invalid="ignore"):
                    if not (np.isfinite(rl).all() and np.isfinite(rh).all()):
                        continue
                    # the rectangle cut with the leaf's box (where they meet at all) lies inside the thin box
                    cl, ch = np.maximum(rl, M.lo(rows)[i]), np.minimum(rh, M.hi(rows)[i])
                    if (cl <= ch).all():
                        assert _inside(cl, ch, M.lo(thin)[i], M.hi(thin)[i]), (label, i, k)
        assert thinner >= 20, (label, thinner)


def test_inner_nodes_stay_inside_their_boxes_and_hold_their_leaves(solr):
    for label, scene in _lists(solr):
        rows, start, records, kinds, margin, thin = _copies(solr, scene)
        cnt, skip = M.counts(rows), M.skips(rows)
        shrunk = 0
        for i in np.flatnonzero(cnt <= 0):
            assert _inside(M.lo(thin)[i], M.hi(thin)[i], M.lo(rows)[i], M.hi(rows)[i]), (label, i)
            leaves = [j for j in range(i + 1, i + int(skip[i])) if cnt[j] > 0]
            if not leaves:
                assert np.array_equal(thin[i].view(np.int32), rows[i].view(np.int32)), (label, i)
                continue
            shrunk += not np.array_equal(thin[i].view(np.int32), rows[i].view(np.int32))
            for j in leaves:
                # ... as far as its own box held them (the union is cut with it)
                with np.errstate(invalid="ignore"):
                    cl, ch = np.maximum(M.lo(thin)[j], M.lo(rows)[i]), np.minimum(M.hi(thin)[j], M.hi(rows)[i])
                    if (cl <= ch).all():
                        assert _inside(cl, ch, M.lo(thin)[i], M.hi(thin)[i]), (label, i, j)
        assert shrunk >= 3, (label, shrunk)


def test_several_lists_one_behind_the_other_keep_to_themselves(solr):
    scene = M.panels(solr)
    rows, start, records, kinds, margin, thin = _copies(solr, scene)
    n = len(rows)
    twice = M.thin_copy(np.concatenate([rows, rows]), np.concatenate([start, start]), records, kinds, margin, list_length=n)
    assert np.array_equal(twice[:n].view(np.int32), thin.view(np.int32))
    assert np.array_equal(twice[n:].view(np.int32), thin.view(np.int32))
    # a skip that reaches past the end of its list (the last node's does not here: made to) is clamped to it
    longer = rows.copy()
    longer[0, 1, 3] = np.int32(n + 5).view(f4)
    clamped = M.thin_copy(np.concatenate([longer, rows]), np.concatenate([start, start]), records, kinds, margin, list_length=n)
    assert np.array_equal(clamped[0, 0].view(np.int32), thin[0, 0].view(np.int32))


def test_the_sorted_copy_unsorts_to_the_rows_and_ends_in_a_zero_record(solr):
    rng = np.random.default_rng(9)
    for nb in (1, 31, 32, 33):
        rows = rng.uniform(-9000, 9000, (8 * nb, 2, 4)).astype(f4)
        rows[:, 1, 2] = rng.integers(0, 4, 8 * nb).astype(np.int32).view(f4)
        rows[:, 1, 3] = rng.integers(1, nb + 1, 8 * nb).astype(np.int32).view(f4)
        s = M.sorted_copy(rows, nb)
        assert s.shape == (8 * nb + 1, 2, 4) and not s[-1].view(np.int32).any()
        assert np.array_equal(M.unsorted(s, nb).view(np.int32), rows.view(np.int32))
        assert np.array_equal(M.skips(s[:-1]), 32 * M.skips(rows))
        assert np.array_equal(s[:nb, :, :3].view(np.int32), rows[:nb, :, :3].view(np.int32))         # octant 0: as they are
        last = slice(7 * nb, 8 * nb)                                                                # octant 7: all three
        assert np.array_equal(s[last, 0, 0], rows[last, 1, 0]) and np.array_equal(s[last, 1, 1], rows[last, 0, 1])
        assert np.array_equal(s[last, 0, 2], rows[last, 0, 3]) and np.array_equal(s[last, 0, 3], rows[last, 0, 2])
        z_only = slice(4 * nb, 5 * nb)                                                              # octant 4: z alone
        assert np.array_equal(s[z_only, 0, :2], rows[z_only, 0, :2]) and np.array_equal(s[z_only, 0, 2], rows[z_only, 0, 3])


def test_leaf_records_carry_the_first_primitive(solr):
    scene = M.panels(solr, odd=True)
    rows, start, records, kinds, margin, thin = _copies(solr, scene)
    leaf = M.leaf_records(rows, start, records)
    cnt = M.counts(rows)
    assert not leaf[cnt <= 0].view(np.int32).any()
    for i in np.flatnonzero(cnt > 0):
        first = int(start[i])
        assert np.array_equal(leaf[i, :2].view(np.int32), records[first, :2].view(np.int32))
        assert leaf[i, 3, 3].view(np.int32) == first and leaf[i, 2, 3].view(np.int32) == scene.prims["index"][first]
        plane = scene.prims["type"][first] in (M.ptXYPlane, M.ptYZPlane, M.ptXZPlane)
        assert np.array_equal(leaf[i, 2, :3], scene.prims["n0" if plane else "p1"][first])


def _slab_admits(lo, hi, o, d, t):
    """the slab test in binary32, reciprocal direction as the walks take it: does [entry, exit] of the box contain t?"""
    inv = f4(1.0) / d
    a, b = (lo - o) * inv, (hi - o) * inv
    near, far = np.minimum(a, b).max(axis=-1), np.maximum(a, b).min(axis=-1)
    return (near <= t) & (t <= far) & (near <= far)


def test_a_tight_ray_that_crosses_a_rectangle_enters_its_thin_box(solr):
    scene = M.panels(solr)
    rows, start, records, kinds, margin, thin = _copies(solr, scene)
    view_distance = 50000.0
    assert view_distance <= 64.0 * float(M.extent(scene.prims))           # what the host demands before it offers the copy
    rng = np.random.default_rng(21)
    m, tested = float(margin), 0
    for i in np.flatnonzero(M.counts(rows) > 0):
        mine = range(int(start[i]), int(start[i]) + int(M.counts(rows)[i]))
        if not all(kinds[k] in PLANES for k in mine):
            continue
        for k in mine:
            across = {M.KIND_PLANE_XY: 2, M.KIND_PLANE_YZ: 0, M.KIND_PLANE_XZ: 1}[int(kinds[k])]
            p0, size = records[k, 0, :3].astype(np.float64), np.abs(records[k, 1, :3].astype(np.float64))
            inner = size - 2.0 * m
            inner[across] = 0.0
            if (np.delete(inner, across) <= 0).any():
                continue
            n = 160
            point = p0 + rng.uniform(-1, 1, (n, 3)) * inner            # on the rectangle, two margins inside its edge
            o = rng.uniform(-view_distance, view_distance, (n, 3))
            o[: n // 4] = point[: n // 4] + rng.normal(size=(n // 4, 3)) * 40.0      # near the plane as well
            o[n // 4: n // 2, rng.integers(0, 3)] = view_distance * rng.choice([-1.0, 1.0])
            o = o.astype(f4)
            t_star = rng.uniform(0.02, 1.5, (n, 1))
            d = ((point - o) / t_star).astype(f4)                       # (the ray as binary32 numbers; the crossing again:)
            keep = (d != 0).all(axis=1) & ((d.astype(np.float64) ** 2).sum(axis=1) >= 4.0) & (np.abs(o) <= view_distance).all(axis=1)
            o, d = o[keep], d[keep]
            t = (p0[across] - o[:, across].astype(np.float64)) / d[:, across].astype(np.float64)
            cross = o.astype(np.float64) + t[:, None] * d.astype(np.float64)
            ok = (t > 0) & (np.abs(np.delete(cross - p0, across, axis=1)) <= np.delete(inner, across)).all(axis=1)
            o, d, t = o[ok], d[ok], t[ok].astype(f4)
            with np.errstate(over="ignore"):
                # (the thin box is cut with the leaf's own: it lets in what that one lets in - a box the builder made flat
                # across its plane, size 0 there, decides by rounding on its own)
                by_the_box = _slab_admits(M.lo(rows)[i], M.hi(rows)[i], o, d, t)
                flat = M.hi(rows)[i][across] - M.lo(rows)[i][across] < 2.0 * m
                assert flat or by_the_box.all(), (i, k)
                o, d, t = o[by_the_box], d[by_the_box], t[by_the_box]
                tested += len(t)
                admitted = _slab_admits(M.lo(thin)[i], M.hi(thin)[i], o, d, t)
            assert admitted.all(), (i, k, int((~admitted).sum()), len(t))
    assert tested >= 3000, tested
