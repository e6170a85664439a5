"""The host builders of the order-free lists and pruneInnerNodes (sol-r_amd/csrc/list_builders.cpp) on the synthetic node
lists of tests/list_builder_cases.py, through the probes that need no GPU (solr_hip_probe_free_lists / _prune_list, route 0).
The host builder is what the device builder is held to (tests/test_list_builders_device_gpu.py), so it is itself held, case
by case, to what eight order-free lists must be whatever the hierarchy (tests/free_lists_check.py) - and the generator to
what it promises: legal lists, leaf counts and alignments that reach the branches the families are named after."""
import numpy as np
import pytest

import engine_probes as E
import free_lists_check
import list_builder_cases as K

i32 = np.int32


@pytest.fixture(scope="module")
def hip(solr):
    lib = solr.hip_lib()
    E.declare(lib)
    lib.solr_hip_clear_error()
    return lib


@pytest.mark.parametrize("name", K.FREE_CASES)
def test_host_lists_are_lists_of_the_input(hip, name):
    rows, start, prims, margin, share, threshold = K.free_case(name)
    free_lists_check.check_nesting(name + " (input)", rows)
    lists = E.free_lists(hip, E.HOST_BUILDER, rows, start, prims, margin, share, threshold)
    if name in K.DECLINED:
        assert lists is None, "a list of fewer than two leaves was built"
        return
    assert lists is not None, "the host builder declined"
    free_lists_check.check(rows, start, lists, name)


def test_the_input_lists_are_what_the_families_promise():
    """legal lists shaped like the reference's: the lamp cell first, inner nodes that are the exact unions of their
    children, about one node in seven no leaf (wrapped) or none (flat); the leaf counts named"""
    for name in K.FREE_CASES:
        rows, start = K.free_case(name)[:2]
        words = rows.view(i32)
        assert words[0, 1, 2] == 1 and words[0, 1, 3] == 1 and rows[0, 0, 0] == -K.VIEW and rows[0, 1, 0] == K.VIEW, name
        leaf = words[:, 1, 2] > 0
        for i in np.flatnonzero(~leaf):
            below = slice(i + 1, i + words[i, 1, 3])
            assert leaf[below].all() and 1 <= leaf[below].sum() <= 7, name
            lo = np.minimum.reduce(rows[below, 0, :3]).tolist() + [np.max(rows[below, 0, 3])]
            hi = [np.max(rows[below, 1, 0]), np.max(rows[below, 1, 1])]
            assert rows[i, 0].tolist() == lo and rows[i, 1, :2].tolist() == hi, (name, i)
        if "-L" in name:
            assert leaf.sum() - 1 == int(name.split("-L")[1].split("-")[0]), name
        if name.endswith("-flat"):
            assert leaf.all(), name
        elif leaf.sum() > 60:
            assert 0.08 < (~leaf).mean() < 0.35, (name, (~leaf).mean())
    assert len(K.FREE_CASES) == len(set(K.FREE_CASES))


def test_the_tiny_extents_make_the_bin_scale_infinite():
    """what the family is for: 16 / (extent of the centres) overflows binary32 on one axis, not on the others"""
    f32 = np.float32
    for name in K.FREE_CASES:
        if not name.startswith("tiny-extent"):
            continue
        rows = K.free_case(name)[0]
        leaf = rows.view(i32)[:, 1, 2] > 0
        lo, hi = free_lists_check._bounds(rows[leaf])
        c = f32(0.5) * (lo + hi)
        with np.errstate(over="ignore", divide="ignore"):
            scale = f32(16.0) / (c.max(axis=0) - c.min(axis=0))
        assert np.isinf(scale).sum() == 1 and (c.max(axis=0) > c.min(axis=0)).all(), (name, scale)


def test_build_bounds_set_dominant_leaves_apart(hip):
    """the room's lists differ from the lists without primitive records and from those with share 0: the apart branch ran"""
    def built(name):
        rows, start, prims, margin, share, threshold = K.free_case(name)
        return E.free_lists(hip, E.HOST_BUILDER, rows, start, prims, margin, share, threshold)
    room, plain, none = built("room-10-spheres"), built("room-no-records"), built("room-share-0")
    assert not np.array_equal(room["origin"][0], plain["origin"][0]) or room["count"] != plain["count"]
    assert not np.array_equal(room["origin"][0], none["origin"][0]) or room["count"] != none["count"]


@pytest.mark.parametrize("name", K.PRUNE_CASES)
def test_host_prune_keeps_the_leaves_and_the_nesting(hip, name):
    rows, start, threshold = K.prune_case(name)
    out = E.prune_list(hip, E.HOST_BUILDER, rows, start, threshold)
    words, got = rows.view(i32), out["rows"].view(i32)
    assert out["declined"] == 0 and out["count"] == len(rows) - out["pruned"]
    if out["count"] > 0:
        free_lists_check.check_nesting(name, out["rows"])
    origin = out["origin"]
    assert (np.diff(origin) > 0).all() and (origin >= 0).all() and (origin < len(rows)).all()
    left_out = np.setdiff1d(np.arange(len(rows)), origin)
    assert (words[left_out, 1, 2] == 0).all(), "a leaf was left out"
    assert np.array_equal(got[:, 0], words[origin, 0]) and np.array_equal(got[:, 1, :3], words[origin, 1, :3])
    assert np.array_equal(out["start"], start[origin])


def test_a_child_that_sticks_out_keeps_its_parent(hip):
    for t in (1.0, 0.25, 4.0):
        within = E.prune_list(hip, E.HOST_BUILDER, *K.prune_case("child-within-threshold-%g" % t))
        out = E.prune_list(hip, E.HOST_BUILDER, *K.prune_case("child-sticks-out-threshold-%g" % t))
        assert 1 not in within["origin"] and within["pruned"] == 1, t
        assert 1 in out["origin"] and out["pruned"] == 0, t


def test_a_list_that_is_not_nested_is_an_error_not_a_decline(hip):
    rows, start = K.free_case("minimum-L3")[:2]
    rows = rows.copy()
    rows.view(i32)[1, 1, 3] = len(rows) + 5
    with pytest.raises(RuntimeError):
        E.free_lists(hip, E.HOST_BUILDER, rows, start)
    with pytest.raises(RuntimeError):
        E.prune_list(hip, E.HOST_BUILDER, rows, start)
    assert E.free_lists(hip, E.HOST_BUILDER, *K.free_case("minimum-L0")[:2]) is None      # a decline sets no error


def test_the_check_notices_lists_that_are_subtly_wrong(hip):
    """what a wrong branch of a builder yields is still a plausible hierarchy: an inner box one leaf short, a zero of the
    other sign, a stale skip word, two leaves exchanged in one list, a leaf's start index lost - each is noticed"""
    rows, start = K.free_case("zeros-of-both-signs-below")[:2]
    good = E.free_lists(hip, E.HOST_BUILDER, rows, start)
    free_lists_check.check(rows, start, good)

    def spoiled(change):
        bad = {key: (value.copy() if isinstance(value, np.ndarray) else value) for key, value in good.items()}
        change(bad)
        with pytest.raises(AssertionError):
            free_lists_check.check(rows, start, bad)

    words = good["rows"].view(i32)
    inner = np.flatnonzero(words[3, :, 1, 2] == 0)
    leaves = np.flatnonzero(words[3, :, 1, 2] > 0)
    zero = [(j, k) for j in inner for k in range(3) if words[3, j, 0, k] == 0]
    assert zero, "no inner node of this case has a lower bound of +0"

    def minus_zero(bad):
        bad["rows"].view(i32)[3, zero[0][0], 0, zero[0][1]] = -0x80000000
    spoiled(minus_zero)

    def one_leaf_short(bad):       # the upper x of an inner node pulled in to the next float below
        bad["rows"][3, inner[-1], 1, 0] = np.nextafter(bad["rows"][3, inner[-1], 1, 0], np.float32(-np.inf))
    spoiled(one_leaf_short)

    def stale_skip(bad):
        bad["rows"].view(i32)[3, inner[-1], 1, 3] += 1
    spoiled(stale_skip)

    def exchanged(bad):
        a, b = leaves[0], leaves[-1]
        for key in ("rows", "start", "origin"):
            bad[key][3, [a, b]] = bad[key][3, [b, a]]
    spoiled(exchanged)

    def start_lost(bad):
        bad["start"][5, leaves[2]] += 1
    spoiled(start_lost)

    def origin_wrong(bad):
        bad["origin"][6, leaves[1]] = bad["origin"][6, leaves[2]]
    spoiled(origin_wrong)

    def too_many_pruned(bad):
        bad["pruned"] = len(leaves)
    spoiled(too_many_pruned)
