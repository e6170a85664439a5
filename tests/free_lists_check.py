"""What eight order-free lists must be, whatever hierarchy the builder chose (test infrastructure, plain numpy).

`check(rows, start, lists)` takes a nested node list as it was handed to a builder (tests/list_builder_cases.py) and what
engine_probes.free_lists returned for it, and raises AssertionError with the list and the node that shows it unless, in
each of the eight lists:
  - the skip words are in range and nested;
  - every leaf of the input appears exactly once: its row bits are the input's with skip 1, its start index the input's,
    its origin its input node;
  - every inner node has origin -1, count 0, and six bounds that are bit for bit the minimum / maximum over the boxes AS
    HANDED IN of the leaves below it, zeros made +0 (with and without build bounds: what is emitted never is a build box);
and unless the inner nodes of the eight lists are the same multiset, the leaf sequence of list 7 - o is the reverse of list
o's (every split swaps its children when all three direction bits flip), and the inner nodes that were left out plus those
that stayed are at most (leaves - 1).  Nothing here restates how a builder splits: any binary hierarchy over the leaves,
flattened near child first per octant, passes; a leaf lost from a union, a stale skip word or a -0 does not.
"""
import numpy as np

i32, f32 = np.int32, np.float32


def _range_table(values, largest):
    """sparse table over axis 0: table[k][i] = min (max) of values[i : i + 2^k]"""
    op = np.maximum if largest else np.minimum
    table = [values]
    span = 1
    while 2 * span <= len(values):
        prev = table[-1]
        table.append(op(prev[:-span], prev[span:]))
        span *= 2
    return table


def _range_query(table, lo, hi, largest):
    """min (max) of values[lo:hi] for arrays of bounds, hi > lo"""
    op = np.maximum if largest else np.minimum
    length = hi - lo
    k = np.floor(np.log2(length)).astype(np.int64)
    out = np.empty((len(lo),) + table[0].shape[1:], table[0].dtype)
    for level in np.unique(k):
        sel = np.flatnonzero(k == level)
        t = table[level]
        out[sel] = op(t[lo[sel]], t[hi[sel] - (1 << int(level))])
    return out


def _bounds(rows):
    """(n, 3) lower and upper bounds of node rows (n, 2, 4)"""
    lo = rows[:, 0, :3]
    hi = np.stack([rows[:, 1, 0], rows[:, 1, 1], rows[:, 0, 3]], axis=1)
    return lo, hi


def check_nesting(what, rows):
    words = rows.view(i32)
    n = len(rows)
    skip = words[:, 1, 3].astype(np.int64)
    at = np.arange(n, dtype=np.int64)
    bad = np.flatnonzero((skip < 1) | (at + skip > n))
    assert len(bad) == 0, "%s: node %d has skip %d in a list of %d" % (what, bad[0], skip[bad[0]], n)
    ends = at + skip
    inner = np.flatnonzero(skip > 1)
    if len(inner):
        table = _range_table(ends, True)
        below = _range_query(table, inner + 1, ends[inner], True)
        bad = inner[below > ends[inner]]
        assert len(bad) == 0, "%s: a node below node %d ends beyond it (%d)" % (what, bad[0], ends[bad[0]])


def check(rows, start, lists, name=""):
    rows, start = np.ascontiguousarray(rows, f32), np.ascontiguousarray(start, i32)
    in_words = rows.view(i32)
    in_leaves = np.flatnonzero(in_words[:, 1, 2] > 0)
    count = lists["count"]
    assert lists["rows"].shape == (8, count, 2, 4) and lists["start"].shape == (8, count) == lists["origin"].shape
    assert count >= len(in_leaves) >= 2, "%s: %d nodes for %d leaves" % (name, count, len(in_leaves))
    sequences, inner_sets = [], []
    for o in range(8):
        what = "%s list %d" % (name, o)
        out = np.ascontiguousarray(lists["rows"][o])
        words = out.view(i32)
        origin, first = lists["origin"][o], lists["start"][o]
        check_nesting(what, out)
        leaf = words[:, 1, 2] > 0
        at = np.flatnonzero(leaf)
        # the leaves
        from_node = origin[at]
        bad = at[(from_node < 0) | (from_node >= len(rows))]
        assert len(bad) == 0, "%s: leaf %d has origin %d" % (what, bad[0], origin[bad[0]])
        seen = np.bincount(from_node, minlength=len(rows))
        expect = np.zeros(len(rows), np.int64)
        expect[in_leaves] = 1
        bad = np.flatnonzero(seen != expect)
        assert len(bad) == 0, "%s: node %d of the input appears %d times as a leaf" % (what, bad[0], seen[bad[0]])
        want = in_words[from_node].copy()
        want[:, 1, 3] = 1
        bad = at[(words[at] != want).any(axis=(1, 2))]
        assert len(bad) == 0, "%s: leaf %d %s is not input node %d %s with skip 1" % (
            what, bad[0], words[bad[0]].tolist(), origin[bad[0]], in_words[origin[bad[0]]].tolist())
        bad = at[first[at] != start[from_node]]
        assert len(bad) == 0, "%s: leaf %d starts at %d, input node %d at %d" % (
            what, bad[0], first[bad[0]], origin[bad[0]], start[origin[bad[0]]])
        # the inner nodes
        inner = np.flatnonzero(~leaf)
        bad = inner[(origin[inner] != -1) | (words[inner, 1, 2] != 0)]
        assert len(bad) == 0, "%s: inner node %d has origin %d and count %d" % (what, bad[0], origin[bad[0]], words[bad[0], 1, 2])
        if len(inner):
            before = np.concatenate([[0], np.cumsum(leaf)]).astype(np.int64)     # leaves before node j
            skip = words[inner, 1, 3].astype(np.int64)
            lo_leaf, hi_leaf = before[inner], before[inner + skip]
            bad = inner[hi_leaf - lo_leaf < 1]
            assert len(bad) == 0, "%s: inner node %d has no leaf below it" % (what, bad[0])
            leaf_lo, leaf_hi = _bounds(rows[from_node])                           # the boxes as handed in, in list order
            lo = _range_query(_range_table(leaf_lo, False), lo_leaf, hi_leaf, False) + f32(0.0)
            hi = _range_query(_range_table(leaf_hi, True), lo_leaf, hi_leaf, True) + f32(0.0)
            got_lo, got_hi = _bounds(out[inner])
            wrong = (np.ascontiguousarray(got_lo).view(i32) != np.ascontiguousarray(lo).view(i32)).any(axis=1) | \
                    (np.ascontiguousarray(got_hi).view(i32) != np.ascontiguousarray(hi).view(i32)).any(axis=1)
            bad = inner[wrong]
            if len(bad):
                j = int(np.flatnonzero(wrong)[0])
                raise AssertionError("%s: inner node %d is [%r .. %r], the union of the %d leaves below it [%r .. %r]" % (
                    what, bad[0], got_lo[j].tolist(), got_hi[j].tolist(), hi_leaf[j] - lo_leaf[j], lo[j].tolist(), hi[j].tolist()))
        sequences.append(from_node.copy())
        rows_inner = words[inner].reshape(len(inner), 8)
        inner_sets.append(rows_inner[np.lexsort(rows_inner.T[::-1])] if len(inner) else rows_inner)
    for o in range(1, 8):
        assert inner_sets[o].shape == inner_sets[0].shape and np.array_equal(inner_sets[o], inner_sets[0]), \
            "%s: lists 0 and %d do not hold the same inner nodes" % (name, o)
    for o in range(4):
        a, b = sequences[o], sequences[7 - o][::-1]
        if not np.array_equal(a, b):
            q = int(np.flatnonzero(a != b)[0])
            raise AssertionError("%s: list %d visits input node %d as leaf number %d, list %d backwards node %d" % (
                name, o, a[q], q, 7 - o, b[q]))
    kept = len(inner_sets[0])
    assert lists["pruned"] >= 0 and lists["pruned"] + kept <= len(in_leaves) - 1, \
        "%s: %d inner nodes left out and %d kept over %d leaves" % (name, lists["pruned"], kept, len(in_leaves))
