/*
 * list_builders.cpp - the host builders of the engine's node lists (list_builders.h): the walk-order list (chains
 * collapsed, siblings grouped, inner nodes that hardly cull pruned), the eight order-free lists, the enclosure check
 * and the refit plan of rotated scenes.  Plain C++17; built into the engine library with the engine's numeric flags
 * (no contraction, no fast-math: the double-precision cost arithmetic decides which nodes exist).
 */
#include "list_builders.h"

#include <algorithm>
#include <cmath>

namespace solreng
{
/* skip pointers must describe nested intervals for the ballot-only walk */
int validateNesting(const BoundingBox *boxes, int n)
{
    std::vector<int> ends;
    for (int i = 0; i < n; ++i)
    {
        const int skip = boxes[i].indexForNextBox.x;
        if (skip < 1 || (long)i + skip > n)
            return 0;
        while (!ends.empty() && ends.back() <= i)
            ends.pop_back();
        const int end = i + skip;
        if (!ends.empty() && end > ends.back())
            return 0;
        ends.push_back(end);
    }
    return 1;
}

/* Collapsed walk order.  The reference's grid builder wraps most leaves in
 * a chain of inner nodes with bit-identical bounds (one per tree level,
 * GPUKernel.cpp:1008-1035).  A ray that enters the first node of such a
 * chain enters all of them - same slabs, same ray, same minDistance since
 * no primitive is tested in between - and a ray that misses it skips all
 * of them, so dropping every inner node whose only child has the same
 * bounds changes no result.  Skip pointers are recomputed in the compacted
 * numbering and stay nested.  `rows` / `start`: the reference's list as uploaded (`nested`: validateNesting's word
 * on it; a list that is not nested is copied).  *orderedExact / *orderedWalk: every bound of that list is ordered and
 * finite.  Returns the new node count. */
int collapseChains(const std::vector<float4> &rows, const std::vector<int> &start, bool nested, std::vector<float4> &outRows,
                   std::vector<int> &outStart, std::vector<int> &outOrigin, int *orderedExact, int *orderedWalk)
{
    const int n = (int)start.size();
    auto countOf = [&](int i) { return bitsi(rows[2 * i + 1].z); };
    auto skipOf = [&](int i) { return bitsi(rows[2 * i + 1].w); };
    /* (one pass: which nodes stay, whether every bound is ordered and finite, the compacted numbering) */
    std::vector<char> keep(n, 1);
    std::vector<int> newIndex((size_t)n + 1);
    newIndex[0] = 0;
    *orderedExact = 1;
    *orderedWalk = 1;
    for (int i = 0; i < n; ++i)
    {
        if (nested && countOf(i) == 0)
        {
            if (i + 1 < n)
            {
                /* (the six bounds bit for bit: the first row and half of the second) */
                if (skipOf(i) >= 2 && skipOf(i + 1) == skipOf(i) - 1 && memcmp(&rows[2 * i], &rows[2 * i + 2], 16) == 0 &&
                    memcmp(&rows[2 * i + 1], &rows[2 * i + 3], 8) == 0)
                    keep[i] = 0;
            }
            /* an inner node without emitted children (its cell held only lights or nothing,
             * GPUKernel.cpp:1096) leads nowhere: entering or missing it changes nothing */
            if (skipOf(i) == 1)
                keep[i] = 0;
        }
        const float lo[3] = {rows[2 * i].x, rows[2 * i].y, rows[2 * i].z}, hi[3] = {rows[2 * i + 1].x, rows[2 * i + 1].y, rows[2 * i].w};
        bool ordered = true;
        for (int k = 0; k < 3; ++k)
            ordered = ordered && (lo[k] <= hi[k]) && (fabsf(lo[k]) < 1.0e30f) && (fabsf(hi[k]) < 1.0e30f);
        if (!ordered)
        {
            *orderedExact = 0;
            if (keep[i])
                *orderedWalk = 0;
        }
        newIndex[(size_t)i + 1] = newIndex[i] + (keep[i] ? 1 : 0);
    }
    const int nc = newIndex[n];
    outRows.assign(2 * (size_t)nc, make_float4(0.f, 0.f, 0.f, 0.f));
    outStart.assign(nc, 0);
    outOrigin.assign(nc, 0);
    for (int i = 0; i < n; ++i)
        if (keep[i])
        {
            const int j = newIndex[i];
            outOrigin[j] = i;
            const int end = std::min(i + skipOf(i), n);
            outRows[2 * j] = rows[2 * i];
            outRows[2 * j + 1] = rows[2 * i + 1];
            outRows[2 * j + 1].w = bitsf(newIndex[end] - j);
            outStart[j] = start[i];
        }
    return nc;
}

/* Inner nodes that hardly ever cull are left out of the walk list.  An inner node - one of the reference's tree
 * whose children all lie inside it, or a grouping node, which is the union of its members - passes whenever one
 * of its children would (the argument of groupSiblings below, read the other way: slab values are monotonic in
 * the bounds, the cut-off only shrinks along a walk), so testing the children without it reaches the same
 * leaves in the same order.  What the node buys is the tests of its subtree for the rays that miss it; what it
 * costs is one test for those that do not.  A ray that is in the parent enters the node
 *   - because it starts there: the rays of a frame start on the geometry (and at the camera, which is in the
 *     room it looks at), so about the share of the parent's leaves whose centre lies in the node;
 *   - otherwise with the surface-area probability area(node) / area(parent).
 * The node stays if (1 - the larger of the two) x (nodes below it) is at least `threshold` tests.  Cornell's
 * upper cells and the groups around its walls hold every leaf centre of the room: they go, the groups of small
 * spheres on the floor stay.  Works on the walk-order rows in place; returns the new node count. */
int pruneInnerNodes(std::vector<float4> &rows, std::vector<int> &start, std::vector<int> &origin, int *nbPruned, double threshold,
                    const PruneDecider &decider)
{
    const int n = (int)start.size();
    *nbPruned = 0;
    if (n < 2 || !(threshold > 0.0))
        return n;
    auto skipOf = [&](int i) { return std::max(bitsi(rows[2 * i + 1].w), 1); };
    auto countOf = [&](int i) { return bitsi(rows[2 * i + 1].z); };
    auto lo = [&](int i, int k) { return k == 0 ? rows[2 * i].x : (k == 1 ? rows[2 * i].y : rows[2 * i].z); };
    auto hi = [&](int i, int k) { return k == 0 ? rows[2 * i + 1].x : (k == 1 ? rows[2 * i + 1].y : rows[2 * i].w); };
    auto areaOf = [&](int i) {
        const double x = (double)hi(i, 0) - lo(i, 0), y = (double)hi(i, 1) - lo(i, 1), z = (double)hi(i, 2) - lo(i, 2);
        return x * y + y * z + z * x;
    };
    std::vector<char> keep(n, 1);
    /* the decisions: the caller's shortcut (the device: solr_lists.hip, one launch per depth of the list; the same
     * arithmetic, the same decisions) where there is one and it does not decline */
    const int decided = decider ? decider(rows.data(), n, threshold, keep) : -1;
    if (decided >= 0)
        *nbPruned = decided;
    else
    {
        keep.assign(n, 1);
        std::vector<int> leaves; /* node indices of the leaves, in walk order */
        std::vector<int> leavesBefore(n + 1, 0);
        for (int i = 0; i < n; ++i)
        {
            leavesBefore[i + 1] = leavesBefore[i] + (countOf(i) > 0 ? 1 : 0);
            if (countOf(i) > 0)
                leaves.push_back(i);
        }
        struct Open
        {
            int node, end;
        };
        std::vector<Open> open; /* kept ancestors of node i */
        double sceneLo[3] = {1e300, 1e300, 1e300}, sceneHi[3] = {-1e300, -1e300, -1e300};
        for (int j = 0; j < n; j += skipOf(j))
            for (int k = 0; k < 3; ++k)
            {
                sceneLo[k] = std::min(sceneLo[k], (double)lo(j, k));
                sceneHi[k] = std::max(sceneHi[k], (double)hi(j, k));
            }
        const double sceneArea = (sceneHi[0] - sceneLo[0]) * (sceneHi[1] - sceneLo[1]) + (sceneHi[1] - sceneLo[1]) * (sceneHi[2] - sceneLo[2]) +
                                 (sceneHi[2] - sceneLo[2]) * (sceneHi[0] - sceneLo[0]);
        for (int i = 0; i < n; ++i)
        {
            while (!open.empty() && open.back().end <= i)
                open.pop_back();
            const int end = std::min(i + skipOf(i), n);
            if (countOf(i) == 0 && end > i + 1)
            {
                const int parentFrom = open.empty() ? 0 : open.back().node, parentTo = open.empty() ? n : open.back().end;
                const double parentArea = open.empty() ? sceneArea : areaOf(open.back().node);
                const double bySurface = parentArea > 0.0 ? std::min(1.0, areaOf(i) / parentArea) : 1.0;
                /* share of the parent's leaves whose centre lies in the node (sampled beyond 4096 leaves) */
                const int firstLeaf = leavesBefore[parentFrom], lastLeaf = leavesBefore[parentTo];
                const int stride = std::max(1, (lastLeaf - firstLeaf) / 4096);
                int sampled = 0, inside = 0;
                for (int q = firstLeaf; q < lastLeaf; q += stride)
                {
                    const int leaf = leaves[q];
                    bool in = true;
                    for (int k = 0; k < 3 && in; ++k)
                    {
                        const double c = 0.5 * ((double)lo(leaf, k) + hi(leaf, k));
                        in = c >= lo(i, k) && c <= hi(i, k);
                    }
                    ++sampled;
                    inside += in ? 1 : 0;
                }
                const double byOrigin = sampled ? (double)inside / sampled : 1.0;
                bool encloses = true; /* every child within the node: what the argument above rests on */
                for (int j = i + 1; j < end && encloses; j += skipOf(j))
                    for (int k = 0; k < 3; ++k)
                        encloses = encloses && lo(j, k) >= lo(i, k) && hi(j, k) <= hi(i, k);
                if (encloses && (1.0 - std::max(bySurface, byOrigin)) * (end - i - 1) < threshold)
                {
                    keep[i] = 0;
                    ++*nbPruned;
                    continue;
                }
            }
            open.push_back({i, end});
        }
    }
    if (*nbPruned == 0)
        return n;
    std::vector<int> newIndex(n + 1, 0);
    for (int i = 0; i < n; ++i)
        newIndex[i + 1] = newIndex[i] + (keep[i] ? 1 : 0);
    const int m = newIndex[n];
    std::vector<float4> outRows(2 * (size_t)m);
    std::vector<int> outStart(m), outOrigin(m);
    for (int i = 0; i < n; ++i)
        if (keep[i])
        {
            const int j = newIndex[i];
            const int end = std::min(i + skipOf(i), n);
            outRows[2 * j] = rows[2 * i];
            outRows[2 * j + 1] = rows[2 * i + 1];
            outRows[2 * j + 1].w = bitsf(newIndex[end] - j);
            outStart[j] = start[i];
            outOrigin[j] = origin[i];
        }
    rows.swap(outRows);
    start.swap(outStart);
    origin.swap(outOrigin);
    return m;
}

/* Grouping nodes.  The reference's grid builder produces wide levels - 31 sibling leaves under the root of
 * the Cornell scene, 134 top-level cells for the 100k-primitive molecule - and a walk tests every sibling
 * of every node it enters.  Here runs of CONSECUTIVE siblings are wrapped in nodes of our own whose bounds
 * are the union of the siblings' bounds (up to four parts per level, split points by the surface-area
 * heuristic, recursively while a part has more than four members; members about as large as their whole
 * run are left out).  No result can change:
 *   - the depth-first order of the original nodes, hence of every primitive test, is untouched (only
 *     consecutive runs are wrapped), so ties and the shadow accumulation resolve as before;
 *   - a walk reaches an original node only through nodes whose tests it passed, and a group passes
 *     whenever one of its members does: the slab values (b - o) * inv are monotonic in b under IEEE
 *     rounding, so the union's near values are <= and its far values >= the member's on every axis, and
 *     the member's three conditions tnear <= tfar, tnear < far, tfar > 0 carry over (for the sign-selected
 *     form with an infinite reciprocal as well: a member can only pass an axis whose slab contains the
 *     origin coordinate, and then so does the union); the closest-distance cut-off a group is tested
 *     with is never smaller than the one its members will see;
 *   - groups hold no primitives and have no side effects.
 * Requires nested skip pointers and ordered finite bounds (checked by the caller).  Rewrites the node
 * rows and the first-primitive plane in place; returns the new node count. */
int groupSiblings(std::vector<float4> &rows, std::vector<int> &start, std::vector<int> &origin, const ListKnobs &knobs)
{
    const int n = (int)start.size();
    auto skipOf = [&](int i) { return bitsi(rows[2 * i + 1].w); };
    struct Bounds
    {
        float lo[3], hi[3];
    };
    auto boundsOf = [&](int i) {
        Bounds b;
        b.lo[0] = rows[2 * i].x, b.lo[1] = rows[2 * i].y, b.lo[2] = rows[2 * i].z;
        b.hi[0] = rows[2 * i + 1].x, b.hi[1] = rows[2 * i + 1].y, b.hi[2] = rows[2 * i].w;
        return b;
    };
    auto merge = [](Bounds a, const Bounds &b) {
        for (int k = 0; k < 3; ++k)
        {
            a.lo[k] = std::min(a.lo[k], b.lo[k]);
            a.hi[k] = std::max(a.hi[k], b.hi[k]);
        }
        return a;
    };
    auto area = [](const Bounds &b) {
        const double x = (double)b.hi[0] - b.lo[0], y = (double)b.hi[1] - b.lo[1], z = (double)b.hi[2] - b.lo[2];
        return x * y + y * z + z * x;
    };
    std::vector<float4> outRows;
    std::vector<int> outStart, outOrigin; /* origin: the caller's tag of each node, -1 for the nodes made here */
    outRows.reserve(rows.size() + rows.size() / 2);
    outStart.reserve(start.size() + start.size() / 2);
    outOrigin.reserve(start.size() + start.size() / 2);

    /* best split of sib[from, to) into two consecutive parts */
    std::vector<Bounds> suffix;
    auto splitPoint = [&](const std::vector<int> &sib, int from, int to) {
        const int count = to - from;
        suffix.resize((size_t)count);
        Bounds acc = boundsOf(sib[to - 1]);
        suffix[count - 1] = acc;
        for (int k = count - 2; k >= 0; --k)
        {
            acc = merge(acc, boundsOf(sib[from + k]));
            suffix[k] = acc;
        }
        Bounds left = boundsOf(sib[from]);
        double best = 1e300;
        int bestAt = from + count / 2;
        for (int k = 1; k < count; ++k)
        {
            const double cost = area(left) * k + area(suffix[k]) * (count - k);
            if (cost < best)
            {
                best = cost;
                bestAt = from + k;
            }
            left = merge(left, boundsOf(sib[from + k]));
        }
        return bestAt;
    };

    /* tuning knobs (ListKnobs; tools/group_sweep.sh); parts[] / next[] below hold at most 2^4 parts */
    const int flatMax = std::max(1, knobs.groupFlat);
    struct Emit
    {
        std::function<void(const std::vector<int> &, int, int)> siblings;
        std::function<void(int)> node;
    } emit;
    emit.node = [&](int i) {
        const size_t at = outStart.size();
        outRows.push_back(rows[2 * i]);
        outRows.push_back(rows[2 * i + 1]);
        outStart.push_back(start[i]);
        outOrigin.push_back(origin[i]);
        /* (most inner nodes have a handful of children, which siblings() would emit as they are: no list is made for
         * them - a vector per inner node was two thirds of this function's time for a 100k-primitive scene) */
        const int end = std::min(i + skipOf(i), n);
        int few = 0;
        for (int j = i + 1; j < end && few <= flatMax; j += std::max(skipOf(j), 1))
            ++few;
        if (few > flatMax)
        {
            std::vector<int> children;
            for (int j = i + 1; j < end; j += std::max(skipOf(j), 1))
                children.push_back(j);
            emit.siblings(children, 0, (int)children.size());
        }
        else
            for (int j = i + 1; j < end;)
            {
                const int next = j + std::max(skipOf(j), 1); /* (read before the node is emitted: rows are not touched, but so it stays) */
                emit.node(j);
                j = next;
            }
        outRows[2 * at + 1].w = bitsf((int)(outStart.size() - at));
    };
    /* (a list of a few dozen nodes - the Cornell room - gains 2 % from a third round of splits, lists of
     * thousands lose 7 %: profiles/r2/group_sweep.txt) */
    /* (at least one round: with none a run longer than flatMax would be wrapped in a node around itself, for ever - no
     * grouping at all is solr_hip_set_variant(5)) */
    const int levels = std::min(4, std::max(1, knobs.groupLevels >= 0 ? knobs.groupLevels : (n <= 64 ? 3 : 2)));
    emit.siblings = [&](const std::vector<int> &sib, int from, int to) {
        if (to - from <= flatMax)
        {
            for (int k = from; k < to; ++k)
                emit.node(sib[k]);
            return;
        }
        /* a member about as large as the whole run (a wall of the room, the light cell that spans the
         * view distance) would make every group around it as large as itself and never culled: such
         * members stay where they are, ungrouped, and the runs between them are grouped on their own */
        {
            Bounds u = boundsOf(sib[from]);
            for (int k = from + 1; k < to; ++k)
                u = merge(u, boundsOf(sib[k]));
            const double limit = 0.5 * area(u);
            bool dominant = false;
            for (int k = from; k < to && !dominant; ++k)
                dominant = area(boundsOf(sib[k])) > limit;
            if (dominant)
            {
                int runStart = from;
                for (int k = from; k <= to; ++k)
                    if (k == to || area(boundsOf(sib[k])) > limit)
                    {
                        if (k > runStart)
                            emit.siblings(sib, runStart, k);
                        if (k < to)
                            emit.node(sib[k]);
                        runStart = k + 1;
                    }
                return;
            }
        }
        /* `levels` rounds of binary splits without intermediate nodes: up to 2^levels parts */
        int parts[17];
        int np = 1;
        parts[0] = from;
        parts[1] = to;
        for (int level = 0; level < levels; ++level)
        {
            int next[17];
            int nn = 0;
            for (int q = 0; q < np; ++q)
            {
                next[nn++] = parts[q];
                if (parts[q + 1] - parts[q] > 2)
                    next[nn++] = splitPoint(sib, parts[q], parts[q + 1]);
            }
            next[nn] = to;
            np = nn;
            for (int q = 0; q <= np; ++q)
                parts[q] = next[q];
        }
        for (int q = 0; q < np; ++q)
        {
            const int a = parts[q], b = parts[q + 1];
            if (b - a == 1)
            {
                emit.node(sib[a]);
                continue;
            }
            Bounds u = boundsOf(sib[a]);
            for (int k = a + 1; k < b; ++k)
                u = merge(u, boundsOf(sib[k]));
            const size_t at = outStart.size();
            outRows.push_back(make_float4(u.lo[0], u.lo[1], u.lo[2], u.hi[2]));
            outRows.push_back(make_float4(u.hi[0], u.hi[1], bitsf(0), bitsf(1)));
            outStart.push_back(0);
            outOrigin.push_back(-1);
            emit.siblings(sib, a, b);
            outRows[2 * at + 1].w = bitsf((int)(outStart.size() - at));
        }
    };
    std::vector<int> top;
    for (int j = 0; j < n; j += std::max(skipOf(j), 1))
        top.push_back(j);
    emit.siblings(top, 0, (int)top.size());
    rows.swap(outRows);
    start.swap(outStart);
    origin.swap(outOrigin);
    return (int)start.size();
}

/* The walk-order list from the collapsed one, in place: cells that do not cull pruned (their children join the run
 * above), siblings grouped, groups that do not cull either pruned.  `mark`: told what has just been done (timing).
 * Returns the new node count. */
int buildWalkOrderList(std::vector<float4> &rows, std::vector<int> &start, std::vector<int> &origin, const ListKnobs &knobs,
                       const PruneDecider &decider, int *prunedBefore, int *prunedAfter, const std::function<void(const char *)> &mark)
{
    pruneInnerNodes(rows, start, origin, prunedBefore, knobs.pruneThreshold, decider);
    if (mark)
        mark("prune");
    groupSiblings(rows, start, origin, knobs);
    if (mark)
        mark("grouping");
    const int n = pruneInnerNodes(rows, start, origin, prunedAfter, knobs.pruneThreshold, decider);
    if (mark)
        mark("prune groups");
    return n;
}

/* The order-free lists: the leaves of the scene - every node with primitives, whatever the reference put above
 * it - under a binary surface-area hierarchy of our own (binned SAH over the leaf boxes' centres, sixteen bins),
 * flattened depth-first with skip pointers like the other lists, EIGHT TIMES: once per sign octant of a ray's
 * direction, the child on the near side of each split first.  Closest-hit walks whose result does not depend on
 * the order of the leaves (rt_device.h closestHitWalk: rays longer than 2, ties to the smaller flattened index)
 * walk the list of their octant instead of the reference's order - near boxes first, so that the first hits
 * shrink the cut-off and the far side of the scene is culled, which no fixed order can do for every direction.
 * Any of the eight is correct for any ray; the choice is only speed.  Inner nodes that hardly cull are left
 * out as in the other lists (decided once, on the first flattening).  Valid only when every primitive lies
 * inside its leaf's box and every inner node of the reference's list encloses its children (the caller checks
 * both).  `rows` / `start`: a nested list.  Output: 8 x count nodes, list after list.
 * `build` (build_bounds.h): with primitive records, the hierarchy is built on the box a long ray tests - a leaf of
 * nothing but axis-plane rectangles by its thin box - and a leaf that dominates its range is set apart before the
 * binned split: centres, bins, SAH areas and the prune decisions see those boxes.  What is emitted stays what it was:
 * the leaves' rows as uploaded, every inner node's row the union of its leaves' uploaded boxes.  A scene without such a
 * leaf, and a call without `build`, get the lists of the builder before build bounds, byte for byte. */
int buildFreeOrderLists(const std::vector<float4> &rows, const std::vector<int> &start, const std::vector<int> &origin,
                        std::vector<float4> &outRows, std::vector<int> &outStart, std::vector<int> &outOrigin, int *nbPruned,
                        double threshold, const PruneDecider &decider, const BuildBounds &build)
{
    struct Leaf
    {
        float lo[3], hi[3]; /* the build box (build_bounds.h) */
        int node;
        bool thin;          /* ... which is not the box as uploaded */
    };
    struct TreeNode
    {
        float lo[3], hi[3];   /* of the build boxes: what the splits and the prune decisions see */
        float ulo[3], uhi[3]; /* of the boxes as uploaded: what is emitted */
        int left, right, axis, leaf; /* leaf: node of the input list, -1 for an inner node */
        bool keep, apart;            /* apart: one child is a dominant leaf set apart; such a node is never emitted */
    };
    bool onBuildBounds = false; /* a leaf is built on another box than its own: only then is anything built differently */
    const int n = (int)start.size();
    std::vector<Leaf> leaves;
    for (int i = 0; i < n; ++i)
        if (bitsi(rows[2 * i + 1].z) > 0)
        {
            Leaf l;
            l.thin = leafBuildBounds(rows[2 * i], rows[2 * i + 1], build.prims, start[i], bitsi(rows[2 * i + 1].z), build.margin, l.lo, l.hi);
            if (l.thin)
                onBuildBounds = true;
            l.node = i;
            leaves.push_back(l);
        }
    outRows.clear();
    outStart.clear();
    outOrigin.clear();
    *nbPruned = 0;
    if (leaves.size() < 2)
        return 0;
    auto area = [](const float *lo, const float *hi) {
        const double x = (double)hi[0] - lo[0], y = (double)hi[1] - lo[1], z = (double)hi[2] - lo[2];
        return x * y + y * z + z * x;
    };
    std::vector<TreeNode> tree;
    tree.reserve(2 * leaves.size());
    struct Range
    {
        int from, to, node;
    };
    std::vector<Range> todo;
    tree.push_back(TreeNode());
    todo.push_back({0, (int)leaves.size(), 0});
    while (!todo.empty())
    {
        const Range r = todo.back();
        todo.pop_back();
        const int count = r.to - r.from;
        TreeNode t;
        t.left = t.right = -1;
        t.axis = 0;
        t.leaf = -1;
        t.keep = true;
        t.apart = false;
        if (count == 1)
        {
            for (int k = 0; k < 3; ++k)
                t.lo[k] = leaves[r.from].lo[k], t.hi[k] = leaves[r.from].hi[k];
            t.leaf = leaves[r.from].node;
            tree[r.node] = t;
            continue;
        }
        float clo[3] = {1e30f, 1e30f, 1e30f}, chi[3] = {-1e30f, -1e30f, -1e30f};
        for (int k = 0; k < 3; ++k)
            t.lo[k] = 1e30f, t.hi[k] = -1e30f;
        for (int q = r.from; q < r.to; ++q)
            for (int k = 0; k < 3; ++k)
            {
                t.lo[k] = std::min(t.lo[k], leaves[q].lo[k]);
                t.hi[k] = std::max(t.hi[k], leaves[q].hi[k]);
                const float c = 0.5f * (leaves[q].lo[k] + leaves[q].hi[k]);
                clo[k] = std::min(clo[k], c);
                chi[k] = std::max(chi[k], c);
            }
        /* zeros are +0 (std::min keeps whichever zero it met first; the device builder of solr_lists.hip, whose
         * minima are atomics, could not tell which that was) */
        for (int k = 0; k < 3; ++k)
            t.lo[k] += 0.f, t.hi[k] += 0.f;
        /* A dominant leaf set apart.  Top-down SAH does not see what peeling a wall off a room buys until all of them
         * are out, so: the leaf with the largest build box (the first of them in the range), if that is more than
         * `dominantShare` of the range's union, becomes one child of this node and the rest of the range the other -
         * on the axis along which its centre lies farthest from the union's, the near side first like every split -
         * and the node itself is never emitted: the leaf is a sibling of the subtree over the rest (groupSiblings
         * above does the same for the walk-order list). */
        if (onBuildBounds && build.dominantShare > 0.0 && count >= 3)
        {
            int largest = -1;
            double largestArea = 0.0;
            for (int q = r.from; q < r.to; ++q)
            {
                const double a = area(leaves[q].lo, leaves[q].hi);
                if (a > largestArea)
                    largestArea = a, largest = q;
            }
            if (largest >= 0 && largestArea > build.dominantShare * area(t.lo, t.hi))
            {
                const Leaf l = leaves[largest];
                float farthest = -1.f;
                bool lowSide = true;
                for (int k = 0; k < 3; ++k)
                {
                    const float cl = 0.5f * (l.lo[k] + l.hi[k]), cu = 0.5f * (t.lo[k] + t.hi[k]);
                    if (fabsf(cl - cu) > farthest)
                        farthest = fabsf(cl - cu), t.axis = k, lowSide = cl <= cu;
                }
                /* (stable: the rest keeps the order of the leaf list) */
                if (lowSide)
                    std::rotate(leaves.begin() + r.from, leaves.begin() + largest, leaves.begin() + largest + 1);
                else
                    std::rotate(leaves.begin() + largest, leaves.begin() + largest + 1, leaves.begin() + r.to);
                const int mid = lowSide ? r.from + 1 : r.to - 1;
                t.apart = true;
                t.keep = false;
                t.left = (int)tree.size();
                t.right = t.left + 1;
                tree.push_back(TreeNode());
                tree.push_back(TreeNode());
                tree[r.node] = t;
                todo.push_back({r.from, mid, t.left});
                todo.push_back({mid, r.to, t.right});
                continue;
            }
        }
        /* binned surface-area split: one pass over the leaves fills the bins of all three axes */
        const int BINS = 16;
        int bestAxis = -1, bestBin = 0;
        double bestCost = 1e300;
        {
            int counts[3][BINS];
            float blo[3][BINS][3], bhi[3][BINS][3];
            float scale[3];
            for (int axis = 0; axis < 3; ++axis)
            {
                const float extent = chi[axis] - clo[axis];
                scale[axis] = extent > 0.f ? BINS / extent : 0.f;
                for (int b = 0; b < BINS; ++b)
                {
                    counts[axis][b] = 0;
                    for (int k = 0; k < 3; ++k)
                        blo[axis][b][k] = 1e30f, bhi[axis][b][k] = -1e30f;
                }
            }
            for (int q = r.from; q < r.to; ++q)
            {
                const Leaf &l = leaves[q];
                for (int axis = 0; axis < 3; ++axis)
                {
                    if (!(scale[axis] > 0.f))
                        continue;
                    const float c = 0.5f * (l.lo[axis] + l.hi[axis]);
                    const int b = centreBin(c, clo[axis], scale[axis], BINS);
                    ++counts[axis][b];
                    float *lo3 = blo[axis][b], *hi3 = bhi[axis][b];
                    lo3[0] = std::min(lo3[0], l.lo[0]), lo3[1] = std::min(lo3[1], l.lo[1]), lo3[2] = std::min(lo3[2], l.lo[2]);
                    hi3[0] = std::max(hi3[0], l.hi[0]), hi3[1] = std::max(hi3[1], l.hi[1]), hi3[2] = std::max(hi3[2], l.hi[2]);
                }
            }
            for (int axis = 0; axis < 3; ++axis)
            {
                if (!(scale[axis] > 0.f))
                    continue;
                double rightArea[BINS];
                int rightCount[BINS];
                float rlo[3] = {1e30f, 1e30f, 1e30f}, rhi[3] = {-1e30f, -1e30f, -1e30f};
                int rc = 0;
                for (int b = BINS - 1; b > 0; --b)
                {
                    rc += counts[axis][b];
                    for (int k = 0; k < 3; ++k)
                    {
                        rlo[k] = std::min(rlo[k], blo[axis][b][k]);
                        rhi[k] = std::max(rhi[k], bhi[axis][b][k]);
                    }
                    rightCount[b] = rc;
                    rightArea[b] = rc ? area(rlo, rhi) : 0.0;
                }
                float llo[3] = {1e30f, 1e30f, 1e30f}, lhi[3] = {-1e30f, -1e30f, -1e30f};
                int lc = 0;
                for (int b = 0; b + 1 < BINS; ++b)
                {
                    lc += counts[axis][b];
                    for (int k = 0; k < 3; ++k)
                    {
                        llo[k] = std::min(llo[k], blo[axis][b][k]);
                        lhi[k] = std::max(lhi[k], bhi[axis][b][k]);
                    }
                    if (lc == 0 || rightCount[b + 1] == 0)
                        continue;
                    const double cost = area(llo, lhi) * lc + rightArea[b + 1] * rightCount[b + 1];
                    if (cost < bestCost)
                    {
                        bestCost = cost;
                        bestAxis = axis;
                        bestBin = b;
                    }
                }
            }
        }
        int mid;
        if (bestAxis < 0)
            mid = r.from + count / 2; /* all centres coincide */
        else
        {
            const float scale = BINS / (chi[bestAxis] - clo[bestAxis]);
            const float origin = clo[bestAxis];
            const int axis = bestAxis, bin = bestBin;
            /* stable: the order inside a node stays the order of the leaf list (it decides the halving by position
             * below, and the device builder partitions the same way) */
            mid = (int)(std::stable_partition(leaves.begin() + r.from, leaves.begin() + r.to,
                                       [&](const Leaf &l) {
                                           const float c = 0.5f * (l.lo[axis] + l.hi[axis]);
                                           return centreBin(c, origin, scale, BINS) <= bin;
                                       }) -
                        leaves.begin());
            if (mid == r.from || mid == r.to)
                mid = r.from + count / 2;
            t.axis = bestAxis;
        }
        t.left = (int)tree.size(); /* the low side of the split */
        t.right = t.left + 1;
        tree.push_back(TreeNode());
        tree.push_back(TreeNode());
        tree[r.node] = t;
        todo.push_back({r.from, mid, t.left});
        todo.push_back({mid, r.to, t.right});
    }

    /* what is emitted for an inner node: the union of its leaves' boxes as uploaded (children are stored behind their
     * parent in `tree`: one backward pass).  Without build bounds that is the box the node was split on. */
    for (int t = (int)tree.size() - 1; t >= 0; --t)
    {
        TreeNode &node = tree[t];
        if (!onBuildBounds)
        {
            for (int k = 0; k < 3; ++k)
                node.ulo[k] = node.lo[k], node.uhi[k] = node.hi[k];
            continue;
        }
        if (node.leaf >= 0)
        {
            node.ulo[0] = rows[2 * node.leaf].x, node.ulo[1] = rows[2 * node.leaf].y, node.ulo[2] = rows[2 * node.leaf].z;
            node.uhi[0] = rows[2 * node.leaf + 1].x, node.uhi[1] = rows[2 * node.leaf + 1].y, node.uhi[2] = rows[2 * node.leaf].w;
            continue;
        }
        for (int k = 0; k < 3; ++k)
        {
            node.ulo[k] = std::min(tree[node.left].ulo[k], tree[node.right].ulo[k]) + 0.f; /* (zeros are +0, as above) */
            node.uhi[k] = std::max(tree[node.left].uhi[k], tree[node.right].uhi[k]) + 0.f;
        }
    }

    /* one flattening: depth-first, the child on the near side of a ray of this octant first (only the prune decisions
     * read it: the nodes with their build boxes) */
    auto flatten = [&](int octant, std::vector<float4> &fr, std::vector<int> &fs, std::vector<int> *which,
                       std::vector<int> *from) {
        struct Visit
        {
            int node, slot; /* slot >= 0: close the inner node written at `slot` */
        };
        std::vector<Visit> stack;
        stack.push_back({0, -1});
        while (!stack.empty())
        {
            const Visit v = stack.back();
            stack.pop_back();
            if (v.slot >= 0)
            {
                fr[2 * v.slot + 1].w = bitsf((int)fs.size() - v.slot);
                continue;
            }
            const TreeNode &t = tree[v.node];
            if (t.leaf >= 0)
            {
                float4 first = rows[2 * t.leaf], second = rows[2 * t.leaf + 1];
                if (onBuildBounds)
                {
                    first = make_float4(t.lo[0], t.lo[1], t.lo[2], t.hi[2]);
                    second.x = t.hi[0], second.y = t.hi[1];
                }
                second.w = bitsf(1);
                fr.push_back(first);
                fr.push_back(second);
                fs.push_back(start[t.leaf]);
                if (which)
                    which->push_back(v.node);
                if (from)
                    from->push_back(origin[t.leaf]); /* the node of the reference's list this leaf is */
                continue;
            }
            if (t.keep)
            {
                const int slot = (int)fs.size();
                fr.push_back(make_float4(t.lo[0], t.lo[1], t.lo[2], t.hi[2]));
                fr.push_back(make_float4(t.hi[0], t.hi[1], bitsf(0), bitsf(1)));
                fs.push_back(0);
                if (which)
                    which->push_back(v.node);
                if (from)
                    from->push_back(-1);
                stack.push_back({0, slot});
            }
            const bool highFirst = (octant >> t.axis) & 1; /* direction negative along the split axis */
            stack.push_back({highFirst ? t.left : t.right, -1});
            stack.push_back({highFirst ? t.right : t.left, -1}); /* popped first */
        }
    };
    /* which inner nodes stay: decided on the first flattening */
    {
        std::vector<float4> fr;
        std::vector<int> fs, which;
        flatten(0, fr, fs, &which, nullptr);
        std::vector<int> survivors(which);
        pruneInnerNodes(fr, fs, survivors, nbPruned, threshold, decider);
        std::vector<char> kept(tree.size(), 0);
        for (int t : survivors)
            kept[t] = 1;
        for (size_t t = 0; t < tree.size(); ++t)
            if (tree[t].leaf < 0)
                tree[t].keep = kept[t] != 0 && !tree[t].apart;
    }
    /* the eight lists: every node's place follows from the sizes of the subtrees before it (children are stored
     * behind their parent in `tree`, so one backward pass gives the sizes); skip pointers are relative, each list
     * is self-contained */
    std::vector<int> size(tree.size(), 0);
    for (int t = (int)tree.size() - 1; t >= 0; --t)
        size[t] = tree[t].leaf >= 0 ? 1 : (tree[t].keep ? 1 : 0) + size[tree[t].left] + size[tree[t].right];
    const int count = size[0];
    outRows.assign(16 * (size_t)count, make_float4(0.f, 0.f, 0.f, 0.f));
    outStart.assign(8 * (size_t)count, 0);
    outOrigin.assign(8 * (size_t)count, -1);
    struct Place
    {
        int node, at;
    };
    std::vector<Place> stack;
    for (int octant = 0; octant < 8; ++octant)
    {
        float4 *fr = outRows.data() + 2 * (size_t)octant * count;
        int *fs = outStart.data() + (size_t)octant * count, *fo = outOrigin.data() + (size_t)octant * count;
        stack.clear();
        stack.push_back({0, 0});
        while (!stack.empty())
        {
            const Place v = stack.back();
            stack.pop_back();
            const TreeNode &t = tree[v.node];
            if (t.leaf >= 0)
            {
                fr[2 * v.at] = rows[2 * t.leaf];
                float4 second = rows[2 * t.leaf + 1];
                second.w = bitsf(1);
                fr[2 * v.at + 1] = second;
                fs[v.at] = start[t.leaf];
                fo[v.at] = origin[t.leaf]; /* the node of the reference's list this leaf is */
                continue;
            }
            int at = v.at;
            if (t.keep)
            {
                fr[2 * at] = make_float4(t.ulo[0], t.ulo[1], t.ulo[2], t.uhi[2]);
                fr[2 * at + 1] = make_float4(t.uhi[0], t.uhi[1], bitsf(0), bitsf(size[v.node]));
                ++at;
            }
            const bool highFirst = (octant >> t.axis) & 1; /* direction negative along the split axis */
            const int first = highFirst ? t.right : t.left, second = highFirst ? t.left : t.right;
            stack.push_back({second, at + size[first]});
            stack.push_back({first, at});
        }
    }
    return count;
}

/* Does a nested node list hold what it names: every inner node its direct children (hence everything below it), every
 * leaf its primitives, as the reference's builder makes it so (GPUKernel.cpp:741-830)?  The host's form of
 * k_listEncloses, the same float arithmetic; `prims`: LB_PRIM_ROWS rows per primitive, tagged or not. */
bool listEnclosesOnHost(const std::vector<float4> &rows, const std::vector<int> &start, const std::vector<float4> &prims)
{
    const int n = (int)start.size();
    if (rows.size() < 2 * (size_t)n)
        return false;
    auto skipOf = [&](int i) { return std::max(bitsi(rows[2 * i + 1].w), 1); };
    bool encloses = true;
    for (int i = 0; i < n && encloses; ++i)
    {
        const int end = std::min(i + skipOf(i), n);
        if (bitsi(rows[2 * i + 1].z) > 0 || end <= i + 1)
            continue;
        for (int j = i + 1; j < end && encloses; j += skipOf(j))
            encloses = rows[2 * j].x >= rows[2 * i].x && rows[2 * j].y >= rows[2 * i].y && rows[2 * j].z >= rows[2 * i].z &&
                       rows[2 * j + 1].x <= rows[2 * i + 1].x && rows[2 * j + 1].y <= rows[2 * i + 1].y &&
                       rows[2 * j].w <= rows[2 * i].w;
    }
    const size_t nbPrims = prims.size() / LB_PRIM_ROWS;
    for (int i = 0; i < n && encloses; ++i)
    {
        const int count = bitsi(rows[2 * i + 1].z);
        for (int k = 0; k < count && encloses; ++k)
        {
            const size_t pi = (size_t)start[i] + k;
            if (start[i] < 0 || pi >= nbPrims)
            {
                encloses = false;
                break;
            }
            const float4 *r = &prims[LB_PRIM_ROWS * pi];
            const int type = bitsi(r[LB_ROW_P0_TYPE].w) & LB_PRIM_TYPE_MASK;
            float lo[3] = {r[LB_ROW_P0_TYPE].x, r[LB_ROW_P0_TYPE].y, r[LB_ROW_P0_TYPE].z};
            float hi[3] = {lo[0], lo[1], lo[2]};
            auto add = [&](const float4 &v) {
                lo[0] = std::min(lo[0], v.x), lo[1] = std::min(lo[1], v.y), lo[2] = std::min(lo[2], v.z);
                hi[0] = std::max(hi[0], v.x), hi[1] = std::max(hi[1], v.y), hi[2] = std::max(hi[2], v.z);
            };
            float grow[3] = {r[LB_ROW_SIZE_MAT].x, r[LB_ROW_SIZE_MAT].y, r[LB_ROW_SIZE_MAT].z};
            if (type == ptTriangle)
            {
                add(r[LB_ROW_P1_INDEX]);
                add(r[LB_ROW_P2]);
                grow[0] = grow[1] = grow[2] = 0.f;
            }
            else if (type == ptCylinder)
            {
                add(r[LB_ROW_P1_INDEX]);
                grow[1] = grow[2] = grow[0];
            }
            else if (type == ptSphere)
                grow[1] = grow[2] = grow[0];
            /* the builder subtracts and adds in another order: four ulps of the coordinates' magnitude of slack, per
             * axis - relative, so that it stays far below the order-free walks' cut-off margin (2e-4 of the distance
             * + 1e-4 of the origin's coordinates, rt_device.h) whatever the scale of the scene */
            auto slack = [&](int k) { return 4.f * 1.1920929e-7f * std::max(std::max(fabsf(lo[k]), fabsf(hi[k])), fabsf(grow[k])); };
            const float ex = slack(0), ey = slack(1), ez = slack(2);
            encloses = rows[2 * i].x <= lo[0] - fabsf(grow[0]) + ex && rows[2 * i].y <= lo[1] - fabsf(grow[1]) + ey &&
                       rows[2 * i].z <= lo[2] - fabsf(grow[2]) + ez && rows[2 * i + 1].x >= hi[0] + fabsf(grow[0]) - ex &&
                       rows[2 * i + 1].y >= hi[1] + fabsf(grow[1]) - ey && rows[2 * i].w >= hi[2] + fabsf(grow[2]) - ez;
        }
    }
    return encloses;
}

/* What a rotation on the device refits and in which order (solr_rotation.hip buildRefitPlan): the nodes of each list by
 * height, children before parents.  `plan`: the entries of all three lists (sign bit: a grouping node, seeded with
 * infinities); per list [offset into plan, count] for every height.  `origin` / `freeOrigin`: per node of the walk-order
 * list and of the eight order-free lists (one behind the other: a forest) the node of the reference's list it is;
 * node 0 of that, the light cell, is never refitted. */
void planRefit(const std::vector<float4> &exact, const std::vector<float4> &walk, const std::vector<int> &origin,
               const std::vector<float4> &free, const std::vector<int> &freeOrigin, std::vector<int> &plan,
               std::vector<int> &exactLevels, std::vector<int> &walkLevels, std::vector<int> &freeLevels)
{
    plan.clear();
    exactLevels.clear();
    walkLevels.clear();
    freeLevels.clear();

    auto heights = [](const std::vector<float4> &rows, std::vector<int> &height) {
        const int n = (int)(rows.size() / 2);
        height.assign(n, 0);
        /* nested skip pointers: a node's subtree is the nodes after it up to its skip; going backwards
         * every child is finished before its parent reads it */
        std::vector<int> parent(n, -1), stack;
        for (int i = 0; i < n; ++i)
        {
            while (!stack.empty() && i >= stack.back() + std::max(bitsi(rows[2 * stack.back() + 1].w), 1))
                stack.pop_back();
            parent[i] = stack.empty() ? -1 : stack.back();
            stack.push_back(i);
        }
        int top = 0;
        for (int i = n - 1; i >= 0; --i)
        {
            if (parent[i] >= 0)
                height[parent[i]] = std::max(height[parent[i]], height[i] + 1);
            top = std::max(top, height[i]);
        }
        return n ? top + 1 : 0;
    };
    auto byHeight = [&](const std::vector<int> &height, int nbHeights, std::vector<int> &levels, auto entry) {
        std::vector<std::vector<int>> bucket((size_t)nbHeights);
        for (int i = 0; i < (int)height.size(); ++i)
        {
            const long e = entry(i);
            if (e != -1)
                bucket[(size_t)height[i]].push_back((int)e);
        }
        for (const std::vector<int> &b : bucket)
            if (!b.empty())
            {
                levels.push_back((int)plan.size());
                levels.push_back((int)b.size());
                plan.insert(plan.end(), b.begin(), b.end());
            }
    };
    std::vector<int> height;
    int nbHeights = heights(exact, height);
    byHeight(height, nbHeights, exactLevels, [](int i) { return i != 0 ? (long)i : -1L; });
    nbHeights = heights(walk, height);
    byHeight(height, nbHeights, walkLevels, [&](int j) {
        if (origin[j] == 0)
            return -1L;                                   /* the light cell */
        return origin[j] < 0 ? (long)(j | (int)0x80000000) : (long)j; /* sign bit: a grouping node */
    });
    /* the eight order-free lists, one behind the other: a forest with the same kinds of node (leaves of the
     * reference's tree, unions above them) */
    if (!free.empty())
    {
        nbHeights = heights(free, height);
        byHeight(height, nbHeights, freeLevels, [&](int j) {
            if (freeOrigin[j] == 0)
                return -1L;
            return freeOrigin[j] < 0 ? (long)(j | (int)0x80000000) : (long)j;
        });
    }
    if (plan.empty())
        plan.push_back(0);
}
} // namespace solreng
