/*
 * list_builders_check.cpp - the host builders of the node lists (sol-r_amd/csrc/list_builders.cpp) on their own: no
 * engine, no device.  tests/test_list_builders.py compiles this file with list_builders.cpp under the address and
 * undefined-behaviour sanitizers and runs it on a scene file:
 *   int32 n, int32 p | float32 rows[n][2][4] | int32 start[n] | float32 prims[p][8][4]
 * (the reference's node list and the primitive records as h2d_scene converts them).  The walk-order list, the eight
 * order-free lists and the refit plan are built with the default parameters and held to what the walks and the refit
 * kernels rely on; every violation is printed with the node that shows it, and the exit status is 1 if there was one.
 */
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <vector>

#include "../sol-r_amd/csrc/list_builders.h"

using namespace solreng;

static int failures = 0;
static void fail(const char *format, ...)
{
    if (++failures > 20)
        return;
    va_list args;
    va_start(args, format);
    fprintf(stderr, "FAILED: ");
    vfprintf(stderr, format, args);
    fprintf(stderr, "\n");
    va_end(args);
}

typedef std::vector<float4> Rows;
static int countOf(const float4 *rows, int i) { return bitsi(rows[2 * i + 1].z); }
static int skipOf(const float4 *rows, int i) { return bitsi(rows[2 * i + 1].w); }
static void bounds(const float4 *rows, int i, float lo[3], float hi[3])
{
    lo[0] = rows[2 * i].x, lo[1] = rows[2 * i].y, lo[2] = rows[2 * i].z;
    hi[0] = rows[2 * i + 1].x, hi[1] = rows[2 * i + 1].y, hi[2] = rows[2 * i].w;
}
/* everything of a node but its skip word, bit for bit */
static bool sameNode(const float4 *a, int i, const float4 *b, int j)
{
    return memcmp(&a[2 * i], &b[2 * j], 16) == 0 && memcmp(&a[2 * i + 1], &b[2 * j + 1], 12) == 0;
}

/* skip pointers in range and nested: every subtree ends where an enclosing one does, or before */
static bool nested(const char *what, const float4 *rows, int n)
{
    std::vector<int> ends;
    for (int i = 0; i < n; ++i)
    {
        const int skip = skipOf(rows, i);
        if (skip < 1 || (long)i + skip > n)
        {
            fail("%s: node %d has skip %d in a list of %d", what, i, skip, n);
            return false;
        }
        while (!ends.empty() && ends.back() <= i)
            ends.pop_back();
        if (!ends.empty() && i + skip > ends.back())
        {
            fail("%s: node %d ends at %d, beyond its parent's %d", what, i, i + skip, ends.back());
            return false;
        }
        ends.push_back(i + skip);
    }
    return true;
}

/* the levels of a refit plan for one list of n nodes: no node twice, every child before its parent */
static void checkLevels(const char *what, const float4 *rows, int n, const std::vector<int> &plan, const std::vector<int> &levels)
{
    std::vector<int> levelOf(n, -1);
    for (size_t l = 0; l + 1 < levels.size(); l += 2)
        for (int k = 0; k < levels[l + 1]; ++k)
        {
            const size_t at = (size_t)levels[l] + k;
            if (at >= plan.size())
            {
                fail("%s: level %zu reaches entry %zu of a plan of %zu", what, l / 2, at, plan.size());
                return;
            }
            const int node = plan[at] & 0x7fffffff;
            if (node >= n)
            {
                fail("%s: level %zu names node %d of %d", what, l / 2, node, n);
                return;
            }
            if (levelOf[node] >= 0)
                fail("%s: node %d is in level %d and in level %zu", what, node, levelOf[node], l / 2);
            levelOf[node] = (int)(l / 2);
        }
    for (int i = 0; i < n; ++i)
        for (int c = i + 1; levelOf[i] >= 0 && c < i + skipOf(rows, i) && c < n; c += std::max(skipOf(rows, c), 1))
            if (levelOf[c] >= levelOf[i])
                fail("%s: node %d (level %d) is refitted before its child %d (level %d)", what, i, levelOf[i], c, levelOf[c]);
}

int main(int argc, char **argv)
{
    if (argc != 2)
    {
        fprintf(stderr, "usage: %s scene-file\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    int head[2] = {0, 0};
    if (!f || fread(head, 4, 2, f) != 2 || head[0] < 1 || head[1] < 0)
    {
        fprintf(stderr, "%s: not a scene file\n", argv[1]);
        return 2;
    }
    const int n = head[0], nbPrims = head[1];
    Rows exact(2 * (size_t)n), prims((size_t)LB_PRIM_ROWS * nbPrims);
    std::vector<int> exactStart(n);
    if (fread(exact.data(), 16, exact.size(), f) != exact.size() || fread(exactStart.data(), 4, n, f) != (size_t)n ||
        fread(prims.data(), 16, prims.size(), f) != prims.size())
    {
        fprintf(stderr, "%s: truncated\n", argv[1]);
        return 2;
    }
    fclose(f);
    if (!nested("exact list", exact.data(), n))
        return 1;
    std::vector<int> exactLeaves;
    for (int i = 0; i < n; ++i)
        if (countOf(exact.data(), i) > 0)
            exactLeaves.push_back(i);

    /* ---- the walk-order list ------------------------------------------------------------------------------------------ */
    const ListKnobs knobs;
    Rows walk;
    std::vector<int> walkStart, walkOrigin;
    int orderedExact = 0, orderedWalk = 0, prunedBefore = 0, prunedAfter = 0;
    const int collapsed = collapseChains(exact, exactStart, true, walk, walkStart, walkOrigin, &orderedExact, &orderedWalk);
    if (!orderedWalk) /* (what the engine asks before it groups and prunes; empty cells of the exact list need not be) */
        fail("the collapsed list's bounds are not ordered and finite");
    const int nw = buildWalkOrderList(walk, walkStart, walkOrigin, knobs, nullptr, &prunedBefore, &prunedAfter);
    printf("%d nodes, %d leaves, %d primitives; %d after the chains, %d in the walk-order list (%d + %d pruned)\n", n,
           (int)exactLeaves.size(), nbPrims, collapsed, nw, prunedBefore, prunedAfter);
    if (walk.size() != 2 * (size_t)nw || walkStart.size() != (size_t)nw || walkOrigin.size() != (size_t)nw)
        fail("walk-order list: %d nodes but %zu rows, %zu start indices, %zu origins", nw, walk.size(), walkStart.size(), walkOrigin.size());
    else if (nested("walk-order list", walk.data(), nw))
    {
        int last = -1;
        std::vector<int> seen(n, 0);
        for (int j = 0; j < nw; ++j)
        {
            const int o = walkOrigin[j];
            if (o < -1 || o >= n)
            {
                fail("walk-order list: node %d has origin %d", j, o);
                continue;
            }
            if (o < 0)
            {
                if (countOf(walk.data(), j) != 0)
                    fail("walk-order list: node %d is ours and has %d primitives", j, countOf(walk.data(), j));
                /* a node of ours is the union of its direct children: std::min / std::max in their order, bit for bit */
                float lo[3], hi[3], clo[3], chi[3];
                bool first = true;
                for (int c = j + 1; c < j + skipOf(walk.data(), j); c += skipOf(walk.data(), c))
                {
                    bounds(walk.data(), c, clo, chi);
                    for (int k = 0; k < 3; ++k)
                    {
                        lo[k] = first ? clo[k] : std::min(lo[k], clo[k]);
                        hi[k] = first ? chi[k] : std::max(hi[k], chi[k]);
                    }
                    first = false;
                }
                float own[3], ownHi[3];
                bounds(walk.data(), j, own, ownHi);
                if (first)
                    fail("walk-order list: node %d is ours and has no child", j);
                else if (memcmp(own, lo, 12) != 0 || memcmp(ownHi, hi, 12) != 0)
                    fail("walk-order list: node %d is ours, [%g %g %g .. %g %g %g], its children's union [%g %g %g .. %g %g %g]", j,
                         own[0], own[1], own[2], ownHi[0], ownHi[1], ownHi[2], lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
                continue;
            }
            if (o <= last)
                fail("walk-order list: node %d (origin %d) comes after origin %d", j, o, last);
            last = o;
            ++seen[o];
            if (!sameNode(walk.data(), j, exact.data(), o))
                fail("walk-order list: node %d is not node %d of the exact list bit for bit", j, o);
        }
        for (int leaf : exactLeaves)
            if (seen[leaf] != 1)
                fail("walk-order list: leaf %d of the exact list appears %d times", leaf, seen[leaf]);
        const bool a = listEnclosesOnHost(exact, exactStart, prims), b = listEnclosesOnHost(walk, walkStart, prims);
        printf("exact list encloses: %d, walk-order list: %d\n", (int)a, (int)b);
        if (a != b)
            fail("listEnclosesOnHost: %d for the exact list, %d for the walk-order list", (int)a, (int)b);
    }

    /* ---- the eight order-free lists ----------------------------------------------------------------------------------- */
    std::vector<int> identity(n);
    for (int i = 0; i < n; ++i)
        identity[i] = i;
    Rows freeRows;
    std::vector<int> freeStart, freeOrigin;
    int prunedFree = 0;
    const int count = buildFreeOrderLists(exact, exactStart, identity, freeRows, freeStart, freeOrigin, &prunedFree, knobs.pruneThreshold);
    printf("order-free lists: 8 x %d nodes (%d pruned)\n", count, prunedFree);
    /* (one length for all eight is how they are stored: what has to hold is that each fills its share) */
    if (count < 0 || freeRows.size() != 16 * (size_t)count || freeStart.size() != 8 * (size_t)count || freeOrigin.size() != 8 * (size_t)count)
        fail("order-free lists: 8 x %d nodes but %zu rows, %zu start indices, %zu origins", count, freeRows.size(), freeStart.size(),
             freeOrigin.size());
    else if (exactLeaves.size() >= 2 && count < (int)exactLeaves.size())
        fail("order-free lists: %d nodes for %zu leaves", count, exactLeaves.size());
    else
    {
        std::vector<int> order[8];
        for (int octant = 0; octant < 8 && count > 0; ++octant)
        {
            char what[32];
            snprintf(what, sizeof(what), "order-free list %d", octant);
            const float4 *rows = freeRows.data() + 2 * (size_t)octant * count;
            const int *origin = freeOrigin.data() + (size_t)octant * count;
            if (!nested(what, rows, count))
                continue;
            std::vector<int> seen(n, 0);
            for (int j = 0; j < count; ++j)
            {
                if (countOf(rows, j) > 0)
                {
                    const int o = origin[j];
                    if (o < 0 || o >= n || countOf(exact.data(), o) <= 0)
                    {
                        fail("%s: leaf %d has origin %d, no leaf of the exact list", what, j, o);
                        continue;
                    }
                    ++seen[o];
                    order[octant].push_back(o);
                    if (!sameNode(rows, j, exact.data(), o))
                        fail("%s: leaf %d is not leaf %d of the exact list bit for bit", what, j, o);
                    continue;
                }
                float lo[3], hi[3], clo[3], chi[3];
                bounds(rows, j, lo, hi);
                for (int c = j + 1; c < j + skipOf(rows, j); c += skipOf(rows, c))
                {
                    bounds(rows, c, clo, chi);
                    for (int k = 0; k < 3; ++k)
                        if (!(clo[k] >= lo[k] && chi[k] <= hi[k]))
                            fail("%s: node %d does not enclose its child %d on axis %d: [%g, %g] around [%g, %g]", what, j, c, k, lo[k],
                                 hi[k], clo[k], chi[k]);
                }
            }
            for (int leaf : exactLeaves)
                if (seen[leaf] != 1)
                    fail("%s: leaf %d of the exact list appears %d times", what, leaf, seen[leaf]);
        }
        if (count > 0 && exactLeaves.size() > 1 && order[0] == order[7])
            fail("order-free lists 0 and 7 visit the leaves in the same order");
    }

    /* ---- the refit plan -------------------------------------------------------------------------------------------------- */
    std::vector<int> plan, exactLevels, walkLevels, freeLevels;
    planRefit(exact, walk, walkOrigin, freeRows, freeOrigin, plan, exactLevels, walkLevels, freeLevels);
    printf("refit plan: %zu entries; %zu, %zu and %zu levels\n", plan.size(), exactLevels.size() / 2, walkLevels.size() / 2,
           freeLevels.size() / 2);
    checkLevels("refit plan, exact list", exact.data(), n, plan, exactLevels);
    checkLevels("refit plan, walk-order list", walk.data(), (int)walkStart.size(), plan, walkLevels);
    /* (the eight lists one behind the other: a child never lies in another list, skip pointers are nested in each) */
    checkLevels("refit plan, order-free lists", freeRows.data(), (int)freeStart.size(), plan, freeLevels);

    if (failures)
        fprintf(stderr, "%d condition(s) violated\n", failures);
    return failures ? 1 : 0;
}
