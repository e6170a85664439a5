/*
 * free_list_topology_check.cpp - the order-free lists built on build bounds (sol-r_amd/csrc/build_bounds.h) against the
 * same lists built on the boxes as uploaded: no engine, no device.  tests/test_free_list_topology.py compiles this file
 * with list_builders.cpp and runs it on a scene file (the format of list_builders_check.cpp):
 *   int32 n, int32 p | float32 rows[n][2][4] | int32 start[n] | float32 prims[p][8][4]
 *
 *   free_list_topology_check scene-file [--walls-at-top] [--share S] [--fat] [--dump file]
 *
 * It prints one line `fat <hash>` with the FNV-1a hash of what buildFreeOrderLists makes without build bounds (the test
 * holds it to the hash recorded from the builder before build bounds existed), one line `built <hash>` for the lists on
 * build bounds, `walls <count>` (leaves of nothing but axis-plane rectangles), `depth <max depth of such a leaf>` (with
 * --walls-at-top, for a room, whose walls dominate: a violation if it is more than 1), and
 * `visits <fat> <built>`: nodes a wave-synchronous walk visits, summed over a fixed grid of 8 x 8-ray beams from inside
 * the scene through the thin copies of both (no distance cut-off: an upper bound both sides share).  Every violated
 * condition is printed; the exit status is 1 if there was one.  --dump: the eight lists on build bounds (or, with
 * --share 0 --fat, on the uploaded boxes) as int32 count | rows | start | origin, for tools/free_list_visits.py.
 *
 * The hashes the test holds the `fat` line to were recorded from the builder of the commit before build bounds: this file
 * compiled with -DTOPOLOGY_CHECK_FAT_ONLY (only the `fat` line; nothing of build_bounds.h is named, so it builds against
 * that commit's list_builders.cpp and header as well as against this one's) in a checkout of that commit, run on the scene
 * files tests/test_free_list_topology.py writes.  To record them again for another scene:
 *   git worktree add /tmp/before <that commit>; cp tests/free_list_topology_check.cpp /tmp/before/tests/
 *   g++ -std=c++17 -ffp-contract=off -DTOPOLOGY_CHECK_FAT_ONLY -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include \
 *       /tmp/before/tests/free_list_topology_check.cpp /tmp/before/sol-r_amd/csrc/list_builders.cpp -o before_check
 */
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
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
struct Lists
{
    Rows rows;
    std::vector<int> start, origin;
    int count = 0, pruned = 0;
};
static int countOf(const float4 *rows, int i) { return bitsi(rows[2 * i + 1].z); }
static int skipOf(const float4 *rows, int i) { return bitsi(rows[2 * i + 1].w); }

static unsigned long long hashOf(const Lists &l)
{
    unsigned long long h = 1469598103934665603ull;
    auto eat = [&](const void *p, size_t bytes) {
        for (size_t k = 0; k < bytes; ++k)
            h = (h ^ ((const unsigned char *)p)[k]) * 1099511628211ull;
    };
    eat(&l.count, 4);
    eat(&l.pruned, 4);
    eat(l.rows.data(), l.rows.size() * 16);
    eat(l.start.data(), l.start.size() * 4);
    eat(l.origin.data(), l.origin.size() * 4);
    return h;
}

#ifndef TOPOLOGY_CHECK_FAT_ONLY
/* the scene's extent as the engine takes it for the thin copies' margin: the largest finite |coordinate| of p0 / p1 / p2,
 * at least 1, plus the largest finite |size| component */
static float extentOf(const Rows &prims)
{
    float e = 1.f, reach = 0.f;
    for (size_t p = 0; p < prims.size() / LB_PRIM_ROWS; ++p)
    {
        const float4 *r = &prims[LB_PRIM_ROWS * p];
        for (const float4 *v : {&r[LB_ROW_P0_TYPE], &r[LB_ROW_P1_INDEX], &r[LB_ROW_P2]})
            for (float c : {fabsf(v->x), fabsf(v->y), fabsf(v->z)})
                if (c < 3.0e38f && c > e)
                    e = c;
        for (float s : {fabsf(r[LB_ROW_SIZE_MAT].x), fabsf(r[LB_ROW_SIZE_MAT].y), fabsf(r[LB_ROW_SIZE_MAT].z)})
            if (s < 3.0e38f && s > reach)
                reach = s;
    }
    return e + reach;
}

/* the thin copy of one list (solr_arena.hip k_tightenLeaves / k_tightenInner; plane leaves by type: the scenes here have
 * plain materials) */
static Rows thinCopy(const float4 *rows, const int *start, int n, const Rows &prims, float margin)
{
    Rows thin(rows, rows + 2 * (size_t)n);
    for (int i = 0; i < n; ++i)
    {
        float lo[3], hi[3];
        if (countOf(rows, i) > 0 && leafBuildBounds(rows[2 * i], rows[2 * i + 1], prims.data(), start[i], countOf(rows, i), margin, lo, hi))
        {
            thin[2 * i] = make_float4(lo[0], lo[1], lo[2], hi[2]);
            thin[2 * i + 1].x = hi[0], thin[2 * i + 1].y = hi[1];
        }
    }
    for (int i = 0; i < n; ++i)
    {
        if (countOf(rows, i) > 0 || skipOf(rows, i) <= 1)
            continue;
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int j = i + 1; j < std::min(i + skipOf(rows, i), n); ++j)
            if (countOf(rows, j) > 0)
            {
                lo[0] = fminf(lo[0], thin[2 * j].x), lo[1] = fminf(lo[1], thin[2 * j].y), lo[2] = fminf(lo[2], thin[2 * j].z);
                hi[0] = fmaxf(hi[0], thin[2 * j + 1].x), hi[1] = fmaxf(hi[1], thin[2 * j + 1].y), hi[2] = fmaxf(hi[2], thin[2 * j].w);
            }
        const float nlx = fmaxf(rows[2 * i].x, lo[0]), nly = fmaxf(rows[2 * i].y, lo[1]), nlz = fmaxf(rows[2 * i].z, lo[2]);
        const float nhx = fminf(rows[2 * i + 1].x, hi[0]), nhy = fminf(rows[2 * i + 1].y, hi[1]), nhz = fminf(rows[2 * i].w, hi[2]);
        if (!(nlx <= nhx && nly <= nhy && nlz <= nhz))
            continue;
        thin[2 * i] = make_float4(nlx, nly, nlz, nhz);
        thin[2 * i + 1].x = nhx, thin[2 * i + 1].y = nhy;
    }
    return thin;
}

/* Nodes a wave visits on one list: a node is visited when the wave's cursor reaches it, its children when any ray's
 * slab test passes (binary32: (b - o) * (1 / d) per axis, entered if tnear <= tfar and tfar > 0). */
static long visitsOf(const Rows &thin, int n, const float o[3], const float (*d)[3], int rays)
{
    long visited = 0;
    for (int i = 0; i < n;)
    {
        ++visited;
        if (countOf(thin.data(), i) > 0)
        {
            ++i;
            continue;
        }
        const float lo[3] = {thin[2 * i].x, thin[2 * i].y, thin[2 * i].z}, hi[3] = {thin[2 * i + 1].x, thin[2 * i + 1].y, thin[2 * i].w};
        bool any = false;
        for (int r = 0; r < rays && !any; ++r)
        {
            float tnear = -INFINITY, tfar = INFINITY;
            for (int k = 0; k < 3; ++k)
            {
                const float inv = 1.f / d[r][k];
                const float a = (lo[k] - o[k]) * inv, b = (hi[k] - o[k]) * inv;
                tnear = fmaxf(tnear, fminf(a, b));
                tfar = fminf(tfar, fmaxf(a, b));
            }
            any = tnear <= tfar && tfar > 0.f;
        }
        i += any ? 1 : std::max(skipOf(thin.data(), i), 1);
    }
    return visited;
}

#endif

int main(int argc, char **argv)
{
    const char *dump = nullptr;
#ifndef TOPOLOGY_CHECK_FAT_ONLY
    double share = SOLR_DOMINANT_SHARE;
#else
    double share = 0.0;
#endif
    bool dumpFat = false, wallsAtTop = false;
    if (argc < 2)
    {
        fprintf(stderr, "usage: %s scene-file [--walls-at-top] [--share S] [--fat] [--dump file]\n", argv[0]);
        return 2;
    }
    for (int a = 2; a < argc; ++a)
        if (!strcmp(argv[a], "--share") && a + 1 < argc)
            share = atof(argv[++a]);
        else if (!strcmp(argv[a], "--dump") && a + 1 < argc)
            dump = argv[++a];
        else if (!strcmp(argv[a], "--fat"))
            dumpFat = true;
        else if (!strcmp(argv[a], "--walls-at-top"))
            wallsAtTop = true;
    FILE *f = fopen(argv[1], "rb");
    int head[2] = {0, 0};
    if (!f || fread(head, 4, 2, f) != 2 || head[0] < 1 || head[1] < 0)
    {
        fprintf(stderr, "%s: not a scene file\n", argv[1]);
        return 2;
    }
    const int n = head[0], nbPrims = head[1];
    Rows exact(2 * (size_t)n), prims((size_t)LB_PRIM_ROWS * nbPrims);
    std::vector<int> exactStart(n), identity(n);
    if (fread(exact.data(), 16, exact.size(), f) != exact.size() || fread(exactStart.data(), 4, n, f) != (size_t)n ||
        fread(prims.data(), 16, prims.size(), f) != prims.size())
    {
        fprintf(stderr, "%s: truncated\n", argv[1]);
        return 2;
    }
    fclose(f);
    for (int i = 0; i < n; ++i)
        identity[i] = i;
    const ListKnobs knobs;

    Lists fat, built;
    fat.count = buildFreeOrderLists(exact, exactStart, identity, fat.rows, fat.start, fat.origin, &fat.pruned, knobs.pruneThreshold);
    printf("fat %016llx\n", hashOf(fat));
#ifndef TOPOLOGY_CHECK_FAT_ONLY
    const float margin = extentOf(prims) * (1.f / 1024.f);
    BuildBounds build;
    build.prims = prims.data();
    build.margin = margin;
    build.dominantShare = share;
    built.count = buildFreeOrderLists(exact, exactStart, identity, built.rows, built.start, built.origin, &built.pruned, knobs.pruneThreshold,
                                      nullptr, build);
    printf("built %016llx\n", hashOf(built));
    printf("nodes %d %d\n", fat.count, built.count);
    if (fat.count <= 0 || built.count <= 0)
    {
        fail("no lists: %d nodes on the uploaded boxes, %d on build bounds", fat.count, built.count);
        return 1;
    }
    if (built.rows.size() != 16 * (size_t)built.count || built.start.size() != 8 * (size_t)built.count ||
        built.origin.size() != 8 * (size_t)built.count)
    {
        fail("8 x %d nodes but %zu rows, %zu start indices, %zu origins", built.count, built.rows.size(), built.start.size(), built.origin.size());
        return 1;
    }
    /* which leaves of the exact list hold nothing but axis-plane rectangles */
    std::vector<char> wall(n, 0);
    int walls = 0;
    for (int i = 0; i < n; ++i)
    {
        float lo[3], hi[3];
        wall[i] = countOf(exact.data(), i) > 0 &&
                  leafBuildBounds(exact[2 * i], exact[2 * i + 1], prims.data(), exactStart[i], countOf(exact.data(), i), margin, lo, hi);
        walls += wall[i];
    }
    printf("walls %d\n", walls);
    int deepest = 0;
    for (int octant = 0; octant < 8; ++octant)
    {
        const float4 *rows = built.rows.data() + 2 * (size_t)octant * built.count, *fatRows = fat.rows.data() + 2 * (size_t)octant * fat.count;
        const int *start = built.start.data() + (size_t)octant * built.count, *origin = built.origin.data() + (size_t)octant * built.count;
        const int *fatStart = fat.start.data() + (size_t)octant * fat.count, *fatOrigin = fat.origin.data() + (size_t)octant * fat.count;
        /* the same leaves, start indices and origins as without: as sets (the order is the hierarchy's) */
        struct LeafOf
        {
            int origin, start;
            float4 a, b;
            bool operator<(const LeafOf &o) const { return origin < o.origin; }
        };
        std::vector<LeafOf> mine, theirs;
        for (int j = 0; j < built.count; ++j)
            if (countOf(rows, j) > 0)
                mine.push_back({origin[j], start[j], rows[2 * j], rows[2 * j + 1]});
        for (int j = 0; j < fat.count; ++j)
            if (countOf(fatRows, j) > 0)
                theirs.push_back({fatOrigin[j], fatStart[j], fatRows[2 * j], fatRows[2 * j + 1]});
        std::sort(mine.begin(), mine.end());
        std::sort(theirs.begin(), theirs.end());
        if (mine.size() != theirs.size())
            fail("list %d: %zu leaves, %zu without build bounds", octant, mine.size(), theirs.size());
        else
            for (size_t q = 0; q < mine.size(); ++q)
                if (mine[q].origin != theirs[q].origin || mine[q].start != theirs[q].start || memcmp(&mine[q].a, &theirs[q].a, 16) != 0 ||
                    memcmp(&mine[q].b, &theirs[q].b, 16) != 0)
                    fail("list %d: leaf of origin %d differs from the one without build bounds (origin %d)", octant, mine[q].origin,
                         theirs[q].origin);
        /* nested skip pointers, depths, inner rows */
        std::vector<int> ends;
        for (int j = 0; j < built.count; ++j)
        {
            const int skip = skipOf(rows, j);
            if (skip < 1 || j + skip > built.count)
            {
                fail("list %d: node %d has skip %d in a list of %d", octant, j, skip, built.count);
                break;
            }
            while (!ends.empty() && ends.back() <= j)
                ends.pop_back();
            if (!ends.empty() && j + skip > ends.back())
            {
                fail("list %d: node %d ends at %d, beyond its parent's %d", octant, j, j + skip, ends.back());
                break;
            }
            const int depth = (int)ends.size();
            ends.push_back(j + skip);
            if (countOf(rows, j) > 0)
            {
                if (skip != 1)
                    fail("list %d: leaf %d has skip %d", octant, j, skip);
                if (origin[j] >= 0 && origin[j] < n && wall[origin[j]])
                {
                    deepest = std::max(deepest, depth);
                    if (wallsAtTop && depth > 1)
                        fail("list %d: the wall leaf %d (origin %d) lies at depth %d", octant, j, origin[j], depth);
                }
                continue;
            }
            if (origin[j] != -1 || start[j] != 0)
                fail("list %d: inner node %d has origin %d, start %d", octant, j, origin[j], start[j]);
            /* the union of its leaves' boxes as uploaded, zeros +0, bit for bit */
            float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
            for (int c = j + 1; c < j + skip; ++c)
                if (countOf(rows, c) > 0)
                {
                    lo[0] = std::min(lo[0], rows[2 * c].x), lo[1] = std::min(lo[1], rows[2 * c].y), lo[2] = std::min(lo[2], rows[2 * c].z);
                    hi[0] = std::max(hi[0], rows[2 * c + 1].x), hi[1] = std::max(hi[1], rows[2 * c + 1].y), hi[2] = std::max(hi[2], rows[2 * c].w);
                }
            for (int k = 0; k < 3; ++k)
                lo[k] += 0.f, hi[k] += 0.f;
            const float4 a = make_float4(lo[0], lo[1], lo[2], hi[2]);
            const float own[2] = {rows[2 * j + 1].x, rows[2 * j + 1].y}, want[2] = {hi[0], hi[1]};
            if (memcmp(&rows[2 * j], &a, 16) != 0 || memcmp(own, want, 8) != 0)
                fail("list %d: inner node %d is not the union of its leaves' uploaded boxes", octant, j);
        }
    }
    printf("depth %d\n", deepest);

    /* the visit model: beams of 8 x 8 rays from a point inside the scene (a quarter of the way in along z, like the
     * camera of the Cornell room), 16 x 12 tiles over a view 0.8 x 0.6 of the distance wide, each on the list of its
     * first ray's octant */
    {
        float slo[3] = {1e30f, 1e30f, 1e30f}, shi[3] = {-1e30f, -1e30f, -1e30f};
        for (int j = 0; j < n; ++j)
            if (countOf(exact.data(), j) > 0)
            {
                float lo[3], hi[3];
                leafBuildBounds(exact[2 * j], exact[2 * j + 1], prims.data(), exactStart[j], countOf(exact.data(), j), margin, lo, hi);
                for (int k = 0; k < 3; ++k)
                    slo[k] = std::min(slo[k], lo[k]), shi[k] = std::max(shi[k], hi[k]);
            }
        const float eye[3] = {0.5f * (slo[0] + shi[0]) + 0.01f * (shi[0] - slo[0]), slo[1] + 0.3f * (shi[1] - slo[1]), slo[2] + 0.125f * (shi[2] - slo[2])};
        const float depth = 0.5f * (shi[2] - slo[2]);
        std::vector<Rows> thinFat(8), thinBuilt(8);
        for (int octant = 0; octant < 8; ++octant)
        {
            thinFat[octant] = thinCopy(fat.rows.data() + 2 * (size_t)octant * fat.count, fat.start.data() + (size_t)octant * fat.count, fat.count, prims, margin);
            thinBuilt[octant] = thinCopy(built.rows.data() + 2 * (size_t)octant * built.count, built.start.data() + (size_t)octant * built.count, built.count, prims, margin);
        }
        long fatVisits = 0, builtVisits = 0;
        const int tilesX = 16, tilesY = 12;
        for (int ty = 0; ty < tilesY; ++ty)
            for (int tx = 0; tx < tilesX; ++tx)
            {
                float d[64][3];
                for (int lane = 0; lane < 64; ++lane)
                {
                    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
                    d[lane][0] = -0.8f * depth * ((float)(x - tilesX * 4) + 0.25f) / (float)(tilesX * 8);
                    d[lane][1] = 0.6f * depth * ((float)(y - tilesY * 4) + 0.25f) / (float)(tilesY * 8);
                    d[lane][2] = depth;
                }
                const int octant = (d[0][0] < 0.f ? 1 : 0) | (d[0][1] < 0.f ? 2 : 0) | (d[0][2] < 0.f ? 4 : 0);
                fatVisits += visitsOf(thinFat[octant], fat.count, eye, d, 64);
                builtVisits += visitsOf(thinBuilt[octant], built.count, eye, d, 64);
            }
        printf("visits %ld %ld\n", fatVisits, builtVisits);
    }
    const Lists &out = dumpFat ? fat : built;
#else
    const Lists &out = fat;
    (void)dumpFat, (void)share, (void)wallsAtTop;
#endif
    if (dump)
    {
        FILE *o = fopen(dump, "wb");
        if (!o)
            return 2;
        fwrite(&out.count, 4, 1, o);
        fwrite(out.rows.data(), 16, out.rows.size(), o);
        fwrite(out.start.data(), 4, out.start.size(), o);
        fwrite(out.origin.data(), 4, out.origin.size(), o);
        fclose(o);
    }
    if (failures)
        fprintf(stderr, "%d condition(s) violated\n", failures);
    return failures ? 1 : 0;
}
