/*
 * solr_arena.hip - the arena of the resident scene (scene_layout.h) and the lists the walks take:
 *   - the arena's device kernels: leaf records, thin copies of plain-plane leaves, copies with sorted bounds, the
 *     enclosure check;
 *   - the arena against its host images: laid out and uploaded (flushGeometry), the order-free lists added behind it
 *     (appendFreeLists), the host images brought up to date (pullGeometry, ensureHostFreeLists).  The order-free lists
 *     are built on the device (solr_lists.hip) when they are due, by the host builders where that is switched off or
 *     declines;
 *   - which short cuts a walk may be offered (the four predicates), and prepareScene(): the SceneArgs a frame's launch is
 *     handed.
 * The uploads: solr_uploads.hip; rotation on the device: solr_rotation.hip.
 * Part of the engine's host side (engine.h); the boundary that calls into it is solr_hip.hip.  gfx950 only.
 */
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/solr_hip.h"
#include "rt_device.h"

using namespace solrdev;

#include "renderer.h"
#include "engine.h"

using namespace solreng;

namespace solreng
{
/* Leaf records (scene_layout.h): for every leaf of a node list, the first primitive's test data and index in
 * one 64-byte line.  A function of the primitive records and the list's start indices alone: run after every
 * upload of the arena and after every device-side rotation of the primitives. */
__global__ __launch_bounds__(256) void k_buildLeafRecords(float4 *__restrict__ arena, unsigned offNodes, unsigned offStart,
                                                         unsigned offPrims, unsigned offLeaf, int nbNodes)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nbNodes)
        return;
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0, r3 = r0;
    const int nb = __float_as_int(arena[offNodes + 2u * (unsigned)i + 1u].z);
    if (nb > 0)
    {
        const int start = ((const int *)arena)[offStart + (unsigned)i];
        const float4 *prim = arena + offPrims + 8u * (unsigned)start;
        r0 = prim[ROW_P0_TYPE];
        r1 = prim[ROW_SIZE_MAT];
        r2 = prim[ROW_P1_INDEX];
        r3 = prim[ROW_P2];
        if (planeClass(__float_as_int(r0.w) & PRIM_TYPE_MASK))
        {
            const float4 n0 = prim[ROW_N0];
            r2 = make_float4(n0.x, n0.y, n0.z, r2.w);
            r3 = make_float4(r3.w, 0.f, 0.f, 0.f);
        }
        r3.w = __int_as_float(start);
    }
    float4 *out = arena + offLeaf + 4u * (unsigned)i;
    out[0] = r0;
    out[1] = r1;
    out[2] = r2;
    out[3] = r3;
}

/* The thin copy of a node list (rt_device.h tightRay; scene_layout.h SceneArgs::tightLists): leaf by leaf.  A leaf
 * whose primitives are all plain axis planes becomes the union of their rectangles, `margin` thick and `margin` wider,
 * cut with the reference's box (never larger than it: a ray the thin box lets in, the reference's let in as well);
 * with a `reach`, a leaf whose primitives are all KIND_SPHERE becomes the union of their boxes for rays from within
 * that reach (build_bounds.h sphereBuildExtent), cut alike - the lamps' cell is the one the reference boxes larger;
 * every other node is copied.  k_tightenInner then makes the inner nodes the unions of the leaves below them. */
__global__ __launch_bounds__(256) void k_tightenLeaves(float4 *__restrict__ arena, unsigned offNodes, unsigned offTight,
                                                      unsigned offStart, unsigned offPrims, int nbNodes, float margin, float reach)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nbNodes)
        return;
    float4 row0 = arena[offNodes + 2u * (unsigned)i], row1 = arena[offNodes + 2u * (unsigned)i + 1u];
    const int nb = __float_as_int(row1.z);
    if (nb > 0)
    {
        /* (build_bounds.h: the rectangles' union cut with the box, finite and ordered, or the reference's box stays; by the
         * records' kinds - a plane that is textured, transparent or emissive keeps its box, and so does a procedural sphere) */
        static_assert(BB_KIND_SHIFT == PRIM_KIND_SHIFT && BB_KIND_PLANE_XY == KIND_PLANE_XY && BB_KIND_PLANE_YZ == KIND_PLANE_YZ &&
                          BB_KIND_PLANE_XZ == KIND_PLANE_XZ && BB_KIND_SPHERE == KIND_SPHERE && ROW_P0_TYPE == 0 && ROW_SIZE_MAT == 1,
                      "build_bounds.h reads the primitive records as scene_layout.h lays them out");
        const int start = ((const int *)arena)[offStart + (unsigned)i];
        float lo[3], hi[3];
        if (leafBuildBounds(row0, row1, arena + offPrims, start, nb, margin, lo, hi, true, reach))
        {
            row0 = make_float4(lo[0], lo[1], lo[2], hi[2]);
            row1 = make_float4(hi[0], hi[1], row1.z, row1.w);
        }
    }
    arena[offTight + 2u * (unsigned)i] = row0;
    arena[offTight + 2u * (unsigned)i + 1u] = row1;
}

/* inner node i of the thin copy: the union of the leaves of its subtree (nodes i + 1 ... i + skip - 1: skip pointers
 * are nested intervals), cut with its own box.  A group still passes whenever one of its members does. */
__global__ __launch_bounds__(256) void k_tightenInner(float4 *__restrict__ arena, unsigned offTight, int nbNodes, int listLength)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nbNodes)
        return;
    const float4 row0 = arena[offTight + 2u * (unsigned)i], row1 = arena[offTight + 2u * (unsigned)i + 1u];
    const int nb = __float_as_int(row1.z), skip = __float_as_int(row1.w);
    if (nb > 0 || skip <= 1)
        return;
    const int listEnd = (i / listLength + 1) * listLength; /* (several lists one behind the other: stay in this one) */
    const int end = min(i + skip, listEnd);
    float lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
    for (int j = i + 1; j < end; ++j)
    {
        const float4 b = arena[offTight + 2u * (unsigned)j + 1u];
        if (__float_as_int(b.z) <= 0)
            continue;
        const float4 a = arena[offTight + 2u * (unsigned)j];
        lx = fminf(lx, a.x), ly = fminf(ly, a.y), lz = fminf(lz, a.z);
        hx = fmaxf(hx, b.x), hy = fmaxf(hy, b.y), hz = fmaxf(hz, a.w);
    }
    const float nlx = fmaxf(row0.x, lx), nly = fmaxf(row0.y, ly), nlz = fmaxf(row0.z, lz);
    const float nhx = fminf(row1.x, hx), nhy = fminf(row1.y, hy), nhz = fminf(row0.w, hz);
    if (!(nlx <= nhx && nly <= nhy && nlz <= nhz))
        return; /* no leaf below it, or bounds that are not numbers: the reference's box stays */
    arena[offTight + 2u * (unsigned)i] = make_float4(nlx, nly, nlz, nhz);
    arena[offTight + 2u * (unsigned)i + 1u] = make_float4(nhx, nhy, row1.z, row1.w);
}

/* maybeBuildOrderFreeLists' precondition, for the exact list as the arena holds it: every inner node holds its
 * direct children, every leaf its primitives (the same float arithmetic as the host loop there, which stays as the
 * route for an arena that is not laid out).  *bad is raised for a node that does not. */
__global__ __launch_bounds__(256) void k_listEncloses(const float4 *__restrict__ arena, unsigned offNodes, unsigned offStart,
                                                      unsigned offPrims, int nbNodes, int nbPrims, int *bad)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nbNodes)
        return;
    const float4 a = arena[offNodes + 2u * (unsigned)i], b = arena[offNodes + 2u * (unsigned)i + 1u];
    const int count = __float_as_int(b.z);
    const int end = min(i + max(__float_as_int(b.w), 1), nbNodes);
    bool encloses = true;
    if (count <= 0)
    {
        for (int j = i + 1; j < end && encloses;)
        {
            const float4 ca = arena[offNodes + 2u * (unsigned)j], cb = arena[offNodes + 2u * (unsigned)j + 1u];
            encloses = ca.x >= a.x && ca.y >= a.y && ca.z >= a.z && cb.x <= b.x && cb.y <= b.y && ca.w <= a.w;
            j += max(__float_as_int(cb.w), 1);
        }
    }
    else
    {
        const int start = ((const int *)arena)[offStart + (unsigned)i];
        for (int k = 0; k < count && encloses; ++k)
        {
            const long long pi = (long long)start + k;
            if (start < 0 || pi >= nbPrims)
            {
                encloses = false;
                break;
            }
            const float4 *r = arena + offPrims + (size_t)PRIM_ROWS * (size_t)pi;
            const float4 p0 = r[ROW_P0_TYPE], size = r[ROW_SIZE_MAT];
            const int type = __float_as_int(p0.w) & PRIM_TYPE_MASK;
            float lo[3] = {p0.x, p0.y, p0.z}, hi[3] = {p0.x, p0.y, p0.z};
            auto add = [&](const float4 &v) {
                lo[0] = v.x < lo[0] ? v.x : lo[0], lo[1] = v.y < lo[1] ? v.y : lo[1], lo[2] = v.z < lo[2] ? v.z : lo[2];
                hi[0] = hi[0] < v.x ? v.x : hi[0], hi[1] = hi[1] < v.y ? v.y : hi[1], hi[2] = hi[2] < v.z ? v.z : hi[2];
            };
            float grow[3] = {size.x, size.y, size.z};
            if (type == ptTriangle)
            {
                add(r[ROW_P1_INDEX]);
                add(r[ROW_P2]);
                grow[0] = grow[1] = grow[2] = 0.f;
            }
            else if (type == ptCylinder)
            {
                add(r[ROW_P1_INDEX]);
                grow[1] = grow[2] = grow[0];
            }
            else if (type == ptSphere)
                grow[1] = grow[2] = grow[0];
            auto larger = [](float x, float y) { return x < y ? y : x; }; /* std::max */
            auto slack = [&](int k) { return 4.f * 1.1920929e-7f * larger(larger(fabsf(lo[k]), fabsf(hi[k])), fabsf(grow[k])); };
            const float ex = slack(0), ey = slack(1), ez = slack(2);
            encloses = a.x <= lo[0] - fabsf(grow[0]) + ex && a.y <= lo[1] - fabsf(grow[1]) + ey && a.z <= lo[2] - fabsf(grow[2]) + ez &&
                       b.x >= hi[0] + fabsf(grow[0]) - ex && b.y >= hi[1] + fabsf(grow[1]) - ey && a.w >= hi[2] + fabsf(grow[2]) - ez;
        }
    }
    if (!encloses)
        *bad = 1;
}

/* host images of order-free lists that were built on the device: from where they are now */
void ensureHostFreeLists()
{
    if (g.scene.lists.freeHostValid || !ok())
        return;
    quiesce();
    NodeList &list = g.scene.orderFree;
    const size_t n = list.nodes();
    list.rows.resize(2 * n);
    list.start.resize(n);
    list.origin.resize(n);
    const bool staged = g.scene.lists.freeStage.rows != nullptr;
    const char *arena = (const char *)g.scene.arena.geometry.ptr;
    if (!staged && !arena)
    {
        setError(-1, "order-free lists neither staged nor in the arena", __FILE__, __LINE__);
        return;
    }
    HIPCHECK(hipMemcpy(list.rows.data(), staged ? (const void *)g.scene.lists.freeStage.rows : arena + (size_t)list.offRows * 16, 2 * n * 16,
                       hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(list.start.data(), staged ? (const void *)g.scene.lists.freeStage.start : arena + (size_t)list.offStart * 4, n * 4,
                       hipMemcpyDeviceToHost));
    if (g.scene.lists.freeStage.origin)
        HIPCHECK(hipMemcpy(list.origin.data(), g.scene.lists.freeStage.origin, n * 4, hipMemcpyDeviceToHost));
    if (ok())
    {
        g.scene.hostListsPulled();
    }
}

/* the arena moved on (device-side rotations): bring the host images up to date before anything reads them */
void pullGeometry()
{
    if (!g.scene.arena.deviceAhead || !g.scene.arena.geometry.ptr)
        return;
    refreshExactList();
    quiesce();
    auto get = [&](unsigned at, void *dst, size_t bytes) {
        if (bytes)
            HIPCHECK(hipMemcpy(dst, (const char *)g.scene.arena.geometry.ptr + (size_t)at * 16, bytes, hipMemcpyDeviceToHost));
    };
    for (NodeList *list : {&g.scene.exact, &g.scene.walk, &g.scene.orderFree})
        if (list != &g.scene.orderFree || g.scene.lists.freeHostValid)
            get(list->offRows, list->rows.data(), list->rows.size() * 16);
    get(g.scene.arena.offPrims, g.scene.hostPrims.data(), g.scene.hostPrims.size() * 16);
    g.scene.hostImagesPulled();
}

/* The reach the thin boxes of sphere leaves are made for (build_bounds.h sphereBuildExtent): the origins of the rays that
 * take the thin copies lie within the frame's viewDistance of zero (rt_device.h tightRay), the scene's extent where no
 * frame has said more.  0: sphere leaves keep their boxes (VARIANT_UPLOADED_SPHERE_LEAVES). */
float thinReachWanted(float viewDistance)
{
    if (g.variant == VARIANT_UPLOADED_SPHERE_LEAVES)
        return 0.f;
    return viewDistance > g.facts.sceneExtent ? viewDistance : g.facts.sceneExtent;
}

/* The thin copy of a node list behind it (NodeList::offThin; rt_device.h tightRay): made where the scene has
 * plain axis planes at all - or spheres that a kernel which walks thin copies tests (thinLeaves there: the F_PLANE rows) -
 * and the list is short enough for an inner node's thread to read its whole subtree (the
 * room of a 100 k-triangle model keeps the reference's boxes).  false: there is no copy to walk. */
static bool tightenList(const NodeList &list)
{
    static const bool off = getenv("SOLR_HIP_NO_TIGHT_LEAVES") != nullptr;
    const int nbNodes = (int)list.nodes(), listLength = list.nb;
    const bool worth = g.facts.plainPlanes || (g.facts.looseSpheres && (g.facts.sceneFeatures & F_PLANE) != 0);
    if (off || !worth || nbNodes <= 0 || listLength <= 0 || listLength > 65536 || !ok())
        return false;
    float4 *arena = (float4 *)g.scene.arena.geometry.ptr;
    const float margin = g.facts.sceneExtent * (1.f / 1024.f);
    const dim3 grid((unsigned)((nbNodes + 255) / 256));
    hipLaunchKernelGGL(k_tightenLeaves, grid, dim3(256), 0, sceneStream(), arena, list.offRows, list.offThin(), list.offStart, g.scene.arena.offPrims,
                       nbNodes, margin, g.facts.thinReach);
    hipLaunchKernelGGL(k_tightenInner, grid, dim3(256), 0, sceneStream(), arena, list.offThin(), nbNodes, listLength);
    HIPCHECK(hipGetLastError());
    return ok();
}

/* The eight order-free lists once more, behind their thin copies: every node's two rows with its bounds as (near, far) per
 * axis for the octant the list was flattened for (bit 0: x, 1: y, 2: z negative) - {n.x, n.y, n.z, f.z} {f.x, f.y, count,
 * 32 x skip} (scene_layout.h sortedLists; rt_device.h SOLR_ORDER_SORTED, SOLR_NEXT_BY_BYTES).  Made wherever the lists'
 * bounds change. */
__global__ __launch_bounds__(256) void k_sortNodeBounds(float4 *__restrict__ arena, unsigned offBoxesFree, unsigned offSorted, int nb)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > 8 * nb)
        return;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a; /* (i == 8 nb: the pad record behind the last list) */
    if (i < 8 * nb)
    {
        const int octant = i / nb;
        a = arena[offBoxesFree + 2u * (unsigned)i];
        b = arena[offBoxesFree + 2u * (unsigned)i + 1u];
        if (octant & 1)
        {
            const float t = a.x;
            a.x = b.x;
            b.x = t;
        }
        if (octant & 2)
        {
            const float t = a.y;
            a.y = b.y;
            b.y = t;
        }
        if (octant & 4)
        {
            const float t = a.z;
            a.z = a.w;
            a.w = t;
        }
        /* the skip word in BYTES: the loop that walks this copy keeps its cursors in bytes (rt_device.h SOLR_NEXT_BY_BYTES) */
        b.w = __int_as_float(__float_as_int(b.w) << 5);
    }
    arena[offSorted + 2u * (unsigned)i] = a;
    arena[offSorted + 2u * (unsigned)i + 1u] = b;
}

static bool sortFreeLists()
{
    static const bool off = getenv("SOLR_HIP_NO_SORTED_LISTS") != nullptr;
    const NodeList &list = g.scene.orderFree;
    if (off || list.nb <= 0 || !ok())
        return false;
    hipLaunchKernelGGL(k_sortNodeBounds, dim3((unsigned)((8 * list.nb + 1 + 255) / 256)), dim3(256), 0, sceneStream(),
                       (float4 *)g.scene.arena.geometry.ptr, list.offRows, list.offSorted(), list.nb);
    HIPCHECK(hipGetLastError());
    return ok();
}

/* what the arena holds of a list beyond its rows, from those and the primitive records as they are now: the leaf
 * records, and the copies behind the rows - they follow the bounds and the primitives they were made from (an upload, a
 * rotation on the device).  Order-free lists that a rotation left behind (freeStale) get none. */
static void deriveList(NodeList &list)
{
    const bool orderFree = &list == &g.scene.orderFree;
    const int n = (orderFree && g.scene.lists.freeStale) ? 0 : (int)list.nodes();
    if (n > 0)
        hipLaunchKernelGGL(k_buildLeafRecords, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sceneStream(), (float4 *)g.scene.arena.geometry.ptr,
                           list.offRows, list.offStart, g.scene.arena.offPrims, list.offLeaf, n);
    HIPCHECK(hipGetLastError());
    list.tight = list.copies > 1 && n > 0 && tightenList(list);
    if (orderFree)
        g.scene.lists.sortedFree = n > 0 && sortFreeLists();
}

/* the leaf records of every node list from the primitive records as the arena holds them now */
void buildLeafRecords()
{
    if (!ok() || !g.scene.arena.geometry.ptr)
        return;
    for (NodeList *list : {&g.scene.exact, &g.scene.walk, &g.scene.orderFree})
        deriveList(*list);
    HIPCHECK(hipStreamSynchronize(sceneStream()));
}

/* The thin copies alone, from the node rows and the primitive records as the arena holds them now: a sphere's thin box
 * follows its centre (solr_moves.hip moveLampOne: the lamps' cell is never refitted, its thin box moves with the lamp) and
 * the reach it was made for (prepareScene).  Nothing may be walking the copies (quiesce). */
void tightenListsAgain()
{
    if (!ok() || !g.scene.arena.geometry.ptr)
        return;
    for (NodeList *list : {&g.scene.walk, &g.scene.orderFree})
        if (list->tight)
            list->tight = tightenList(*list);
    HIPCHECK(hipStreamSynchronize(sceneStream()));
}

/* the lists the device builder left (g.scene.lists.freeStage) to their place in the arena */
static void copyStagedLists()
{
    const NodeList &list = g.scene.orderFree;
    char *arena = (char *)g.scene.arena.geometry.ptr;
    const SolrDeviceLists &stage = g.scene.lists.freeStage;
    HIPCHECK(hipMemcpyAsync(arena + (size_t)list.offRows * 16, stage.rows, (size_t)list.nodes() * 32, hipMemcpyDeviceToDevice, sceneStream()));
    HIPCHECK(hipMemcpyAsync(arena + (size_t)list.offStart * 4, stage.start, (size_t)list.nodes() * 4, hipMemcpyDeviceToDevice, sceneStream()));
}

/* the lists the device builder has just left (g.scene.lists.freeStage) into an arena that holds everything else already: what
 * is there stays where it is (moved to a larger allocation when this one is too small), nothing is uploaded again */
static void appendFreeLists()
{
    /* (the order-free lists lie behind everything else, so that they can be added to an arena that is laid out) */
    const unsigned end = g.scene.orderFree.layLeaf(g.scene.orderFree.layStart(g.scene.orderFree.layRows(g.scene.arena.rowsFixed)));
    const size_t bytes = (size_t)end * 16, fixedBytes = (size_t)g.scene.arena.rowsFixed * 16;
    PhaseTimer phase;
    if (g.scene.arena.geometry.bytes < bytes)
    {
        DeviceBuffer larger;
        reserve(larger, bytes);
        if (!ok())
            return;
        HIPCHECK(hipMemcpyAsync(larger.ptr, g.scene.arena.geometry.ptr, fixedBytes, hipMemcpyDeviceToDevice, sceneStream()));
        HIPCHECK(hipStreamSynchronize(sceneStream()));
        release(g.scene.arena.geometry);
        g.scene.arena.geometry = larger;
    }
    HIPCHECK(hipMemsetAsync((char *)g.scene.arena.geometry.ptr + fixedBytes, 0, bytes - fixedBytes, sceneStream()));
    copyStagedLists();
    if (ok())
        deriveList(g.scene.orderFree);
    HIPCHECK(hipStreamSynchronize(sceneStream()));
    phase.mark("geometry: lists appended");
    if (ok())
        g.scene.listsAppended();
}

/* assemble and upload the geometry arena from its host images (scene_layout.h) */
void flushGeometry()
{
    if (!g.scene.arena.geometryDirty)
    {
        if (g.scene.lists.freeDirty && g.scene.lists.freeStage.rows && g.scene.arena.geometry.ptr && g.scene.arena.rowsFixed > 0)
            appendFreeLists();
        else if (g.scene.lists.freeDirty)
            g.scene.arena.layOutAgain(); /* (not the case this shortcut is for: everything again) */
        if (!g.scene.arena.geometryDirty)
            return;
    }
    pullGeometry();
    if (!g.scene.lists.freeStage.rows)
        ensureHostFreeLists(); /* laid out again from the host images: the lists too, then */
    /* node rows (NodeList: pad records and copies behind them), primitive and light records, start indices, leaf records;
     * then the order-free lists, whole */
    unsigned row = g.scene.walk.layRows(g.scene.exact.layRows(0));
    row = (row + 3u) & ~3u; /* primitive records start on a 64-byte line */
    g.scene.arena.offPrims = row;
    row += (unsigned)g.scene.hostPrims.size();
    g.scene.arena.offLights = row;
    row += (unsigned)g.lights.hostLights.size();
    row = g.scene.walk.layStart(g.scene.exact.layStart(row));
    row = g.scene.walk.layLeaf(g.scene.exact.layLeaf(row));
    g.scene.arena.rowsFixed = row;
    row = g.scene.orderFree.layLeaf(g.scene.orderFree.layStart(g.scene.orderFree.layRows(row)));
    PhaseTimer phase;
    /* the pieces go straight to their rows of the arena (a staged host copy of the whole arena, zero-filled first,
     * took 10-14 ms for 100 k primitives); pad records and the leaf-record area start as zeros */
    reserve(g.scene.arena.geometry, (size_t)std::max(row, 1u) * 16);
    if (!ok())
        return;
    HIPCHECK(hipMemsetAsync(g.scene.arena.geometry.ptr, 0, (size_t)std::max(row, 1u) * 16, sceneStream()));
    auto put = [&](unsigned at, const void *src, size_t bytes) {
        if (bytes && ok())
            HIPCHECK(hipMemcpyAsync((char *)g.scene.arena.geometry.ptr + (size_t)at * 16, src, bytes, hipMemcpyHostToDevice, sceneStream()));
    };
    for (const NodeList *list : {&g.scene.exact, &g.scene.walk, &g.scene.orderFree})
        if (list == &g.scene.orderFree && g.scene.lists.freeStage.rows)
        {
            if (ok())
                copyStagedLists();
        }
        else
        {
            put(list->offRows, list->rows.data(), list->rows.size() * 16);
            put(list->offStart / 4, list->start.data(), list->start.size() * 4);
        }
    put(g.scene.arena.offPrims, g.scene.hostPrims.data(), g.scene.hostPrims.size() * 16);
    put(g.scene.arena.offLights, g.lights.hostLights.data(), g.lights.hostLights.size() * 16);
    HIPCHECK(hipStreamSynchronize(sceneStream())); /* pageable sources: complete for the caller when this returns */
    if (ok())
        g.scene.lists.dropStage(false);
    phase.mark("geometry: upload");
    buildLeafRecords();
    phase.mark("geometry: leaf records");
    if (ok())
        g.scene.arenaFlushed();
}

/* does a list of the arena as it is now hold what it names (k_listEncloses; the host's form of the question is
 * listEnclosesOnHost, list_builders.cpp)?  Waits for the stream */
bool listEnclosesInArena(const NodeList &list)
{
    const int n = (int)list.nodes();
    HIPCHECK(hipSetDevice(g.device));
    reserve(g.scene.refit.enclosesFlag, sizeof(int));
    if (!ok())
        return false;
    int found = 1;
    HIPCHECK(hipMemsetAsync(g.scene.refit.enclosesFlag.ptr, 0, sizeof(int), sceneStream()));
    hipLaunchKernelGGL(k_listEncloses, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sceneStream(),
                       (const float4 *)g.scene.arena.geometry.ptr, list.offRows, list.offStart, g.scene.arena.offPrims, n,
                       (int)(g.scene.hostPrims.size() / PRIM_ROWS), (int *)g.scene.refit.enclosesFlag.ptr);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(&found, g.scene.refit.enclosesFlag.ptr, sizeof(int), hipMemcpyDeviceToHost, sceneStream()));
    HIPCHECK(hipStreamSynchronize(sceneStream()));
    return ok() && found == 0;
}

/* the host builders' parameters (list_builders.h), read once per build */
ListKnobs listKnobs()
{
    ListKnobs knobs;
    if (const char *v = getenv("SOLR_HIP_PRUNE"))
        knobs.pruneThreshold = atof(v);
    if (const char *v = getenv("SOLR_HIP_GROUP_FLAT"))
        knobs.groupFlat = atoi(v);
    if (const char *v = getenv("SOLR_HIP_GROUP_LEVELS"))
        knobs.groupLevels = std::max(atoi(v), 0);
    return knobs;
}

/* pruneInnerNodes' decisions on the device (solr_lists.hip) unless SOLR_HIP_LISTS_ON_HOST says otherwise */
PruneDecider pruneDecider()
{
    if (getenv("SOLR_HIP_LISTS_ON_HOST"))
        return nullptr;
    const hipStream_t stream = sceneStream();
    return [stream](const float4 *rows, int n, double threshold, std::vector<char> &keep) {
        return solrPruneDecisionsOnDevice(rows, n, threshold, keep, stream);
    };
}

/* The scene has been rendered `freeCountdown` times since its upload: build the order-free lists now, from the
 * host images of the reference's list and the primitives as they are (brought up to date first if rotations ran
 * on the device), after checking what their use rests on - every inner node encloses its children, every leaf
 * holds its primitives (the reference's builder makes it so, GPUKernel.cpp:741-830; another host's boxes are
 * taken at their word only after this check; the types whose extent is not what the builder adds around p0 -
 * cones, ellipsoids ... - are sorted out by retagPrimitives). */
void maybeBuildOrderFreeLists()
{
    if (!g.scene.orderFreeDue())
        return;
    if (!g.facts.primsContained)
    {
        g.scene.orderFreeAskAgain();
        return;
    }
    PhaseTimer phase;
    quiesce();
    pullGeometry();
    if (!ok())
        return;
    phase.mark("order-free: host images");
    const std::vector<float4> &rows = g.scene.exact.rows;
    const std::vector<int> &start = g.scene.exact.start;
    const int n = (int)start.size();
    if (n < 2 || rows.size() != 2 * (size_t)n || n > 16000000) /* (beyond that the eight lists pass a dozen GB) */
        return;
    const ListKnobs knobs = listKnobs();
    const bool onHost = getenv("SOLR_HIP_LISTS_ON_HOST") != nullptr;
    /* with the arena laid out as the host images are (the usual case: the scene has been rendered once), the checks
     * and the builder read the exact list and the primitive records there */
    const bool fromArena = !g.scene.arena.geometryDirty && g.scene.arena.geometry.ptr != nullptr && !g.scene.refit.exactStale &&
                           !g.scene.arena.deviceAhead && !onHost;
    const float4 *arena = (const float4 *)g.scene.arena.geometry.ptr;
    const bool encloses = fromArena ? listEnclosesInArena(g.scene.exact) : listEnclosesOnHost(rows, start, g.scene.hostPrims);
    if (!ok())
        return;
    if (!encloses)
    {
        if (getenv("SOLR_HIP_DEBUG_TREE"))
            fprintf(stderr, "solr_hip: no order-free lists: a node does not hold its children or primitives\n");
        return;
    }
    phase.mark("order-free: checks");
    std::vector<int> origin; /* (every node of the exact list is its own origin) */
    auto ownOrigins = [&]() {
        origin.resize(n);
        for (int i = 0; i < n; ++i)
            origin[i] = i;
    };
    int prunedFree = 0;
    /* what the hierarchy is built on (build_bounds.h): the box a long ray tests - a leaf of axis-plane rectangles by its
     * thin box, such leaves set apart where they dominate - unless the variant asks for the boxes as uploaded */
    BuildBounds build;
    if (g.variant != VARIANT_UPLOADED_BUILD_BOXES)
    {
        build.prims = g.scene.hostPrims.data();
        build.margin = g.facts.sceneExtent * (1.f / 1024.f);
    }
    /* on the device (solr_lists.hip: the same tree level by level, the same lists bit for bit) unless told otherwise
     * or declined */
    int count = -1;
    if (!onHost)
    {
        HIPCHECK(hipSetDevice(g.device));
        if (ok() && knobs.pruneThreshold > 0.0)
        {
            g.scene.lists.dropStage(true);
            if (fromArena)
            {
                BuildBounds inArena = build; /* (the primitive records where the rows are) */
                if (build.prims)
                    inArena.prims = arena + g.scene.arena.offPrims;
                count = solrBuildOrderFreeListsOnDevice(arena + g.scene.exact.offRows, (const int *)arena + g.scene.exact.offStart, nullptr, n,
                                                        knobs.pruneThreshold, &prunedFree, sceneStream(), &g.scene.lists.freeStage, inArena);
            }
            else
            {
                ownOrigins();
                count = solrBuildOrderFreeListsOnDevice(rows.data(), start.data(), origin.data(), n, knobs.pruneThreshold, &prunedFree,
                                                        sceneStream(), &g.scene.lists.freeStage, build);
            }
        }
    }
    const bool stayed = count > 0 && g.scene.lists.freeStage.rows != nullptr;
    NodeList built(g.scene.orderFree.copies, g.scene.orderFree.lists);
    if (count < 0)
    {
        if (origin.empty())
            ownOrigins();
        count = buildFreeOrderLists(rows, start, origin, built.rows, built.start, built.origin, &prunedFree, knobs.pruneThreshold,
                                    pruneDecider(), build);
    }
    if (getenv("SOLR_HIP_DEBUG_TREE"))
        fprintf(stderr, "solr_hip: order-free lists: 8 x %d nodes (%d inner nodes that hardly cull left out)\n", count, prunedFree);
    if (count <= 0)
        return;
    phase.mark("order-free: tree, pruning, eight flattenings");
    built.nb = count;
    g.scene.orderFreeBuilt(built, stayed, fromArena); /* (in the arena with the next flushGeometry) */
}

/* ---- which short cuts a walk is offered: the four predicates, each with what it rests on ---------------------------- */
/* the order-free lists exist for the resident scene and every condition of their use holds (rt_device.h closestHitWalk) */
bool orderFreeListsUsable()
{
    return g.scene.orderFree.nb > 0 && g.facts.primsContained && !g.scene.lists.freeStale && g.scene.nested && g.scene.walk.ordered &&
           g.variant != VARIANT_NO_ORDER_FREE;
}

/* shadow walks in the reference's order may leave out the boxes that begin beyond the lamp (rt_device.h shadowWalk,
 * lampCut): the walk-order list is nested and ordered, it holds what it names (checked where it was built or last
 * refitted; its thin copy is made from it, leaves cut out of its leaves, inner nodes their unions), and no primitive
 * reaches beyond what the check takes for its extent (retagPrimitives) */
bool lampCutoffUsable()
{
    return g.scene.walkEncloses && g.facts.primsContained && g.scene.nested && g.scene.walk.ordered && g.variant != VARIANT_NO_LAMP_CUTOFF;
}

/* may the walks of a frame with this SceneInfo take the thin copies of the lists S names (rt_device.h tightRay)?  A thin
 * leaf is its planes' rectangle CUT WITH THE BOX AS UPLOADED, and the reference never asks a hit to lie inside its leaf's
 * box, only the ray to enter it: through a box smaller than its plane's rectangle a ray can hit the plane beside the box -
 * the reference finds that hit, the copy does not.  So only for a list that holds what it names (walkEncloses: checked at
 * h2d_scene and after every rotation on the device; the order-free lists exist only behind the same check of the
 * reference's list) - the reference's builder makes no other, another host's boxes are taken at their word only after it. */
static int tightListsFor(const SceneArgs &S, const SceneInfo &sceneInfo, bool exactNodes)
{
    if (exactNodes || g.variant == VARIANT_REFERENCE_LEAVES || !g.scene.walk.tight || !g.scene.walkEncloses || !sceneInfo.extendedGeometry)
        return 0;
    if (S.nbBoxesFree > 0 && !g.scene.orderFree.tight)
        return 0;
    return (sceneInfo.viewDistance > 0.f && sceneInfo.viewDistance <= 64.f * g.facts.sceneExtent) ? 1 : 0;
}

/* ... and the copies of the order-free lists with sorted bounds behind those, where a frame walks these lists at all
 * (nbBoxesFree: makeScene's answer from orderFreeListsUsable): made with the lists' other copies wherever their bounds
 * change (deriveList).  VARIANT_UNSORTED_LISTS: the walks take the lists as they are */
static bool sortedListsUsable(int nbBoxesFree)
{
    return nbBoxesFree > 0 && g.scene.lists.sortedFree && g.variant != VARIANT_UNSORTED_LISTS;
}

/* bounce rays on the order-free lists: the API's word, else SOLR_HIP_SHORT_RAY_LISTS=0|1 (experiments), else the engine's
 * own choice for this frame */
bool shortRayListsChoice()
{
    static const int fromEnv = getenv("SOLR_HIP_SHORT_RAY_LISTS") ? atoi(getenv("SOLR_HIP_SHORT_RAY_LISTS")) : -1;
    const int mode = g.shortRayListsMode >= 0 ? g.shortRayListsMode : fromEnv;
    /* The engine's own choice.  Bounce rays on the order-free lists save work in nearly every tile and add some to the
     * few whose lanes have to be walked again (the mesh's horizon tiles: + 13 %).  With frames in flight the next frame
     * fills the chip behind those tiles and the saving is what shows (the mesh delivered 0.368 -> 0.356 ms, a 136-row
     * frame of it 0.239 -> 0.222); one frame at a time is as long as its longest tile and gets longer (0.43 -> 0.48 ms). */
    return mode < 0 ? activeFlights() >= 2 : mode != 0;
}

static SceneArgs makeScene(bool exactNodes)
{
    const NodeList &list = exactNodes ? g.scene.exact : g.scene.walk;
    SceneArgs S;
    memset(&S, 0, sizeof(S));
    S.geometry = g.scene.arena.geometry.ptr;
    S.materials = g.materials.table.ptr;
    S.textures = g.textures.atlas.ptr;
    S.randoms = g.randoms.values.ptr;
    S.offBoxes = list.offRows;
    S.offBoxStart = list.offStart;
    S.offLeaf = list.offLeaf;
    S.offPrims = g.scene.arena.offPrims;
    S.offLights = g.scene.arena.offLights;
    S.offMatCold = g.materials.offMatCold;
    S.nbBoxes = list.nb;
    S.nbPrimitives = g.scene.nbPrimitives;
    S.nbLights = g.lights.nbLights;
    S.nbLamps = g.scene.nbLamps;
    S.nested = g.scene.nested;
    S.orderedBoxes = list.ordered;
    S.nbRandoms = g.randoms.values.ptr ? g.randoms.nbRandoms : 0;
    if (!exactNodes && orderFreeListsUsable())
    {
        S.offBoxesFree = g.scene.orderFree.offRows;
        S.offLeafFree = g.scene.orderFree.offLeaf;
        S.nbBoxesFree = g.scene.orderFree.nb; /* per list; the eight lists and their leaf records lie one behind the other */
        S.opaqueShadows = g.facts.opaqueShadows ? SHADOWS_OPAQUE : 0;
        S.shortRayLists = shortRayListsChoice() ? 1 : 0;
    }
    if (!exactNodes && lampCutoffUsable())
        S.opaqueShadows |= SHADOWS_LAMP_CUTOFF;
    if (g.variant == VARIANT_ALL_TRIPS)
        S.opaqueShadows |= SHADOWS_ALL_TRIPS;
    /* the thin copies behind the lists this frame walks (set by tightListsFor: they also depend on the frame) */
    S.tightLists = 0;
    S.sortedLists = sortedListsUsable(S.nbBoxesFree) ? 1 : 0;
    return S;
}

/* The resident scene as a frame with this SceneInfo walks it (renderImpl; the probes, solrprobe::residentScene): pending
 * uploads flushed, the order-free lists built when they are due, the reference's own node list refitted when it is the
 * one wanted (exactNodes).  A failure is the engine's error (ok()). */
SceneArgs prepareScene(const SceneInfo &sceneInfo, bool exactNodes)
{
    maybeBuildOrderFreeLists();
    flushGeometry();
    if (exactNodes)
        refreshExactList();
    if (!ok())
        return SceneArgs();
    SceneArgs S = makeScene(exactNodes);
    S.tightLists = tightListsFor(S, sceneInfo, exactNodes);
    /* the thin boxes of sphere leaves are made for a reach: a frame with another one (its viewDistance beyond the scene's
     * extent, VARIANT_UPLOADED_SPHERE_LEAVES set or taken back) has them made again before it walks them */
    g.facts.frameViewDistance = sceneInfo.viewDistance;
    if (S.tightLists && thinReachWanted(sceneInfo.viewDistance) != g.facts.thinReach)
    {
        quiesce();
        g.facts.thinReach = thinReachWanted(sceneInfo.viewDistance);
        tightenListsAgain();
        if (!ok())
            return SceneArgs();
    }
    return S;
}

/* a list of more than a thousand nodes does not live in the scalar cache: skips land on cold records, and the walks take
 * the three-bank node loop (F_DEEP) */
bool deepNodeList(const SceneArgs &S)
{
    return S.nbBoxes > 1024;
}

} // namespace solreng
