/*
 * solr_rotation.hip - animated scenes of the MI355X rendering engine: solr_hip_rotate_primitives rotates the resident
 * primitives and refits the node lists in the arena (engine.h Refit: the plan and the flags, Scene::requestServed: what a
 * served request changes, Engine::served: the counters; the arena: solr_arena.hip).
 * Part of the engine's host side (engine.h); the boundary that calls into it is solr_hip.hip.  gfx950 only.
 */
#include <hip/hip_runtime.h>

#include "../../include/solr_hip.h"
#include "rt_device.h"

using namespace solrdev;

#include "renderer.h"
#include "engine.h"

using namespace solreng;

namespace solreng
{
/* ---- animated scenes: rotate + refit on the device ---------------------------------------------------
 * The reference animates a scene by GPUKernel::rotatePrimitives + compactBoxes(false) on the host and a
 * full upload, every frame (MoleculeScene.cpp:75-81; GPUKernel.cpp:1378-1460 rotates the primitives of
 * the level-0 boxes and refits every level, :1151-1281 flattens again).  The flattened tree keeps its
 * shape under that - only primitive coordinates and node bounds change - so the same arithmetic runs
 * here on the resident arena instead: the primitive rows in place, then the nodes bottom-up.  Every
 * expression below is the host builder's (sol-r_amd/host/GPUKernel.cpp rotateVector, updateBoundingBox,
 * updateOutterBoundingBox), in its order and with its comparisons, so that the arena afterwards holds
 * bit for bit what a host rotation followed by a fresh upload would have put there. */
struct RotationArgs
{
    float cx, cy, cz;
    float cosx, cosy, cosz;
    float sinx, siny, sinz;
};

__device__ inline void rotateRow(float4 &v, float cx, float cy, float cz, const RotationArgs &R)
{
    float vx = v.x - cx, vy = v.y - cy, vz = v.z - cz;
    float ry = vy * R.cosx - vz * R.sinx;
    float rz = vy * R.sinx + vz * R.cosx;
    vy = ry;
    vz = rz;
    rz = vz * R.cosy - vx * R.siny;
    float rx = vz * R.siny + vx * R.cosy;
    vz = rz;
    vx = rx;
    rx = vx * R.cosz - vy * R.sinz;
    ry = vx * R.sinz + vy * R.cosz;
    v.x = rx + cx;
    v.y = ry + cy;
    v.z = rz + cz;
}

__global__ __launch_bounds__(256) void k_rotatePrimitives(float4 *__restrict__ arena, unsigned offPrims, int nbPrimitives,
                                                          const unsigned char *__restrict__ movable,
                                                          const RotationArgs R)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nbPrimitives || !movable[i])
        return;
    float4 *r = arena + offPrims + (size_t)PRIM_ROWS * i;
    float4 p0 = r[ROW_P0_TYPE];
    const int type = __float_as_int(p0.w) & PRIM_TYPE_MASK;
    rotateRow(p0, R.cx, R.cy, R.cz, R);
    r[ROW_P0_TYPE] = p0;
    if (type == ptCylinder || type == ptTriangle)
    {
        float4 p1 = r[ROW_P1_INDEX], p2 = r[ROW_P2], n0 = r[ROW_N0], n1 = r[ROW_N1], n2 = r[ROW_N2];
        rotateRow(p1, R.cx, R.cy, R.cz, R);
        rotateRow(p2, R.cx, R.cy, R.cz, R);
        rotateRow(n0, 0.f, 0.f, 0.f, R);
        rotateRow(n1, 0.f, 0.f, 0.f, R);
        rotateRow(n2, 0.f, 0.f, 0.f, R);
        if (type == ptCylinder)
        {
            float ax = p1.x - p0.x, ay = p1.y - p0.y, az = p1.z - p0.z;
            const float len = __builtin_sqrtf(ax * ax + ay * ay + az * az);
            if (len != 0)
            {
                ax /= len;
                ay /= len;
                az /= len;
            }
            n1.x = ax;
            n1.y = ay;
            n1.z = az;
        }
        r[ROW_P1_INDEX] = p1;
        r[ROW_P2] = p2;
        r[ROW_N0] = n0;
        r[ROW_N1] = n1;
        r[ROW_N2] = n2;
    }
}

/* One node per thread, the nodes of one height of the tree per launch (children first).  A node with
 * primitives is a level-0 box: updateBoundingBox; one without is the union of its children:
 * updateOutterBoundingBox, seeded like it (+-viewDistance; +-infinity for our own grouping nodes, which
 * the list marks with the sign bit). */
__global__ __launch_bounds__(256) void k_refitNodes(float4 *__restrict__ arena, unsigned offNodes, unsigned offStart,
                                                    unsigned offPrims, const int *__restrict__ list, int count,
                                                    float seed)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count)
        return;
    const int entry = list[t];
    const int node = entry & 0x7fffffff;
    if (entry < 0)
        seed = INFINITY; /* one of our own grouping nodes: the plain union */
    float4 *rows = arena + offNodes;
    const float4 row1 = rows[2 * node + 1];
    const int nb = __float_as_int(row1.z);
    const int skip = __float_as_int(row1.w);
    float lx, ly, lz, hx, hy, hz;
    if (nb > 0)
    {
        const int first = ((const int *)arena)[offStart + node];
        lx = ly = lz = 1000000.f;
        hx = hy = hz = -1000000.f;
        for (int k = 0; k < nb; ++k)
        {
            const float4 *r = arena + offPrims + (size_t)PRIM_ROWS * (first + k);
            const float4 p0 = r[ROW_P0_TYPE];
            const float4 size = r[ROW_SIZE_MAT];
            const int type = __float_as_int(p0.w) & PRIM_TYPE_MASK;
            /* std::min(a, b) is (b < a) ? b : a and std::max(a, b) is (a < b) ? b : a: kept as such, the
             * sign of a zero that ties depends on it */
            float c0x = p0.x, c0y = p0.y, c0z = p0.z, c1x = p0.x, c1y = p0.y, c1z = p0.z;
            if (type == ptTriangle || type == ptCylinder)
            {
                const float4 p1 = r[ROW_P1_INDEX];
                c0x = (p1.x < p0.x) ? p1.x : p0.x;
                c0y = (p1.y < p0.y) ? p1.y : p0.y;
                c0z = (p1.z < p0.z) ? p1.z : p0.z;
                c1x = (p0.x < p1.x) ? p1.x : p0.x;
                c1y = (p0.y < p1.y) ? p1.y : p0.y;
                c1z = (p0.z < p1.z) ? p1.z : p0.z;
                if (type == ptTriangle)
                {
                    const float4 p2 = r[ROW_P2];
                    c0x = (p2.x < c0x) ? p2.x : c0x;
                    c0y = (p2.y < c0y) ? p2.y : c0y;
                    c0z = (p2.z < c0z) ? p2.z : c0z;
                    c1x = (c1x < p2.x) ? p2.x : c1x;
                    c1y = (c1y < p2.y) ? p2.y : c1y;
                    c1z = (c1z < p2.z) ? p2.z : c1z;
                }
            }
            float ax = (c1x < c0x) ? c1x : c0x, ay = (c1y < c0y) ? c1y : c0y, az = (c1z < c0z) ? c1z : c0z;
            float bx = (c0x > c1x) ? c0x : c1x, by = (c0y > c1y) ? c0y : c1y, bz = (c0z > c1z) ? c0z : c1z;
            const bool round = type == ptCylinder || type == ptSphere || type == ptCone;
            const float sy = round ? size.x : size.y, sz = round ? size.x : size.z;
            ax -= size.x;
            ay -= sy;
            az -= sz;
            bx += size.x;
            by += sy;
            bz += sz;
            if (ax < lx) lx = ax;
            if (ay < ly) ly = ay;
            if (az < lz) lz = az;
            if (bx > hx) hx = bx;
            if (by > hy) hy = by;
            if (bz > hz) hz = bz;
        }
    }
    else
    {
        lx = ly = lz = seed;
        hx = hy = hz = -seed;
        for (int c = node + 1; c < node + skip;)
        {
            const float4 a = rows[2 * c], b = rows[2 * c + 1];
            if (lx > a.x) lx = a.x;
            if (ly > a.y) ly = a.y;
            if (lz > a.z) lz = a.z;
            if (hx < b.x) hx = b.x;
            if (hy < b.y) hy = b.y;
            if (hz < a.w) hz = a.w;
            const int s = __float_as_int(b.w);
            c += (s > 1) ? s : 1;
        }
    }
    rows[2 * node] = make_float4(lx, ly, lz, hz);
    rows[2 * node + 1] = make_float4(hx, hy, row1.z, row1.w);
}

/* What solr_hip_rotate_primitives refits and in which order: the nodes of a list by height, children
 * before parents.  A frame walks the walk-order list, so that is the one refitted with every rotation; the
 * reference's own list (box-debug view, census, VARIANT_EXACT_LIST, read-back) follows when somebody needs it
 * (refreshExactList) - node bounds are a function of the primitives alone, so late is as good as at once.
 * Both give a node of the reference's tree the same bounds: min / max over the level-0 boxes below it,
 * clamped once or several times by the same +-viewDistance seed, first occurrence winning a tie in either
 * nesting.  Node 0, the light cell, keeps its +-viewDistance (GPUKernel.cpp:1189). */
static void buildRefitPlan()
{
    g.scene.refit.refitPlanPending = false;
    g.scene.refit.refitReady = false;
    g.scene.refit.exactStale = false;
    for (NodeList *list : {&g.scene.exact, &g.scene.walk, &g.scene.orderFree})
        list->refitLevels.clear();
    if (!g.scene.nested)
        return;
    std::vector<int> plan;
    planRefit(g.scene.exact.rows, g.scene.walk.rows, g.scene.walk.origin, g.scene.orderFree.rows, g.scene.orderFree.origin, plan,
              g.scene.exact.refitLevels, g.scene.walk.refitLevels, g.scene.orderFree.refitLevels);
    upload(g.scene.refit.refitPlan, plan);
    g.scene.refit.refitReady = ok();
}

static void refitList(const NodeList &list, float viewDistance)
{
    float4 *arena = (float4 *)g.scene.arena.geometry.ptr;
    const int *plan = (const int *)g.scene.refit.refitPlan.ptr;
    const std::vector<int> &levels = list.refitLevels;
    for (size_t l = 0; l + 1 < levels.size(); l += 2)
        hipLaunchKernelGGL(k_refitNodes, dim3((unsigned)((levels[l + 1] + 255) / 256)), dim3(256), 0, sceneStream(), arena,
                           list.offRows, list.offStart, g.scene.arena.offPrims, plan + levels[l], levels[l + 1], viewDistance);
}

/* the reference's node list is wanted: refit it from the primitives as they are now */
void refreshExactList()
{
    if (!g.scene.refit.exactStale || !g.scene.arena.geometry.ptr)
        return;
    quiesce();
    refitList(g.scene.exact, g.scene.refit.exactStaleViewDistance);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(sceneStream()));
    g.scene.exactRefitted();
}

/* A kernel that moves the resident primitives (k_rotatePrimitives; solr_morph.hip k_morphPrimitives) is queued on the scene
 * stream: what follows it, for a rotation and a morph alike - the refit of the walk-order list and, where they can follow, of
 * the order-free lists, the reference's list marked stale, the leaf records and the copies behind the lists, the enclosure
 * check, one synchronisation of the scene stream.  Returns whether the walk-order list still holds what it names. */
bool refitMovedScene(float viewDistance)
{
    refitList(g.scene.walk, viewDistance);
    const bool listsFollow = g.scene.orderFree.nb > 0 && !g.scene.orderFree.refitLevels.empty();
    if (listsFollow)
        refitList(g.scene.orderFree, viewDistance);
    g.scene.refitQueued(listsFollow, viewDistance);
    buildLeafRecords(); /* the leaves' copies of their first primitive follow the primitives */
    /* the refitted list encloses by construction (k_refitNodes); asked all the same, like any list the walks cut off at
     * the lamp (a scene that failed the check at its upload is not asked again) */
    const bool walkHolds = g.scene.walkEncloses && listEnclosesInArena(g.scene.walk);
    HIPCHECK(hipGetLastError());
    /* the other flights' streams start their next frame only after this */
    HIPCHECK(hipStreamSynchronize(sceneStream()));
    return walkHolds;
}

/* can this engine move primitives of its resident scene and refit the lists behind them?  What a rotation, a translation,
 * an edit and a morph all ask first.  (Makes the refit plan when the lists changed; changes nothing else.) */
bool canRefitOne(float viewDistance, const char *who)
{
    if (!ready(who))
        return false;
    if (g.scene.refit.refitPlanPending)
    {
        /* which nodes to refit, in which order: made for the first request after the lists changed */
        ensureHostFreeLists();
        buildRefitPlan();
    }
    /* the seeds of the two box updates only commute with the unions while viewDistance <= 1e6, and a
     * tree cut off at NB_MAX_BOXES has host-side children the flattened list does not show */
    if (!g.scene.refit.refitReady || g.scene.refit.nbMovable != g.scene.nbPrimitives || g.scene.nbPrimitives <= 0 ||
        !(viewDistance <= 1000000.f) || !(viewDistance > 0.f) || g.scene.exact.nb >= NB_MAX_BOXES)
    {
        noteRefusal(who, "plan %d, flags for %d of %d primitives, viewDistance %g, %d nodes", (int)g.scene.refit.refitReady,
                    g.scene.refit.nbMovable, g.scene.nbPrimitives, viewDistance, g.scene.exact.nb);
        return false;
    }
    return true;
}

/* can this engine rotate its resident scene?  (canRefitOne, and the rotation's own three arrays) */
bool canRotateOne(const float center[3], const float cosAngles[3], const float sinAngles[3], float viewDistance)
{
    if (!canRefitOne(viewDistance, "solr_hip_rotate_primitives"))
        return false;
    if (!center || !cosAngles || !sinAngles)
    {
        noteRefusal("solr_hip_rotate_primitives", "no centre, cosines or sines");
        return false;
    }
    return true;
}

/* Extension: GPUKernel::rotatePrimitives + compactBoxes(false) + h2d_scene on the resident scene
 * (GPUKernel.cpp:1378-1460, 1151-1281 of the reference), see k_rotatePrimitives.  Returns 1 when the
 * arena now holds the rotated scene, 0 when the request cannot be served here and the caller has to
 * take the host route (nothing was changed). */
int rotatePrimitivesOne(const float center[3], const float cosAngles[3], const float sinAngles[3], float viewDistance)
{
    if (!canRotateOne(center, cosAngles, sinAngles, viewDistance) || !beginRequest())
        return 0;
    RotationArgs R;
    R.cx = center[0], R.cy = center[1], R.cz = center[2];
    R.cosx = cosAngles[0], R.cosy = cosAngles[1], R.cosz = cosAngles[2];
    R.sinx = sinAngles[0], R.siny = sinAngles[1], R.sinz = sinAngles[2];
    hipLaunchKernelGGL(k_rotatePrimitives, dim3((unsigned)((g.scene.nbPrimitives + 255) / 256)), dim3(256), 0, sceneStream(),
                       (float4 *)g.scene.arena.geometry.ptr, g.scene.arena.offPrims, g.scene.nbPrimitives,
                       (const unsigned char *)g.scene.refit.movable.ptr, R);
    return finishRequest(REQUEST_ROTATION, refitMovedScene(viewDistance));
}

} // namespace solreng

extern "C" {
int solr_hip_device_rotations(void)
{
    return g.served[REQUEST_ROTATION];
}
} // extern "C"
