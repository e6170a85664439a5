/*
 * solr_moves.hip - the rigid moves of the MI355X rendering engine besides the rotation: solr_hip_translate_primitives pushes
 * the resident primitives along and refits the node lists in the arena (the refit and what follows it: solr_rotation.hip
 * refitMovedScene), solr_hip_move_lamp sets a lamp's centre and its light record in place (engine.h RequestKind and
 * Scene::requestServed: what either changes in the scene's record; Engine::served: the counters), solr_hip_read_lights hands
 * the resident light records to the tests.
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
/* ---- models that are pushed along: translate + refit on the device -----------------------------------
 * The reference moves a model by GPUKernel::translatePrimitives + compactBoxes(false) on the host and a full upload
 * (GPUKernel.cpp:1462-1511: p0, p1 and p2 of the primitives of the level-0 boxes incremented, every level refitted;
 * apps/scenes/Scene.cpp:1546-1548 runs it behind a rotation).  Like a rotation it leaves the flattened tree in shape, so
 * the same three additions a point run here on the resident arena - binary32, nothing to contract - and the nodes follow
 * bottom-up through the rotation's refit.  Sizes, normals and the fourth words of the rows stay, as in the host loop
 * (sol-r_amd/host/GPUKernel.cpp translatePrimitivesOnly), whatever the primitive's type. */
__device__ inline void translateRow(float4 &v, float tx, float ty, float tz)
{
    v.x = v.x + tx;
    v.y = v.y + ty;
    v.z = v.z + tz;
}

__global__ __launch_bounds__(256) void k_translatePrimitives(float4 *__restrict__ arena, unsigned offPrims, int nbPrimitives,
                                                             const unsigned char *__restrict__ movable, float tx, float ty,
                                                             float tz)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nbPrimitives || !movable[i])
        return;
    float4 *r = arena + offPrims + (size_t)PRIM_ROWS * i;
    float4 p0 = r[ROW_P0_TYPE], p1 = r[ROW_P1_INDEX], p2 = r[ROW_P2];
    translateRow(p0, tx, ty, tz);
    translateRow(p1, tx, ty, tz);
    translateRow(p2, tx, ty, tz);
    r[ROW_P0_TYPE] = p0;
    r[ROW_P1_INDEX] = p1;
    r[ROW_P2] = p2;
}

/* can this engine translate its resident scene?  (canRefitOne, and a translation of three numbers; changes nothing but
 * the refit plan) */
bool canTranslateOne(const float translation[3], float viewDistance)
{
    if (!canRefitOne(viewDistance, "solr_hip_translate_primitives"))
        return false;
    if (!translation || !std::isfinite(translation[0]) || !std::isfinite(translation[1]) || !std::isfinite(translation[2]))
    {
        noteRefusal("solr_hip_translate_primitives", "no translation, or a component that is not finite");
        return false;
    }
    return true;
}

/* Extension: GPUKernel::translatePrimitives + compactBoxes(false) + h2d_scene on the resident scene, see
 * k_translatePrimitives.  Returns 1 when the arena now holds the translated scene, 0 when the request cannot be served here
 * and the caller has to take the host route (nothing was changed). */
int translatePrimitivesOne(const float translation[3], float viewDistance)
{
    if (!canTranslateOne(translation, viewDistance) || !beginRequest())
        return 0;
    hipLaunchKernelGGL(k_translatePrimitives, dim3((unsigned)((g.scene.nbPrimitives + 255) / 256)), dim3(256), 0, sceneStream(),
                       (float4 *)g.scene.arena.geometry.ptr, g.scene.arena.offPrims, g.scene.nbPrimitives,
                       (const unsigned char *)g.scene.refit.movable.ptr, translation[0], translation[1], translation[2]);
    return finishRequest(REQUEST_TRANSLATION, refitMovedScene(viewDistance));
}

/* ---- a lamp that is dragged: its centre and its light record in place ----------------------------------
 * The reference's viewer drags a lamp with setPrimitiveCenter + compactBoxes(false) per mouse event (apps/solrViewer.cpp:
 * 1058-1069, 1111-1123; apps/scenes/science/SwcScene.cpp:84-87).  compactBoxes(false) refits nothing, and the lamps sit in the
 * first box of the top level, whose flattened node is pinned to +-viewDistance (GPUKernel.cpp:1183-1188): of everything that
 * is uploaded, the move changes the p0 of one primitive and the location of one light record (:1218-1220).  Here those two
 * are written in the arena, and with them what the engine derives from that p0 and keeps elsewhere - the leaf records of the
 * leaves whose first primitive the lamp is (k_buildLeafRecords: record 0 is the primitive's first row), the host images. */
struct LampMove
{
    LeafRecordsOf list[3]; /* (engine.h) */
    unsigned offPrims, offLights;
    int lamp;
    float x, y, z;
};

/* One thread per node of the lists, one list behind the other; the first thread also sets the primitive's and the light
 * record's centre (nobody here reads either).  The fourth words - the primitive's tag, the light's primitive id - stay. */
__global__ __launch_bounds__(256) void k_moveLamp(float4 *__restrict__ arena, const LampMove M)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0)
    {
        float4 *p0 = arena + M.offPrims + (size_t)PRIM_ROWS * M.lamp + ROW_P0_TYPE;
        float4 *location = arena + M.offLights + 3u * (unsigned)M.lamp;
        p0->x = M.x, p0->y = M.y, p0->z = M.z;
        location->x = M.x, location->y = M.y, location->z = M.z;
    }
    for (int l = 0; l < 3; ++l)
    {
        const LeafRecordsOf &L = M.list[l];
        if (t < L.nodes)
        {
            const int nb = __float_as_int(arena[L.offRows + 2u * (unsigned)t + 1u].z);
            if (nb > 0 && ((const int *)arena)[L.offStart + (unsigned)t] == M.lamp)
            {
                float4 *record = arena + L.offLeaf + 4u * (unsigned)t;
                record->x = M.x, record->y = M.y, record->z = M.z;
            }
            return;
        }
        t -= L.nodes;
    }
}

/* can this engine move that lamp of its resident scene there?  (changes nothing) */
bool canMoveLampOne(int lamp, const float center[3])
{
    if (!g.initialized || !ok())
        return false;
    const Scene &s = g.scene;
    const char *why = nullptr;
    if (s.nbPrimitives <= 0 || s.hostPrims.size() < (size_t)PRIM_ROWS * (size_t)s.nbPrimitives || s.exact.nb <= 0 || s.exact.start.empty() ||
        s.exact.rows.size() < 2)
        why = "no resident scene";
    else if (lamp < 0 || lamp >= s.nbLamps || lamp >= s.nbPrimitives)
        why = "no such lamp";
    else if (!center || !std::isfinite(center[0]) || !std::isfinite(center[1]) || !std::isfinite(center[2]))
        why = "no centre, or a component that is not finite";
    else if (g.lights.nbLights < s.nbLamps || g.lights.hostLights.size() < 3 * (size_t)s.nbLamps ||
             bitsi(g.lights.hostLights[3 * (size_t)lamp].w) != bitsi(s.hostPrims[(size_t)PRIM_ROWS * lamp + ROW_P1_INDEX].w))
        why = "the light records are not the lamps'";
    else
    {
        /* the lamp has to stay inside its leaf (lampCutoffUsable, tightListsFor: the facts are not derived again): the first
         * node - the lamps' cell, which no refit touches, so its host image is what the arena holds - by the extent
         * k_listEncloses takes for a sphere.  A lamp of another cell is the host's, and so is one of another type: an axis
         * plane's p0 reaches the thin copies of the lists through another clause (tightenList: a leaf of plain axis planes
         * becomes their rectangles); a sphere's does too, and moveLampOne has the copies made again (tightenListsAgain) */
        const float4 a = s.exact.rows[0], b = s.exact.rows[1];
        const float grow = fabsf(s.hostPrims[(size_t)PRIM_ROWS * lamp + ROW_SIZE_MAT].x);
        const int type = bitsi(s.hostPrims[(size_t)PRIM_ROWS * lamp + ROW_P0_TYPE].w) & PRIM_TYPE_MASK;
        if (s.exact.start[0] > lamp || (long)s.exact.start[0] + bitsi(b.z) <= lamp || type != ptSphere)
            why = "not a sphere of the first cell";
        else if (!(a.x <= center[0] - grow && a.y <= center[1] - grow && a.z <= center[2] - grow && b.x >= center[0] + grow &&
                   b.y >= center[1] + grow && a.w >= center[2] + grow))
            why = "the lamp would leave its cell";
    }
    if (why)
        noteRefusal("solr_hip_move_lamp", "%s (lamp %d of %d, %d light records)", why, lamp, s.nbLamps, g.lights.nbLights);
    return why == nullptr;
}

/* Extension: GPUKernel::setPrimitiveCenter on a lamp + compactBoxes(false) + h2d_scene + h2d_lightInformation on the resident
 * scene, see k_moveLamp.  Returns 1 when the arena and the host images now hold the lamp there, 0 when the request cannot be
 * served here and the caller has to take the host route (nothing was changed). */
int moveLampOne(int lamp, const float center[3])
{
    if (!canMoveLampOne(lamp, center) || !beginRequest()) /* (no frame in flight reads a lamp that is half here and half there) */
        return 0;
    LampMove M;
    const int total = 1 + leafRecordsOfLists(g.scene, M.list);
    M.offPrims = g.scene.arena.offPrims;
    M.offLights = g.scene.arena.offLights;
    M.lamp = lamp;
    M.x = center[0], M.y = center[1], M.z = center[2];
    hipLaunchKernelGGL(k_moveLamp, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, sceneStream(), (float4 *)g.scene.arena.geometry.ptr, M);
    HIPCHECK(hipGetLastError());
    /* the lamps' cell is refitted by nobody, but its box in the thin copies is its spheres' (build_bounds.h): made again
     * from the centre as it is now, on the same stream; the other flights' streams start their next frame only after this */
    tightenListsAgain();
    HIPCHECK(hipStreamSynchronize(sceneStream()));
    if (ok())
    {
        float4 &p0 = g.scene.hostPrims[(size_t)PRIM_ROWS * lamp + ROW_P0_TYPE], &location = g.lights.hostLights[3 * (size_t)lamp];
        p0.x = location.x = center[0];
        p0.y = location.y = center[1];
        p0.z = location.z = center[2];
    }
    return finishRequest(REQUEST_LAMP_MOVE);
}

} // namespace solreng

extern "C" {
int solr_hip_device_translations(void)
{
    return g.served[REQUEST_TRANSLATION];
}

int solr_hip_device_lamp_moves(void)
{
    return g.served[REQUEST_LAMP_MOVE];
}

/* Diagnostics / tests: the resident arena's light records as the device holds them now, three float4 rows a light.
 * Returns the number of rows written, with rows == NULL only that; -1 if the capacity is too small. */
int solr_hip_read_lights(float *rows, int capacityRows)
{
    if (!ready("solr_hip_read_lights") || !g.scene.arena.geometry.ptr)
        return -1;
    flushGeometry();
    quiesce();
    const int n = (int)g.lights.hostLights.size();
    if (!rows)
        return n;
    if (n > capacityRows)
        return -1;
    if (n)
        HIPCHECK(hipMemcpy(rows, (const char *)g.scene.arena.geometry.ptr + (size_t)g.scene.arena.offLights * 16, (size_t)n * 16,
                           hipMemcpyDeviceToHost));
    return ok() ? n : -1;
}
} // extern "C"
