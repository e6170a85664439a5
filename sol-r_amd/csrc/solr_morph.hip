/*
 * solr_morph.hip - key-frame morphing of the MI355X rendering engine: solr_hip_set_morph_keys hands over the two key
 * frames of the resident scene, solr_hip_morph_primitives blends them into the resident primitives at any weight and
 * refits the node lists in the arena (engine.h Morph; the refit and what follows it: solr_rotation.hip refitMovedScene).
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
/* ---- deforming scenes: blend two key frames + refit on the device ------------------------------------
 * The reference makes the frames between two key frames on the host (GPUKernel::morphPrimitives, GPUKernel.cpp:1513-1572:
 * every primitive set anew from `first + r * (last - first)`, a tree per frame) and shows them by switching frames and
 * flattening again.  The flattened tree of such a frame keeps its shape when the same frame is blended at another weight -
 * only primitive coordinates and node bounds change - so the blend runs here on the resident arena: the primitive rows in
 * place, then the nodes bottom-up like after a rotation.  Every expression below is the host loop's (sol-r_amd/host/
 * GPUKernel.cpp morphFrame: the reference's mix, setPrimitive, setPrimitiveNormals with normalizeVector), in its order,
 * binary32 without contraction, so that the arena afterwards holds bit for bit what that loop followed by a fresh upload
 * would have put there (h2d_scene copies the geometry words as they are, solr_uploads.hip).
 *
 * The keys: per key frame seven planes of nbPrimitives float4 (MORPH_KEY_*; .w unused), primitives in the flattened order of
 * the resident scene - lane i of a wave reads the 16 bytes next to lane i - 1's. */
enum MorphKeyRow
{
    MORPH_KEY_P0 = 0,
    MORPH_KEY_P1,
    MORPH_KEY_P2,
    MORPH_KEY_N0,
    MORPH_KEY_N1,
    MORPH_KEY_N2,
    MORPH_KEY_SIZE,
    MORPH_KEY_ROWS
};

struct Vec3
{
    float x, y, z;
};

/* primitive1.c + r * (primitive2.c - primitive1.c), component by component (GPUKernel.cpp:1530-1557) */
__device__ inline Vec3 mixKeys(const float4 &a, const float4 &b, float r)
{
    Vec3 v;
    v.x = a.x + r * (b.x - a.x);
    v.y = a.y + r * (b.y - a.y);
    v.z = a.z + r * (b.z - a.z);
    return v;
}

/* GPUKernel::normalizeVector: division by the length, a zero vector left alone */
__device__ inline void normalizeVec3(Vec3 &v)
{
    const float l = __builtin_sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
    if (l != 0.f)
    {
        v.x /= l;
        v.y /= l;
        v.z /= l;
    }
}

/* the geometry words of a row; the fourth word (tag, material id, index, colour key, texture coordinates) stays */
__device__ inline void storeXyz(float4 *row, const Vec3 &v)
{
    row->x = v.x;
    row->y = v.y;
    row->z = v.z;
}

__global__ __launch_bounds__(256) void k_morphPrimitives(float4 *__restrict__ arena, unsigned offPrims, int nbPrimitives,
                                                         const float4 *__restrict__ first, const float4 *__restrict__ last,
                                                         float r)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nbPrimitives)
        return;
    const size_t plane = (size_t)nbPrimitives;
    float4 *rows = arena + offPrims + (size_t)PRIM_ROWS * i;
    const int type = __float_as_int(rows[ROW_P0_TYPE].w) & PRIM_TYPE_MASK;
    const Vec3 p0 = mixKeys(first[MORPH_KEY_P0 * plane + i], last[MORPH_KEY_P0 * plane + i], r);
    const Vec3 p1 = mixKeys(first[MORPH_KEY_P1 * plane + i], last[MORPH_KEY_P1 * plane + i], r);
    Vec3 p2 = mixKeys(first[MORPH_KEY_P2 * plane + i], last[MORPH_KEY_P2 * plane + i], r);
    Vec3 size = mixKeys(first[MORPH_KEY_SIZE * plane + i], last[MORPH_KEY_SIZE * plane + i], r);
    Vec3 n0 = mixKeys(first[MORPH_KEY_N0 * plane + i], last[MORPH_KEY_N0 * plane + i], r);
    Vec3 n1 = mixKeys(first[MORPH_KEY_N1 * plane + i], last[MORPH_KEY_N1 * plane + i], r);
    Vec3 n2 = mixKeys(first[MORPH_KEY_N2 * plane + i], last[MORPH_KEY_N2 * plane + i], r);
    /* setPrimitive (GPUKernel.cpp:539-684), what it derives per type.  Of that the size and the mid-point stay: the normals
     * it derives - the cylinder's axis in n1, the planes' normals, the triangle's face normal - are all three overwritten
     * by setPrimitiveNormals right after it, whatever the type */
    if (type == ptSphere)
        size.y = size.z = size.x;
    else if (type == ptCylinder || type == ptCone)
    {
        p2.x = (p0.x + p1.x) / 2.f;
        p2.y = (p0.y + p1.y) / 2.f;
        p2.z = (p0.z + p1.z) / 2.f;
        size.y = size.z = size.x;
    }
    /* setPrimitiveNormals (GPUKernel.cpp:715-727) */
    normalizeVec3(n0);
    normalizeVec3(n1);
    normalizeVec3(n2);
    storeXyz(rows + ROW_P0_TYPE, p0);
    storeXyz(rows + ROW_SIZE_MAT, size);
    storeXyz(rows + ROW_P1_INDEX, p1);
    storeXyz(rows + ROW_P2, p2);
    storeXyz(rows + ROW_N0, n0);
    storeXyz(rows + ROW_N1, n1);
    storeXyz(rows + ROW_N2, n2);
}

/* solr_hip_set_morph_keys on one engine: the keys re-packed into planes and uploaded; per primitive whether its keys differ
 * (a lamp must not move: the light table would have to follow).  Keys for another number of primitives than the resident
 * scene's are kept all the same - the request is what gets refused, like a rotation with flags for another scene */
int setMorphKeysOne(const Primitive *first, const Primitive *last, int nbPrimitives)
{
    if (!ready("solr_hip_set_morph_keys"))
        return 0;
    g.scene.morphKeysDropped();
    if (!first || !last || nbPrimitives <= 0)
        return 0;
    quiesce();
    HIPCHECK(hipSetDevice(g.device));
    const size_t n = (size_t)nbPrimitives;
    std::vector<float4> planes[2];
    std::vector<unsigned char> differ(n, 0);
    for (int key = 0; key < 2; ++key)
    {
        const Primitive *p = key ? last : first;
        std::vector<float4> &out = planes[key];
        out.resize(MORPH_KEY_ROWS * n);
        for (size_t i = 0; i < n; ++i)
        {
            out[MORPH_KEY_P0 * n + i] = make_float4(p[i].p0.x, p[i].p0.y, p[i].p0.z, 0.f);
            out[MORPH_KEY_P1 * n + i] = make_float4(p[i].p1.x, p[i].p1.y, p[i].p1.z, 0.f);
            out[MORPH_KEY_P2 * n + i] = make_float4(p[i].p2.x, p[i].p2.y, p[i].p2.z, 0.f);
            out[MORPH_KEY_N0 * n + i] = make_float4(p[i].n0.x, p[i].n0.y, p[i].n0.z, 0.f);
            out[MORPH_KEY_N1 * n + i] = make_float4(p[i].n1.x, p[i].n1.y, p[i].n1.z, 0.f);
            out[MORPH_KEY_N2 * n + i] = make_float4(p[i].n2.x, p[i].n2.y, p[i].n2.z, 0.f);
            out[MORPH_KEY_SIZE * n + i] = make_float4(p[i].size.x, p[i].size.y, p[i].size.z, 0.f);
        }
    }
    for (size_t i = 0; i < n; ++i)
        for (int row = 0; row < MORPH_KEY_ROWS && !differ[i]; ++row)
            differ[i] = memcmp(&planes[0][row * n + i], &planes[1][row * n + i], sizeof(float4)) != 0;
    upload(g.scene.morph.first, planes[0]);
    upload(g.scene.morph.last, planes[1]);
    if (!ok())
        return 0;
    g.scene.morphKeysSet(nbPrimitives, differ);
    return 1;
}

/* does a primitive that lights the scene have keys that differ?  By the tags as they are now (a change of materials
 * retags the primitives: asked again then) */
static bool lampWouldMove()
{
    const Morph &m = g.scene.morph;
    if (m.lampChecked == g.scene.retags)
        return m.lampMoves;
    bool moves = false;
    const size_t n = std::min(m.keysDiffer.size(), g.scene.hostPrims.size() / PRIM_ROWS);
    for (size_t i = 0; i < n && !moves; ++i)
        moves = m.keysDiffer[i] && (bitsi(g.scene.hostPrims[PRIM_ROWS * i + ROW_P0_TYPE].w) & PRIM_EMISSIVE);
    g.scene.morphLampChecked(moves);
    return moves;
}

/* can this engine morph its resident scene?  (what canRotateOne asks, and the keys; changes nothing but the refit plan) */
bool canMorphOne(float weight, float viewDistance)
{
    static const float none[3] = {0.f, 0.f, 0.f};
    if (!canRotateOne(none, none, none, viewDistance, "solr_hip_morph_primitives"))
        return false;
    const Morph &m = g.scene.morph;
    /* (a lamp that was moved on the device, solr_moves.hip: the blend would put its p0 back at the keys' place and leave
     * its light record where the move put it - the host route makes the record from p0 again; primitives that were set
     * anew on the device, solr_edits.hip: the blend would leave their texture coordinates and movable flags behind) */
    if (m.nbKeys != g.scene.nbPrimitives || !m.first.ptr || !m.last.ptr || !std::isfinite(weight) || lampWouldMove() ||
        g.scene.rotation.lampMoved || g.scene.rotation.edited)
    {
        if (getenv("SOLR_HIP_DEBUG_TREE"))
            fprintf(stderr, "solr_hip_morph_primitives refused: keys for %d of %d primitives, weight %g, a lamp moved here: %d\n",
                    m.nbKeys, g.scene.nbPrimitives, weight, (int)g.scene.rotation.lampMoved);
        return false;
    }
    return true;
}

/* Extension: GPUKernel::morphFrame + h2d_scene on the resident scene, see k_morphPrimitives.  Returns 1 when the arena now
 * holds the morphed scene, 0 when the request cannot be served here and the caller has to take the host route (nothing
 * was changed). */
int morphPrimitivesOne(float weight, float viewDistance)
{
    if (!canMorphOne(weight, viewDistance))
        return 0;
    HIPCHECK(hipSetDevice(g.device));
    flushGeometry();
    if (!ok())
        return 0;
    quiesce();
    hipLaunchKernelGGL(k_morphPrimitives, dim3((unsigned)((g.scene.nbPrimitives + 255) / 256)), dim3(256), 0, sceneStream(),
                       (float4 *)g.scene.arena.geometry.ptr, g.scene.arena.offPrims, g.scene.nbPrimitives,
                       (const float4 *)g.scene.morph.first.ptr, (const float4 *)g.scene.morph.last.ptr, weight);
    const bool walkHolds = refitMovedScene(viewDistance);
    g.scene.morphServed(walkHolds, ok());
    return ok() ? 1 : 0;
}

} // namespace solreng

extern "C" {
int solr_hip_device_morphs(void)
{
    return g.scene.morph.nbDeviceMorphs;
}
} // extern "C"
