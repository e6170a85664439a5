/*
 * solr_edits.hip - primitives set anew on the resident scene of the MI355X rendering engine: solr_hip_set_primitives takes a
 * batch of edited primitives, derives what GPUKernel::setPrimitive derives per type, scatters them into the arena and refits
 * the node lists (engine.h Scene::editBatch: the batch's buffer, RequestKind and Scene::requestServed: what a served batch
 * changes in the scene's record, Engine::served: the counter; the refit and what follows it: solr_rotation.hip refitMovedScene).
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
/* ---- scenes that animate their own vertices: set a batch of primitives + refit on the device ---------------------------
 * The reference's water scene sets 1152 of its triangles anew every frame - setPrimitive, setPrimitiveNormals,
 * setPrimitiveTextureCoordinates -, runs the box updates and flattens again (apps/scenes/animation/WaterScene.cpp doAnimate,
 * GPUKernel.cpp:539-727), a full upload per frame.  None of that changes the shape of the flattened tree, so the setters run
 * here on the resident arena, one thread per edited primitive: every expression below is the host setters' (sol-r_amd/host/
 * GPUKernel.cpp setPrimitive, setPrimitiveNormals with normalizeVector and crossProduct), in their order, binary32 without
 * contraction, so that the arena afterwards holds bit for bit what the setters followed by a fresh upload would have put there.
 * The nodes follow bottom-up through the rotation's refit.
 *
 * The batch: seven planes of n float4 and one of n floats, edits in the order given - lane i of a wave reads the 16 bytes next
 * to lane i - 1's.  The fourth words of the float4 planes carry the slot, the flags and five of the six texture words. */
enum EditPlane
{
    EDIT_P0_SLOT = 0, /* .w: the slot, bits of an int */
    EDIT_P1_FLAGS,    /* .w: SolrEditFlags, bits of an int */
    EDIT_P2_VT0X,
    EDIT_SIZE_VT0Y,
    EDIT_N0_VT1X,
    EDIT_N1_VT1Y,
    EDIT_N2_VT2X,
    EDIT_PLANES /* behind them: a plane of n floats, vt2.y */
};

struct Vec3
{
    float x, y, z;
};

__device__ inline Vec3 xyzOf(const float4 &v)
{
    Vec3 r;
    r.x = v.x;
    r.y = v.y;
    r.z = v.z;
    return r;
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

__device__ inline Vec3 axisNormal(float x, float y, float z)
{
    Vec3 v;
    v.x = x;
    v.y = y;
    v.z = z;
    return v;
}

/* a row's geometry words and its fourth word / the geometry words alone (tag, material id, index and colour key stay) */
__device__ inline void storeRow(float4 *row, const Vec3 &v, float w)
{
    *row = make_float4(v.x, v.y, v.z, w);
}
__device__ inline void storeXyz(float4 *row, const Vec3 &v)
{
    row->x = v.x;
    row->y = v.y;
    row->z = v.z;
}

__global__ __launch_bounds__(256) void k_setPrimitives(float4 *__restrict__ arena, unsigned offPrims, int nbPrimitives,
                                                       unsigned char *__restrict__ movable, const float4 *__restrict__ batch,
                                                       int nbEdits)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nbEdits)
        return;
    const size_t plane = (size_t)nbEdits;
    const float4 a0 = batch[EDIT_P0_SLOT * plane + e], a1 = batch[EDIT_P1_FLAGS * plane + e], a2 = batch[EDIT_P2_VT0X * plane + e];
    const float4 as = batch[EDIT_SIZE_VT0Y * plane + e];
    const int slot = __float_as_int(a0.w);
    const int flags = __float_as_int(a1.w);
    if (slot < 0 || slot >= nbPrimitives) /* (checked on the host: canSetPrimitivesOne) */
        return;
    float4 *rows = arena + offPrims + (size_t)PRIM_ROWS * slot;
    const int type = __float_as_int(rows[ROW_P0_TYPE].w) & PRIM_TYPE_MASK;
    /* setPrimitive (GPUKernel.cpp:539-684): the points and the size as given, normals and texture coordinates zero, then
     * what it derives per type */
    const Vec3 p0 = xyzOf(a0), p1 = xyzOf(a1);
    Vec3 p2 = xyzOf(a2), size = xyzOf(as);
    Vec3 n0 = axisNormal(0.f, 0.f, 0.f), n1 = n0, n2 = n0;
    switch (type)
    {
    case ptSphere:
        size.y = size.z = size.x;
        break;
    case ptCylinder:
    case ptCone:
    {
        Vec3 axis = axisNormal(p1.x - p0.x, p1.y - p0.y, p1.z - p0.z);
        normalizeVec3(axis);
        n1 = axis;
        p2.x = (p0.x + p1.x) / 2.f;
        p2.y = (p0.y + p1.y) / 2.f;
        p2.z = (p0.z + p1.z) / 2.f;
        size.y = size.z = size.x;
        break;
    }
    case ptXYPlane:
        n0 = n1 = n2 = axisNormal(0.f, 0.f, 1.f);
        break;
    case ptYZPlane:
        n0 = n1 = n2 = axisNormal(1.f, 0.f, 0.f);
        break;
    case ptXZPlane:
    case ptCheckboard:
        n0 = n1 = n2 = axisNormal(0.f, 1.f, 0.f);
        break;
    case ptTriangle:
    {
        Vec3 v0 = axisNormal(p1.x - p0.x, p1.y - p0.y, p1.z - p0.z);
        normalizeVec3(v0);
        Vec3 v1 = axisNormal(p2.x - p0.x, p2.y - p0.y, p2.z - p0.z);
        normalizeVec3(v1);
        /* crossProduct(v0, v1) */
        n0.x = v0.y * v1.z - v0.z * v1.y;
        n0.y = v0.z * v1.x - v0.x * v1.z;
        n0.z = v0.x * v1.y - v0.y * v1.x;
        normalizeVec3(n0);
        n1 = n2 = n0;
        break;
    }
    default:
        break;
    }
    const float4 b0 = batch[EDIT_N0_VT1X * plane + e], b1 = batch[EDIT_N1_VT1Y * plane + e], b2 = batch[EDIT_N2_VT2X * plane + e];
    /* setPrimitiveNormals (GPUKernel.cpp:715-727) */
    if (flags & SOLR_EDIT_NORMALS)
    {
        n0 = xyzOf(b0);
        n1 = xyzOf(b1);
        n2 = xyzOf(b2);
        normalizeVec3(n0);
        normalizeVec3(n1);
        normalizeVec3(n2);
    }
    /* setPrimitiveTextureCoordinates; setPrimitive's zeros without it (h2d_scene keeps the six words in N0.w N1.w N2.w UV.xyz) */
    float vt0x = 0.f, vt0y = 0.f, vt1x = 0.f, vt1y = 0.f, vt2x = 0.f, vt2y = 0.f;
    if (flags & SOLR_EDIT_TEXTURE_COORDINATES)
    {
        vt0x = a2.w;
        vt0y = as.w;
        vt1x = b0.w;
        vt1y = b1.w;
        vt2x = b2.w;
        vt2y = ((const float *)(batch + EDIT_PLANES * plane))[e];
    }
    storeXyz(rows + ROW_P0_TYPE, p0);
    storeXyz(rows + ROW_SIZE_MAT, size);
    storeXyz(rows + ROW_P1_INDEX, p1);
    storeXyz(rows + ROW_P2, p2);
    storeRow(rows + ROW_N0, n0, vt0x);
    storeRow(rows + ROW_N1, n1, vt0y);
    storeRow(rows + ROW_N2, n2, vt1x);
    float4 *uv = rows + ROW_UV;
    uv->x = vt1y;
    uv->y = vt2x;
    uv->z = vt2y;
    /* setPrimitive makes the primitive movable; the camera primitive is never moved (GPUKernel::appendPrimitive) */
    movable[slot] = (unsigned char)(type != ptCamera);
}

static bool finite3(const vec3f &v)
{
    return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z);
}
static bool finite2(const vec2f &v)
{
    return std::isfinite(v.x) && std::isfinite(v.y);
}

/* can this engine set these primitives of its resident scene?  (canRefitOne, and every record against the resident
 * primitive it names; changes nothing but the refit plan) */
bool canSetPrimitivesOne(const SolrPrimitiveEdit *edits, const int *slots, int n, float viewDistance)
{
    if (!canRefitOne(viewDistance, "solr_hip_set_primitives"))
        return false;
    const Scene &s = g.scene;
    const char *why = nullptr;
    int at = -1;
    if (!edits || !slots || n <= 0)
        why = "no records";
    else if (s.hostPrims.size() < (size_t)PRIM_ROWS * (size_t)s.nbPrimitives)
        why = "no resident scene";
    std::vector<unsigned char> taken(why ? 0 : (size_t)s.nbPrimitives, 0);
    for (int i = 0; i < n && !why; ++i)
    {
        const SolrPrimitiveEdit &e = edits[i];
        const int slot = slots[i];
        at = i;
        if (slot < 0 || slot >= s.nbPrimitives)
            why = "a slot out of range";
        else if (taken[slot])
            why = "a slot twice";
        else if (slot < s.nbLamps)
            why = "a slot among the lamps'"; /* the lamps' cell is no level-0 box: no move reaches it, its light record would lag */
        else
        {
            taken[slot] = 1;
            /* (tag, material id and index are not moved by anything the device does: the host image holds them) */
            const float4 *r = &s.hostPrims[(size_t)PRIM_ROWS * slot];
            if (bitsi(r[ROW_P1_INDEX].w) != e.index)
                why = "a record for another primitive than its slot holds";
            else if (bitsi(r[ROW_SIZE_MAT].w) != e.materialId)
                why = "another material than the resident primitive's"; /* tag and colour key are a join with the materials */
            else if (bitsi(r[ROW_P0_TYPE].w) & PRIM_EMISSIVE)
                why = "a primitive of an emissive material";
            else if (!finite3(e.p0) || !finite3(e.p1) || !finite3(e.p2) || !finite3(e.size) || !finite3(e.n0) || !finite3(e.n1) ||
                     !finite3(e.n2) || !finite2(e.vt0) || !finite2(e.vt1) || !finite2(e.vt2))
                why = "a float that is not finite";
        }
    }
    if (why)
        noteRefusal("solr_hip_set_primitives", "%s (record %d of %d)", why, at, n);
    return why == nullptr;
}

/* Extension: GPUKernel::setPrimitives + compactBoxes(false) + h2d_scene on the resident scene, see k_setPrimitives.  Returns 1
 * when the arena now holds the edited scene, 0 when the request cannot be served here and the caller has to take the host
 * route (nothing was changed). */
int setPrimitivesOne(const SolrPrimitiveEdit *edits, const int *slots, int n, float viewDistance)
{
    if (!canSetPrimitivesOne(edits, slots, n, viewDistance) || !beginRequest() || !g.scene.refit.movable.ptr)
        return 0; /* (the kernel writes the flags too) */
    const size_t plane = (size_t)n;
    /* (float4 planes first, so that the plane of floats behind them needs no padding) */
    std::vector<float> batch((size_t)EDIT_PLANES * 4 * plane + plane);
    float4 *planes = (float4 *)batch.data();
    float *last = batch.data() + (size_t)EDIT_PLANES * 4 * plane;
    for (size_t i = 0; i < plane; ++i)
    {
        const SolrPrimitiveEdit &e = edits[i];
        planes[EDIT_P0_SLOT * plane + i] = make_float4(e.p0.x, e.p0.y, e.p0.z, bitsf(slots[i]));
        planes[EDIT_P1_FLAGS * plane + i] = make_float4(e.p1.x, e.p1.y, e.p1.z, bitsf((int)e.flags));
        planes[EDIT_P2_VT0X * plane + i] = make_float4(e.p2.x, e.p2.y, e.p2.z, e.vt0.x);
        planes[EDIT_SIZE_VT0Y * plane + i] = make_float4(e.size.x, e.size.y, e.size.z, e.vt0.y);
        planes[EDIT_N0_VT1X * plane + i] = make_float4(e.n0.x, e.n0.y, e.n0.z, e.vt1.x);
        planes[EDIT_N1_VT1Y * plane + i] = make_float4(e.n1.x, e.n1.y, e.n1.z, e.vt1.y);
        planes[EDIT_N2_VT2X * plane + i] = make_float4(e.n2.x, e.n2.y, e.n2.z, e.vt2.x);
        last[i] = e.vt2.y;
    }
    upload(g.scene.editBatch, batch);
    if (!ok())
        return 0;
    hipLaunchKernelGGL(k_setPrimitives, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sceneStream(),
                       (float4 *)g.scene.arena.geometry.ptr, g.scene.arena.offPrims, g.scene.nbPrimitives,
                       (unsigned char *)g.scene.refit.movable.ptr, (const float4 *)g.scene.editBatch.ptr, n);
    return finishRequest(REQUEST_EDIT, refitMovedScene(viewDistance));
}

} // namespace solreng

extern "C" {
int solr_hip_device_edits(void)
{
    return g.served[REQUEST_EDIT];
}
} // extern "C"
