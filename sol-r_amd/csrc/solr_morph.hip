/*
 * solr_morph.hip - key-frame morphing of the MI355X rendering engine: solr_hip_set_morph_track_key hands over one key frame
 * of the resident scene per slot (k_packMorphKeys packs it on the device), solr_hip_morph_between blends any two of them into
 * the resident primitives at any weight and refits the node lists in the arena; solr_hip_set_morph_keys and
 * solr_hip_morph_primitives are the same with two slots of their own (engine.h Morph: the keys, RequestKind and
 * Scene::requestServed: what a served morph changes and which requests bar one, Engine::served: the counters; the refit and
 * what follows it: solr_rotation.hip refitMovedScene).
 * Part of the engine's host side (engine.h); the boundary that calls into it is solr_hip.hip.  gfx950 only.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>

#include "../../include/solr_hip.h"
#include "device_pool.h"
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

/* A key frame's records into its seven planes: lane i gathers the geometry of key[rankOf[i]] - the 21 floats p0 p1 p2 n0 n1 n2
 * size at the head of a 128-byte, 16-byte aligned record, read as six 16-byte loads of which the last 12 bytes (type, index,
 * materialId) are dropped - and stores seven float4 next to lane i - 1's.  The gather is the one access that is not
 * coalesced (a record per lane, wherever its rank lies); it is paid once per key, and every frame blended from the key
 * afterwards reads the planes lane next to lane.  rankOf == nullptr: the records are in the resident order already. */
__global__ __launch_bounds__(256) void k_packMorphKeys(const Primitive *__restrict__ key, const int *__restrict__ rankOf,
                                                       int nbPrimitives, float4 *__restrict__ planes)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nbPrimitives)
        return;
    const size_t plane = (size_t)nbPrimitives;
    const int rank = rankOf ? rankOf[i] : i;
    const float4 *record = (const float4 *)(key + rank);
    const float4 a = record[0], b = record[1], c = record[2], d = record[3], e = record[4], f = record[5];
    planes[MORPH_KEY_P0 * plane + i] = make_float4(a.x, a.y, a.z, 0.f);
    planes[MORPH_KEY_P1 * plane + i] = make_float4(a.w, b.x, b.y, 0.f);
    planes[MORPH_KEY_P2 * plane + i] = make_float4(b.z, b.w, c.x, 0.f);
    planes[MORPH_KEY_N0 * plane + i] = make_float4(c.y, c.z, c.w, 0.f);
    planes[MORPH_KEY_N1 * plane + i] = make_float4(d.x, d.y, d.z, 0.f);
    planes[MORPH_KEY_N2 * plane + i] = make_float4(d.w, e.x, e.y, 0.f);
    planes[MORPH_KEY_SIZE * plane + i] = make_float4(e.z, e.w, f.x, 0.f);
}
static_assert(offsetof(Primitive, p0) == 0 && offsetof(Primitive, p1) == 12 && offsetof(Primitive, p2) == 24 &&
                  offsetof(Primitive, n0) == 36 && offsetof(Primitive, n1) == 48 && offsetof(Primitive, n2) == 60 &&
                  offsetof(Primitive, size) == 72 && sizeof(Primitive) == 128 && alignof(Primitive) == 16,
              "k_packMorphKeys reads a record's geometry as six float4");

/* The lamp rule: does a primitive that lights the scene - by the tag the arena holds for it - have rows that differ, in any
 * bit, between two keys?  Such a pair is not blended here: the light table would have to follow. */
__global__ __launch_bounds__(256) void k_lampKeysDiffer(const float4 *__restrict__ arena, unsigned offPrims, int nbPrimitives,
                                                        const float4 *__restrict__ keyA, const float4 *__restrict__ keyB,
                                                        int *__restrict__ differ)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nbPrimitives)
        return;
    if (!(__float_as_int(arena[offPrims + (size_t)PRIM_ROWS * i + ROW_P0_TYPE].w) & PRIM_EMISSIVE))
        return;
    const size_t plane = (size_t)nbPrimitives;
    bool same = true;
    for (int row = 0; row < MORPH_KEY_ROWS; ++row)
    {
        const float4 a = keyA[row * plane + i], b = keyB[row * plane + i];
        same = same && __float_as_int(a.x) == __float_as_int(b.x) && __float_as_int(a.y) == __float_as_int(b.y) &&
               __float_as_int(a.z) == __float_as_int(b.z) && __float_as_int(a.w) == __float_as_int(b.w);
    }
    if (!same)
        *differ = 1; /* (every lane that writes, writes the same word) */
}

/* one slot's key on one engine: the records and the ranks go up with one copy each, into scratch that is given back before
 * this returns, and k_packMorphKeys makes the planes.  The slot holds no key until they are in place; an allocation that
 * fails declines the key (no error state: the caller takes the host route) */
static int packKeyOne(int slot, const Primitive *key, const int *rankOf, int nbPrimitives)
{
    g.scene.morphKeyDropped(slot);
    quiesce();
    HIPCHECK(hipSetDevice(g.device));
    if (!ok())
        return 0;
    const size_t n = (size_t)nbPrimitives;
    DeviceBuffer &planes = g.scene.morph.keys[slot].planes;
    const size_t bytes = (size_t)MORPH_KEY_ROWS * n * sizeof(float4);
    if (!planes.ptr || planes.bytes < bytes)
    {
        release(planes);
        if (hipMalloc(&planes.ptr, bytes) != hipSuccess)
        {
            (void)hipGetLastError();
            planes.ptr = nullptr;
            return 0;
        }
        planes.bytes = bytes;
    }
    SolrScratchPool &pool = solrScratchPool();
    std::lock_guard<std::mutex> oneBuild(pool.busy);
    pool.begin(n * (sizeof(Primitive) + sizeof(int)) + 1024);
    void *own[2] = {nullptr, nullptr};
    auto scratch = [&](int which, size_t size) -> void * {
        void *p = pool.take(size);
        if (!p && hipMalloc(&own[which], size) == hipSuccess)
            p = own[which];
        return p;
    };
    Primitive *records = (Primitive *)scratch(0, n * sizeof(Primitive));
    int *ranks = rankOf ? (int *)scratch(1, n * sizeof(int)) : nullptr;
    const bool fits = records && (ranks || !rankOf);
    if (fits)
    {
        /* pageable sources: the copies are complete for the caller when the stream has been waited for */
        HIPCHECK(hipMemcpyAsync(records, key, n * sizeof(Primitive), hipMemcpyHostToDevice, sceneStream()));
        if (ranks)
            HIPCHECK(hipMemcpyAsync(ranks, rankOf, n * sizeof(int), hipMemcpyHostToDevice, sceneStream()));
        if (ok())
            solrmorph::packMorphKeys(sceneStream(), records, ranks, nbPrimitives, (float4 *)planes.ptr);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(sceneStream()));
    }
    else
        (void)hipGetLastError();
    pool.end();
    for (void *p : own)
        if (p)
            (void)hipFree(p);
    if (!fits || !ok())
        return 0;
    g.scene.morphKeySet(slot, nbPrimitives);
    return 1;
}

/* solr_hip_set_morph_keys on one engine: its two slots, the records in the resident order already.  Keys for another
 * number of primitives than the resident scene's are kept all the same - the request is what gets refused, like a rotation
 * with flags for another scene */
int setMorphKeysOne(const Primitive *first, const Primitive *last, int nbPrimitives)
{
    if (!ready("solr_hip_set_morph_keys"))
        return 0;
    g.scene.morphKeyDropped(MORPH_SLOT_FIRST);
    g.scene.morphKeyDropped(MORPH_SLOT_LAST);
    if (!first || !last || nbPrimitives <= 0)
        return 0;
    return packKeyOne(MORPH_SLOT_FIRST, first, nullptr, nbPrimitives) && packKeyOne(MORPH_SLOT_LAST, last, nullptr, nbPrimitives);
}

/* solr_hip_set_morph_track_key on one engine: what cannot be a key of the resident scene is refused before anything is
 * launched, and leaves the slots as they are */
int setMorphTrackKeyOne(int slot, const Primitive *key, const int *rankOf, int nbPrimitives)
{
    if (!ready("solr_hip_set_morph_track_key"))
        return 0;
    if (slot < 0 || slot >= SOLR_MORPH_TRACK_MAX_KEYS || !key || !rankOf || nbPrimitives <= 0 || nbPrimitives != g.scene.nbPrimitives)
        return 0;
    for (int i = 0; i < nbPrimitives; ++i)
        if (rankOf[i] < 0 || rankOf[i] >= nbPrimitives)
            return 0;
    return packKeyOne(slot, key, rankOf, nbPrimitives);
}

/* does a primitive that lights the scene have rows that differ between the two slots (both hold keys of the resident
 * scene)?  By the tags as they are now (a change of materials retags the primitives: asked again then), once per ordered
 * pair of slots.  Asked on the device, where the planes are: a host-side answer would need a host copy of every key */
static bool lampWouldMove(int slotA, int slotB)
{
    Morph &m = g.scene.morph;
    if (m.lampChecked == g.scene.retags)
        for (const MorphLampAnswer &answer : m.lampAnswers)
            if (answer.slotA == slotA && answer.slotB == slotB)
                return answer.moves;
    if (slotA == slotB)
    {
        g.scene.morphLampNoted(slotA, slotB, false);
        return false;
    }
    HIPCHECK(hipSetDevice(g.device));
    flushGeometry(); /* the tags, where a host image has changed */
    reserve(m.lampFlag, sizeof(int));
    if (!ok() || !g.scene.arena.geometry.ptr)
        return true;
    quiesce();
    int differ = 0;
    HIPCHECK(hipMemsetAsync(m.lampFlag.ptr, 0, sizeof(int), sceneStream()));
    hipLaunchKernelGGL(k_lampKeysDiffer, dim3((unsigned)((g.scene.nbPrimitives + 255) / 256)), dim3(256), 0, sceneStream(),
                       (const float4 *)g.scene.arena.geometry.ptr, g.scene.arena.offPrims, g.scene.nbPrimitives,
                       (const float4 *)m.keys[slotA].planes.ptr, (const float4 *)m.keys[slotB].planes.ptr, (int *)m.lampFlag.ptr);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(&differ, m.lampFlag.ptr, sizeof(int), hipMemcpyDeviceToHost, sceneStream()));
    HIPCHECK(hipStreamSynchronize(sceneStream()));
    if (!ok())
        return true;
    g.scene.morphLampNoted(slotA, slotB, differ != 0);
    return differ != 0;
}

/* can this engine blend these two slots into its resident scene?  (canRefitOne, and the keys; changes nothing but the
 * refit plan and what is known about lamps) */
bool canMorphOne(int slotA, int slotB, float weight, float viewDistance, const char *who)
{
    if (!canRefitOne(viewDistance, who))
        return false;
    if (slotA < 0 || slotA >= MORPH_SLOTS || slotB < 0 || slotB >= MORPH_SLOTS)
        return false;
    const Morph &m = g.scene.morph;
    const MorphKey &a = m.keys[slotA], &b = m.keys[slotB];
    /* (morphBarredBy: a lamp move, an edit or a batch of materials served since h2d_scene, which the blend would undo in
     * part - engine.h RequestKind says how) */
    if (a.nbPrimitives != g.scene.nbPrimitives || b.nbPrimitives != g.scene.nbPrimitives || !a.planes.ptr || !b.planes.ptr ||
        !std::isfinite(weight) || g.scene.morphBarredBy != 0 || lampWouldMove(slotA, slotB))
    {
        noteRefusal(who, "keys for %d and %d of %d primitives, weight %g, barred by the request kinds of mask 0x%x", a.nbPrimitives,
                    b.nbPrimitives, g.scene.nbPrimitives, weight, g.scene.morphBarredBy);
        return false;
    }
    return true;
}

/* Extension: GPUKernel::morphBetween + h2d_scene on the resident scene, see k_morphPrimitives.  Returns 1 when the arena now
 * holds the morphed scene, 0 when the request cannot be served here and the caller has to take the host route (nothing
 * was changed). */
int morphKeysOne(int slotA, int slotB, float weight, float viewDistance, const char *who)
{
    if (!canMorphOne(slotA, slotB, weight, viewDistance, who) || !beginRequest())
        return 0;
    hipLaunchKernelGGL(k_morphPrimitives, dim3((unsigned)((g.scene.nbPrimitives + 255) / 256)), dim3(256), 0, sceneStream(),
                       (float4 *)g.scene.arena.geometry.ptr, g.scene.arena.offPrims, g.scene.nbPrimitives,
                       (const float4 *)g.scene.morph.keys[slotA].planes.ptr, (const float4 *)g.scene.morph.keys[slotB].planes.ptr,
                       weight);
    /* (a track's slots come first: asked through solr_hip_morph_between) */
    return finishRequest(slotA < SOLR_MORPH_TRACK_MAX_KEYS ? REQUEST_TRACK_MORPH : REQUEST_MORPH, refitMovedScene(viewDistance));
}

} // namespace solreng

namespace solrmorph
{
void packMorphKeys(hipStream_t stream, const Primitive *key, const int *rankOf, int nbPrimitives, float4 *planes)
{
    hipLaunchKernelGGL(solreng::k_packMorphKeys, dim3((unsigned)((nbPrimitives + 255) / 256)), dim3(256), 0, stream, key, rankOf,
                       nbPrimitives, planes);
}
} // namespace solrmorph

extern "C" {
int solr_hip_device_morphs(void)
{
    return g.served[REQUEST_MORPH];
}

int solr_hip_device_track_morphs(void)
{
    return g.served[REQUEST_TRACK_MORPH];
}

int solr_hip_morph_track_keys(void)
{
    return g.scene.morph.nbTrackKeys;
}
} // extern "C"
