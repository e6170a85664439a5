/*
 * solr_materials.hip - primitives' materials set on the resident scene of the MI355X rendering engine:
 * solr_hip_set_primitive_materials takes a batch of (slot, material id), joins the materials' facts into the tags of those
 * primitives as retagPrimitives does for all of them at an upload, and sets tag, material id and colour key in the arena, in
 * the leaf records and in the host image (engine.h Rotation: the batch's buffer, the counter, materialsSet; SceneFacts: the
 * counts the scene's facts follow by).  Nothing is pulled, laid out, uploaded or refitted.
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
/* ---- a sample that is marked, a picked primitive that is highlighted, atoms that are recoloured ------------------------
 * The reference's SWC scene gives one sample of the morphology the light material per frame and the sample before it its own
 * back (apps/scenes/science/SwcScene.cpp:66-89: setPrimitiveMaterial twice, the lamp moved next to the sample,
 * compactBoxes(false)), a full upload per frame.  Of everything that is uploaded, a material id reaches three words of the
 * primitive's record - the tag (ROW_P0_TYPE.w: type | the material's facts | kind), the id (ROW_SIZE_MAT.w) and the colour
 * key (ROW_P2.w) - and the copy of them in the leaf record of every leaf whose first primitive it is.  No box follows a
 * material (the flatten updates none), the light table is made of the lamps' cell alone, and the thin copies and the
 * order-free hierarchy read the primitives' kinds, which a served batch leaves as they are.
 *
 * The batch: one int4 a record - slot, material id, the material's facts (materialTag), the bits of its colour key -, records
 * in the order given: lane i of a wave reads the 16 bytes next to lane i - 1's.  Facts and colour key ride in the batch and
 * are not looked up in a table on the device: such a table would have NB_MAX_MATERIALS + 1 entries to keep in step with
 * every h2d_materials - which the reference's hosts call whenever one material changes - for the sake of batches that are
 * two records long in the scene this is for; the host holds both per material already (Materials::materialTags,
 * materialAverage) and 8 bytes more a record cost nothing next to the launch. */
__global__ __launch_bounds__(256) void k_setPrimitiveMaterials(float4 *__restrict__ arena, unsigned offPrims, int nbPrimitives,
                                                               const int4 *__restrict__ batch, int nbRecords, int noKinds)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nbRecords)
        return;
    const int4 r = batch[e];
    const int slot = r.x;
    if (slot < 0 || slot >= nbPrimitives) /* (checked on the host: canSetPrimitiveMaterialsOne) */
        return;
    float4 *rows = arena + offPrims + (size_t)PRIM_ROWS * slot;
    /* the type stays; the kind is the rule's again (the host has seen that it comes out as it was).  The geometry words of
     * the three rows are not written */
    const int type = __float_as_int(rows[ROW_P0_TYPE].w) & PRIM_TYPE_MASK;
    rows[ROW_P0_TYPE].w = __int_as_float(primitiveTag(type, r.z, noKinds != 0));
    rows[ROW_SIZE_MAT].w = __int_as_float(r.y);
    rows[ROW_P2].w = __int_as_float(r.w);
}

/* The leaf records follow (k_buildLeafRecords: record 0 and 1 are the first primitive's first two rows, a plane's colour
 * key is the first word of record 3): one thread per node of the lists, one list behind the other, the three words copied
 * from the primitive record as it is now - the same bits again for a leaf whose first primitive the batch did not name. */
struct LeafMaterialsFollow
{
    LeafRecordsOf list[3]; /* (engine.h) */
    unsigned offPrims;
    int nbPrimitives;
};
__global__ __launch_bounds__(256) void k_followLeafRecords(float4 *__restrict__ arena, const LeafMaterialsFollow M)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    for (int l = 0; l < 3; ++l)
    {
        const LeafRecordsOf &L = M.list[l];
        if (t < L.nodes)
        {
            const int nb = __float_as_int(arena[L.offRows + 2u * (unsigned)t + 1u].z);
            const int start = ((const int *)arena)[L.offStart + (unsigned)t];
            if (nb > 0 && start >= 0 && start < M.nbPrimitives)
            {
                const float4 *prim = arena + M.offPrims + (size_t)PRIM_ROWS * start;
                float4 *record = arena + L.offLeaf + 4u * (unsigned)t;
                const float tag = prim[ROW_P0_TYPE].w;
                record[0].w = tag;
                record[1].w = prim[ROW_SIZE_MAT].w;
                if (planeClass(__float_as_int(tag) & PRIM_TYPE_MASK))
                    record[3].x = prim[ROW_P2].w;
            }
            return;
        }
        t -= L.nodes;
    }
}

/* the facts and the colour key of an uploaded material, as retagPrimitives takes them */
static int factsOfMaterial(int materialId)
{
    return g.materials.materialTags[(size_t)materialId];
}
static float colourKeyOfMaterial(int materialId)
{
    return (size_t)materialId < g.materials.materialAverage.size() ? g.materials.materialAverage[(size_t)materialId] : 0.f;
}
static bool noKinds()
{
    return getenv("SOLR_HIP_NO_KINDS") != nullptr; /* (retagPrimitives) */
}
/* the material's facts of a tag word: everything between the type and the kind */
static int factsOfTag(int tag)
{
    return tag & ~PRIM_TYPE_MASK & ((1 << PRIM_KIND_SHIFT) - 1);
}

/* can this engine give these primitives of its resident scene these materials in place?  (changes nothing) */
bool canSetPrimitiveMaterialsOne(const int *slots, const int *materialIds, int n)
{
    if (!g.initialized || !ok())
        return false;
    const Scene &s = g.scene;
    const char *why = nullptr;
    int at = -1;
    if (s.nbPrimitives <= 0 || s.hostPrims.size() < (size_t)PRIM_ROWS * (size_t)s.nbPrimitives || s.exact.nb <= 0 ||
        g.facts.nbCounted != (int)(s.hostPrims.size() / PRIM_ROWS))
        why = "no resident scene";
    else if (!slots || !materialIds || n <= 0)
        why = "no records";
    std::vector<unsigned char> taken(why ? 0 : (size_t)s.nbPrimitives, 0);
    SceneFacts after = g.facts; /* (its counts: a few words) */
    const bool general = noKinds();
    for (int i = 0; i < n && !why; ++i)
    {
        const int slot = slots[i], material = materialIds[i];
        at = i;
        if (slot < 0 || slot >= s.nbPrimitives)
            why = "a slot out of range";
        else if (taken[slot])
            why = "a slot twice";
        else if (slot < s.nbLamps)
            why = "a slot among the lamps'"; /* its light record carries the material's id, colour and intensity */
        else if (material < 0 || material >= g.materials.nbMaterials || (size_t)material >= g.materials.materialTags.size())
            why = "a material that was not uploaded";
        else
        {
            taken[slot] = 1;
            /* (the tags are not moved by anything the device does: the host image holds them) */
            const int tag = bitsi(s.hostPrims[(size_t)PRIM_ROWS * slot + ROW_P0_TYPE].w);
            const int type = tag & PRIM_TYPE_MASK;
            const int facts = factsOfMaterial(material);
            /* the thin copies were made from the kinds, the order-free hierarchy on the thin boxes; plainPlanes and
             * looseSpheres are functions of the kinds */
            if (((primitiveTag(type, facts, general) ^ tag) >> PRIM_KIND_SHIFT) != 0)
                why = "a primitive whose kind would change";
            after.count(type, factsOfTag(tag), -1);
            after.count(type, facts, +1);
        }
    }
    if (!why)
    {
        after.deriveFromCounts();
        /* primsContained decides whether order-free lists exist at all (maybeBuildOrderFreeLists); sceneFeatures and
         * opaqueShadows only steer what a frame is told, and follow in place */
        if (after.primsContained != g.facts.primsContained)
            why = "a batch after which the primitives lie inside their leaves where they did not, or the other way round";
    }
    if (why && getenv("SOLR_HIP_DEBUG_TREE"))
        fprintf(stderr, "solr_hip_set_primitive_materials refused: %s (record %d of %d)\n", why, at, n);
    return why == nullptr;
}

/* Extension: GPUKernel::setPrimitiveMaterial per record + compactBoxes(false) + h2d_scene on the resident scene, see
 * k_setPrimitiveMaterials.  Returns 1 when the arena and the host image now hold the materials, 0 when the request cannot be
 * served here and the caller has to take the host route (nothing was changed). */
int setPrimitiveMaterialsOne(const int *slots, const int *materialIds, int n)
{
    if (!canSetPrimitiveMaterialsOne(slots, materialIds, n))
        return 0;
    HIPCHECK(hipSetDevice(g.device));
    flushGeometry();
    if (!ok() || !g.scene.arena.geometry.ptr)
        return 0;
    quiesce(); /* no frame in flight reads a tag that says one material next to the id of another */
    const bool general = noKinds();
    std::vector<int4> batch((size_t)n);
    for (int i = 0; i < n; ++i)
        batch[(size_t)i] = make_int4(slots[i], materialIds[i], factsOfMaterial(materialIds[i]), bitsi(colourKeyOfMaterial(materialIds[i])));
    reserve(g.scene.rotation.materialSets, batch.size() * sizeof(int4));
    if (!ok())
        return 0;
    /* (a pageable source: `batch` lives until the one synchronisation below) */
    HIPCHECK(hipMemcpyAsync(g.scene.rotation.materialSets.ptr, batch.data(), batch.size() * sizeof(int4), hipMemcpyHostToDevice, sceneStream()));
    hipLaunchKernelGGL(k_setPrimitiveMaterials, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sceneStream(),
                       (float4 *)g.scene.arena.geometry.ptr, g.scene.arena.offPrims, g.scene.nbPrimitives,
                       (const int4 *)g.scene.rotation.materialSets.ptr, n, general ? 1 : 0);
    LeafMaterialsFollow M;
    const int nodes = leafRecordsOfLists(g.scene, M.list);
    M.offPrims = g.scene.arena.offPrims;
    M.nbPrimitives = g.scene.nbPrimitives;
    if (nodes > 0)
        hipLaunchKernelGGL(k_followLeafRecords, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, sceneStream(),
                           (float4 *)g.scene.arena.geometry.ptr, M);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(sceneStream()));
    if (ok())
    {
        /* the host image and the scene's facts follow: the same words, the counts moved from the old facts to the new */
        for (int i = 0; i < n; ++i)
        {
            float4 *r = &g.scene.hostPrims[(size_t)PRIM_ROWS * slots[i]];
            const int tag = bitsi(r[ROW_P0_TYPE].w), type = tag & PRIM_TYPE_MASK, facts = batch[(size_t)i].z;
            g.facts.count(type, factsOfTag(tag), -1);
            g.facts.count(type, facts, +1);
            r[ROW_P0_TYPE].w = bitsf(primitiveTag(type, facts, general));
            r[ROW_SIZE_MAT].w = bitsf(materialIds[i]);
            r[ROW_P2].w = bitsf(batch[(size_t)i].w);
        }
        g.facts.deriveFromCounts();
        g.scene.retagged(); /* (the morph's lamp answers were given for the tags as they were) */
    }
    g.scene.materialSetsServed(ok());
    return ok() ? 1 : 0;
}

} // namespace solreng

extern "C" {
int solr_hip_device_material_sets(void)
{
    return g.scene.rotation.nbDeviceMaterialSets;
}
} // extern "C"
