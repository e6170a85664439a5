/*
 * solr_materials.hip - primitives' materials set on the resident scene of the MI355X rendering engine:
 * solr_hip_set_primitive_materials takes a batch of (slot, material id), joins the materials' facts into the tags of those
 * primitives as retagPrimitives does for all of them at an upload, and sets tag, material id and colour key in the arena, in
 * the leaf records and in the host image (engine.h Scene::materialSetBatch: the batch's buffer, RequestKind and
 * Scene::requestServed: what a served batch changes in the scene's record, Engine::served: the counter; SceneFacts: the
 * counts the scene's facts follow by).  Nothing is pulled, laid out, uploaded or refitted.
 * And the other direction of that join: solr_hip_edit_materials takes a table of which some materials were given other
 * values, overwrites their records in the device table and rewrites tag and colour key of every primitive that has one of
 * them (k_retagMaterials), against the host image of the table that h2dMaterialsOne keeps (engine.h Materials).
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
/* ... queued on the scene stream, behind the kernel that changed the primitives' words */
static void followLeafRecords()
{
    LeafMaterialsFollow M;
    const int nodes = leafRecordsOfLists(g.scene, M.list);
    M.offPrims = g.scene.arena.offPrims;
    M.nbPrimitives = g.scene.nbPrimitives;
    if (nodes > 0)
        hipLaunchKernelGGL(k_followLeafRecords, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, sceneStream(),
                           (float4 *)g.scene.arena.geometry.ptr, M);
    HIPCHECK(hipGetLastError());
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
    if (why)
        noteRefusal("solr_hip_set_primitive_materials", "%s (record %d of %d)", why, at, n);
    return why == nullptr;
}

/* Extension: GPUKernel::setPrimitiveMaterial per record + compactBoxes(false) + h2d_scene on the resident scene, see
 * k_setPrimitiveMaterials.  Returns 1 when the arena and the host image now hold the materials, 0 when the request cannot be
 * served here and the caller has to take the host route (nothing was changed). */
int setPrimitiveMaterialsOne(const int *slots, const int *materialIds, int n)
{
    /* (no frame in flight reads a tag that says one material next to the id of another) */
    if (!canSetPrimitiveMaterialsOne(slots, materialIds, n) || !beginRequest())
        return 0;
    const bool general = noKinds();
    std::vector<int4> batch((size_t)n);
    for (int i = 0; i < n; ++i)
        batch[(size_t)i] = make_int4(slots[i], materialIds[i], factsOfMaterial(materialIds[i]), bitsi(colourKeyOfMaterial(materialIds[i])));
    reserve(g.scene.materialSetBatch, batch.size() * sizeof(int4));
    if (!ok())
        return 0;
    /* (a pageable source: `batch` lives until the one synchronisation below) */
    HIPCHECK(hipMemcpyAsync(g.scene.materialSetBatch.ptr, batch.data(), batch.size() * sizeof(int4), hipMemcpyHostToDevice, sceneStream()));
    hipLaunchKernelGGL(k_setPrimitiveMaterials, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sceneStream(),
                       (float4 *)g.scene.arena.geometry.ptr, g.scene.arena.offPrims, g.scene.nbPrimitives,
                       (const int4 *)g.scene.materialSetBatch.ptr, n, general ? 1 : 0);
    followLeafRecords();
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
    return finishRequest(REQUEST_MATERIAL_SETS);
}

/* ---- a colour that pulses, glass that fades in, a wireframe toggled, a texture swapped -----------------------------------
 * The other direction of the same join: not a primitive given another material, but a material given other values
 * (SolR_SetMaterial, GPUKernel::setMaterialColor, setMaterialTextureId; the reference's hosts then upload the table, and
 * h2dMaterialsOne retags every primitive and has the arena laid out and uploaded again).  Of all that, a material reaches
 * its two records of the table, and in every primitive that has it the tag (ROW_P0_TYPE.w) and the colour key (ROW_P2.w),
 * with their copies in the leaf records; the material id stays, and so does every box, the light table (made at the
 * flatten, h2d_materials does not touch it either) and - as long as no kind changes - the thin copies and the order-free
 * hierarchy.
 *
 * One lane per primitive of the resident scene; the batch: one int4 per material whose facts or colour key changed - id,
 * facts (materialTag), the bits of the colour key, 0 -, ascending by id.  A lane looks its primitive's material id up in the
 * batch: up to RETAG_LINEAR records by a loop whose counter every lane of the wave shares (the records come through scalar
 * loads, the pulse of one material is one record), more by a binary search per lane.  Only a lane that finds its material
 * writes, and only the two words. */
enum
{
    RETAG_LINEAR = 8
};
__global__ __launch_bounds__(256) void k_retagMaterials(float4 *__restrict__ arena, unsigned offPrims, int nbPrimitives,
                                                        const int4 *__restrict__ batch, int nbRecords, int noKinds)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nbPrimitives)
        return;
    float4 *rows = arena + offPrims + (size_t)PRIM_ROWS * p;
    const int material = __float_as_int(rows[ROW_SIZE_MAT].w);
    int facts = 0, key = 0;
    bool found = false;
    if (nbRecords <= RETAG_LINEAR)
    {
        for (int e = 0; e < nbRecords; ++e)
        {
            const int4 r = batch[e];
            if (r.x == material)
            {
                found = true;
                facts = r.y;
                key = r.z;
            }
        }
    }
    else
    {
        int lo = 0, hi = nbRecords - 1;
        while (lo < hi)
        {
            const int mid = (lo + hi) >> 1;
            if (batch[mid].x < material)
                lo = mid + 1;
            else
                hi = mid;
        }
        const int4 r = batch[lo];
        found = r.x == material;
        facts = r.y;
        key = r.z;
    }
    if (!found)
        return;
    /* the type stays; the kind is the rule's again (the host has seen that it comes out as it was) */
    const int type = __float_as_int(rows[ROW_P0_TYPE].w) & PRIM_TYPE_MASK;
    rows[ROW_P0_TYPE].w = __int_as_float(primitiveTag(type, facts, noKinds != 0));
    rows[ROW_P2].w = __int_as_float(key);
}

/* what an edited table changes, against the image of the table as uploaded (Materials::imageHot, imageCold) */
struct MaterialEditPlan
{
    std::vector<int> ids; /* the materials whose records differ, ascending */
    std::vector<MaterialHot> hot;
    std::vector<MaterialCold> cold;
    std::vector<MaterialRecord> records;
    std::vector<int4> batch; /* k_retagMaterials': those of them whose facts or colour key differ */
    bool factsChange = false;
    SceneFacts after;
};

/* nullptr: the engine can follow the edit, and `plan` says how; else why not (nothing was changed either way) */
static const char *planMaterialEdit(const Material *materials, int nbActiveMaterials, MaterialEditPlan &plan)
{
    if (!g.initialized || !ok())
        return "no engine, or an error pending";
    const Scene &s = g.scene;
    const Materials &M = g.materials;
    if (s.nbPrimitives <= 0 || s.hostPrims.size() < (size_t)PRIM_ROWS * (size_t)s.nbPrimitives || s.exact.nb <= 0 ||
        g.facts.nbCounted != (int)(s.hostPrims.size() / PRIM_ROWS) || !s.arena.geometry.ptr)
        return "no resident scene";
    if (s.arena.geometryDirty)
        return "a layout of the arena is due anyway";
    /* Behind a move on the device h2dMaterialsOne's retag also takes the scene's extent and whether a leaf of spheres is
     * boxed loosely from the geometry as it was moved, and the thin copies of the lists are made again with the margin and
     * the reach that follow from them.  Thin copies are made of scenes with axis planes alone (tightenList): of those the
     * table is uploaded, and the copies come out as that leaves them; every other scene keeps no copy that could differ */
    if (s.arena.deviceAhead && (g.facts.sceneFeatures & F_PLANE))
        return "a scene with axis planes that was moved on the device: its thin copies follow the extent of the moved scene";
    if (!materials || nbActiveMaterials <= 0 || nbActiveMaterials != M.nbMaterials)
        return "another number of materials than the table holds";
    if (M.nbImaged != std::min(nbActiveMaterials, NB_MAX_MATERIALS + 1) || !M.table.ptr ||
        M.imageHot.size() < (size_t)M.nbImaged || M.imageCold.size() < (size_t)M.nbImaged)
        return "no image of the table";
    MaterialHot hot;
    MaterialCold cold;
    std::vector<int> changedAt((size_t)M.nbImaged, -1); /* material id -> its place in plan.batch */
    for (int i = 0; i < M.nbImaged; ++i)
    {
        memset(&hot, 0, sizeof hot);
        memset(&cold, 0, sizeof cold);
        const MaterialRecord record = materialRecord(materials[i], i, hot, cold);
        if (!memcmp(&hot, &M.imageHot[(size_t)i], sizeof hot) && !memcmp(&cold, &M.imageCold[(size_t)i], sizeof cold))
            continue;
        plan.ids.push_back(i);
        plan.hot.push_back(hot);
        plan.cold.push_back(cold);
        plan.records.push_back(record);
        const bool facts = record.facts != factsOfMaterial(i);
        if (facts || bitsi(record.average) != bitsi(colourKeyOfMaterial(i)))
        {
            changedAt[(size_t)i] = (int)plan.batch.size();
            plan.batch.push_back(make_int4(i, record.facts, bitsi(record.average), 0));
        }
        plan.factsChange = plan.factsChange || facts;
    }
    plan.after = g.facts;
    if (!plan.factsChange)
        return nullptr; /* no tag changes: no kind and no fact of the scene can */
    /* how many primitives of each type have each of those materials: from the host image (no move on the device changes
     * a tag or a material id, and setPrimitiveMaterialsOne keeps the image current) */
    const int types = PRIM_TYPE_MASK + 1;
    std::vector<int> census(plan.batch.size() * (size_t)types, 0);
    for (int p = 0; p < s.nbPrimitives; ++p)
    {
        const float4 *r = &s.hostPrims[(size_t)PRIM_ROWS * p];
        const int material = bitsi(r[ROW_SIZE_MAT].w);
        if (material >= 0 && material < M.nbImaged && changedAt[(size_t)material] >= 0)
            ++census[(size_t)changedAt[(size_t)material] * types + (bitsi(r[ROW_P0_TYPE].w) & PRIM_TYPE_MASK)];
    }
    const bool general = noKinds();
    for (size_t e = 0; e < plan.batch.size(); ++e)
    {
        const int before = factsOfMaterial(plan.batch[e].x), facts = plan.batch[e].y;
        for (int type = 0; type < types; ++type)
        {
            const int n = census[e * types + type];
            if (n == 0 || facts == before)
                continue;
            /* the thin copies were made from the kinds, the order-free hierarchy on the thin boxes; plainPlanes and
             * looseSpheres are functions of the kinds (canSetPrimitiveMaterialsOne) */
            if (((primitiveTag(type, facts, general) ^ primitiveTag(type, before, general)) >> PRIM_KIND_SHIFT) != 0)
                return "a material of primitives whose kind would change";
            plan.after.count(type, before, -n);
            plan.after.count(type, facts, +n);
        }
    }
    plan.after.deriveFromCounts();
    if (plan.after.primsContained != g.facts.primsContained)
        return "an edit after which the primitives lie inside their leaves where they did not, or the other way round";
    return nullptr;
}

/* can this engine follow this edit of the table on its resident scene?  (changes nothing) */
bool canEditMaterialsOne(const Material *materials, int nbActiveMaterials)
{
    MaterialEditPlan plan;
    const char *why = planMaterialEdit(materials, nbActiveMaterials, plan);
    if (why)
        noteRefusal("solr_hip_edit_materials", "%s (%d materials)", why, nbActiveMaterials);
    return why == nullptr;
}

/* Extension: h2d_materials for a table of which a few materials changed, on the resident scene - see k_retagMaterials.
 * Returns 1 when the table, the arena and the host images now hold the edit, 0 when the request cannot be served here and the
 * caller has to call h2d_materials (nothing was changed).
 * The changed records go to the table one copy per run of consecutive ids, straight from the plan: an edit is one material
 * in the hosts this is for - two copies of 96 bytes -, and a scatter kernel would want the same records staged in a buffer of
 * its own first, a copy and a launch where the copies alone do. */
int editMaterialsOne(const Material *materials, int nbActiveMaterials)
{
    MaterialEditPlan plan;
    if (planMaterialEdit(materials, nbActiveMaterials, plan))
        return 0;
    Materials &M = g.materials;
    if (plan.ids.empty())
    {
        ++M.nbDeviceEdits; /* the table holds it already */
        return 1;
    }
    /* (no layout is due - planMaterialEdit -: the flush takes order-free lists the builder has just left into the arena,
     * where the next frame would, so that their leaf records follow with the others'; no frame in flight reads a record next
     * to a tag of the material as it was) */
    if (!beginRequest())
        return 0;
    char *table = (char *)M.table.ptr;
    const size_t coldAt = (size_t)M.offMatCold * sizeof(float4);
    for (size_t a = 0, b; a < plan.ids.size(); a = b)
    {
        for (b = a + 1; b < plan.ids.size() && plan.ids[b] == plan.ids[b - 1] + 1;)
            ++b;
        /* (pageable sources: `plan` lives until the one synchronisation below) */
        HIPCHECK(hipMemcpyAsync(table + (size_t)plan.ids[a] * sizeof(MaterialHot), &plan.hot[a], (b - a) * sizeof(MaterialHot),
                                hipMemcpyHostToDevice, sceneStream()));
        HIPCHECK(hipMemcpyAsync(table + coldAt + (size_t)plan.ids[a] * sizeof(MaterialCold), &plan.cold[a],
                                (b - a) * sizeof(MaterialCold), hipMemcpyHostToDevice, sceneStream()));
    }
    const bool retag = !plan.batch.empty();
    const bool general = noKinds();
    if (retag && ok())
    {
        reserve(M.editBatch, plan.batch.size() * sizeof(int4));
        if (ok())
        {
            HIPCHECK(hipMemcpyAsync(M.editBatch.ptr, plan.batch.data(), plan.batch.size() * sizeof(int4), hipMemcpyHostToDevice,
                                    sceneStream()));
            hipLaunchKernelGGL(k_retagMaterials, dim3((unsigned)((g.scene.nbPrimitives + 255) / 256)), dim3(256), 0, sceneStream(),
                               (float4 *)g.scene.arena.geometry.ptr, g.scene.arena.offPrims, g.scene.nbPrimitives,
                               (const int4 *)M.editBatch.ptr, (int)plan.batch.size(), general ? 1 : 0);
            followLeafRecords();
        }
    }
    HIPCHECK(hipStreamSynchronize(sceneStream()));
    /* (a copy that failed leaves a table nobody can vouch for: the image goes, and the next upload is a whole one) */
    M.nbImaged = ok() ? M.nbImaged : -1;
    if (!ok())
        return 0;
    /* what h2dMaterialsOne leaves on the host, for the changed materials */
    for (size_t k = 0; k < plan.ids.size(); ++k)
    {
        const size_t id = (size_t)plan.ids[k];
        M.imageHot[id] = plan.hot[k];
        M.imageCold[id] = plan.cold[k];
        M.materialTags[id] = plan.records[k].facts;
        M.materialAverage[id] = plan.records[k].average;
    }
    std::vector<TextureUse> uses;
    size_t k = 0;
    for (const TextureUse &use : M.textureUses) /* (ascending by material, as h2dMaterialsOne leaves them) */
    {
        for (; k < plan.ids.size() && plan.ids[k] < use.material; ++k)
            if (plan.records[k].textured)
                uses.push_back(plan.records[k].use);
        if (k < plan.ids.size() && plan.ids[k] == use.material)
            continue; /* (its new tables, if it has any, come with the loop above or below) */
        uses.push_back(use);
    }
    for (; k < plan.ids.size(); ++k)
        if (plan.records[k].textured)
            uses.push_back(plan.records[k].use);
    M.textureUses.swap(uses);
    g.textures.textureTablesChecked = false; /* the atlas check runs again before the next frame, as after h2d_materials */
    ++M.generation;                          /* a parked scene is retagged at its resume (solr_bank.hip) */
    if (retag)
    {
        /* the host image's two words follow, and the scene's facts by the counts */
        std::vector<int> changedAt((size_t)M.nbImaged, -1);
        for (size_t e = 0; e < plan.batch.size(); ++e)
            changedAt[(size_t)plan.batch[e].x] = (int)e;
        for (int p = 0; p < g.scene.nbPrimitives; ++p)
        {
            float4 *r = &g.scene.hostPrims[(size_t)PRIM_ROWS * p];
            const int material = bitsi(r[ROW_SIZE_MAT].w);
            if (material < 0 || material >= M.nbImaged || changedAt[(size_t)material] < 0)
                continue;
            const int4 &record = plan.batch[(size_t)changedAt[(size_t)material]];
            r[ROW_P0_TYPE].w = bitsf(primitiveTag(bitsi(r[ROW_P0_TYPE].w) & PRIM_TYPE_MASK, record.y, general));
            r[ROW_P2].w = bitsf(record.z);
        }
        g.facts = plan.after; /* (count(type, old facts, -n), count(type, new facts, +n), deriveFromCounts: planMaterialEdit) */
        g.scene.retagged();   /* (the morph's lamp answers were given for the tags as they were) */
        ++M.nbDeviceRetags;
    }
    ++M.nbDeviceEdits;
    return 1;
}

} // namespace solreng

extern "C" {
int solr_hip_device_material_sets(void)
{
    return g.served[REQUEST_MATERIAL_SETS];
}
int solr_hip_device_material_edits(void)
{
    return g.materials.nbDeviceEdits;
}
int solr_hip_device_material_retags(void)
{
    return g.materials.nbDeviceRetags;
}
} // extern "C"
