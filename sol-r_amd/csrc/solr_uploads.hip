/*
 * solr_uploads.hip - the uploads of the MI355X rendering engine: what h2d_scene / h2d_materials / h2d_textures /
 * h2d_randoms / h2d_lightInformation (CudaRayTracer.cu:1536-1625) and solr_hip_set_movable leave in the engine's records
 * (engine.h Scene, Lights, Materials, Textures, Randoms) - row conversion (scene_layout.h), material tags, what the tags
 * and the primitives say about the scene (retagPrimitives), texture tables; the walk-order list comes from the host
 * builders (list_builders.cpp) - and the read-back of the resident lists and primitives for tests.  The arena they are
 * resident in: solr_arena.hip; rotation on the device: solr_rotation.hip.
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
/* list_builders.h names the rows of a primitive record on its own (it is compiled without the device headers) */
static_assert((int)LB_ROW_P0_TYPE == (int)ROW_P0_TYPE && (int)LB_ROW_SIZE_MAT == (int)ROW_SIZE_MAT &&
                  (int)LB_ROW_P1_INDEX == (int)ROW_P1_INDEX && (int)LB_ROW_P2 == (int)ROW_P2 && (int)LB_PRIM_ROWS == (int)PRIM_ROWS &&
                  (int)LB_PRIM_TYPE_MASK == (int)PRIM_TYPE_MASK,
              "list_builders.h and scene_layout.h disagree about the primitive record");

/* join the material facts the walks need into every primitive's tag (scene_layout.h) */
int materialTag(const Material &m)
{
    int tag = 0;
    if (m.attributes.x == 0)
        tag |= PRIM_FAST0;
    if (m.attributes.x == 1)
        tag |= PRIM_FAST1;
    if (m.attributes.y != 0)
        tag |= PRIM_PROCEDURAL;
    if (m.transparency != 0.f)
        tag |= PRIM_TRANSPARENT;
    if (m.attributes.z == 1)
        tag |= PRIM_WIRE1;
    if (m.attributes.z == 2)
        tag |= PRIM_WIRE2;
    if (m.innerIllumination.x != 0.f)
        tag |= PRIM_EMISSIVE;
    if (m.textureIds.x != TEXTURE_NONE)
        tag |= PRIM_TEXTURED;
    int w = m.attributes.w;
    w = w < -1 ? -1 : (w > 100 ? 100 : w); /* wireFrameMapping compares X % 100 <= width */
    tag |= (w + 1) << PRIM_WIDTH_SHIFT;
    return tag;
}

void retagPrimitives()
{
    pullGeometry();
    const size_t n = g.scene.hostPrims.size() / PRIM_ROWS;
    const bool noKinds = getenv("SOLR_HIP_NO_KINDS") != nullptr; /* tests: every primitive through the general tests */
    bool planes = false, spheres = false;
    float extent = 1.f;
    g.facts.forgetCounts();
    for (size_t i = 0; i < n; ++i)
    {
        float4 *r = &g.scene.hostPrims[PRIM_ROWS * i];
        for (int row : {(int)ROW_P0_TYPE, (int)ROW_P1_INDEX, (int)ROW_P2})
            for (float c : {r[row].x, r[row].y, r[row].z})
                if (fabsf(c) < 3.0e38f) /* (a comparison with NaN is false: the extent stays a number) */
                    extent = std::max(extent, fabsf(c));
        int tag, mat;
        memcpy(&tag, &r[ROW_P0_TYPE].w, 4);
        memcpy(&mat, &r[ROW_SIZE_MAT].w, 4);
        const int type = tag & PRIM_TYPE_MASK;
        /* a material that was never uploaded reads as all zeros on the device */
        const int facts = (mat >= 0 && (size_t)mat < g.materials.materialTags.size()) ? g.materials.materialTags[mat]
                                                                                      : (PRIM_FAST0 | (1 << PRIM_WIDTH_SHIFT));
        /* the kind, and what the primitive says about the scene - contained, opaque to shadows, features -: engine.h */
        const int retagged = primitiveTag(type, facts, noKinds);
        const int kind = (retagged >> PRIM_KIND_SHIFT) & 15;
        r[ROW_P0_TYPE].w = bitsf(retagged);
        planes = planes || kind == KIND_PLANE_XY || kind == KIND_PLANE_YZ || kind == KIND_PLANE_XZ;
        spheres = spheres || kind == KIND_SPHERE;
        g.facts.count(type, facts, +1);
        r[ROW_P2].w = (mat >= 0 && (size_t)mat < g.materials.materialAverage.size()) ? g.materials.materialAverage[mat] : 0.f;
    }
    /* |p0| + |size| of the largest primitive, at least: the scale the thin leaves' margin is a 2^-10 of */
    float reach = 0.f;
    for (size_t i = 0; i < n; ++i)
        for (float c : {g.scene.hostPrims[PRIM_ROWS * i + ROW_SIZE_MAT].x, g.scene.hostPrims[PRIM_ROWS * i + ROW_SIZE_MAT].y,
                        g.scene.hostPrims[PRIM_ROWS * i + ROW_SIZE_MAT].z})
            if (fabsf(c) < 3.0e38f)
                reach = std::max(reach, fabsf(c));
    g.facts.sceneExtent = extent + reach;
    g.facts.plainPlanes = planes;
    /* ... and is a leaf of nothing but such spheres boxed larger than they are?  (The reference's builder does that to the
     * lamps' cell alone; every list has the leaves of the reference's.)  Only then is a thin copy worth making for them. */
    bool loose = false;
    const std::vector<float4> &rows = g.scene.exact.rows;
    const std::vector<int> &start = g.scene.exact.start;
    for (size_t i = 0; spheres && !loose && i < start.size() && 2 * i + 1 < rows.size(); ++i)
    {
        const float4 a = rows[2 * i], b = rows[2 * i + 1];
        const int count = bitsi(b.z);
        if (count <= 0 || start[i] < 0 || (size_t)start[i] + (size_t)count > n)
            continue;
        bool all = true;
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = 0; k < count && all; ++k)
        {
            const float4 p = g.scene.hostPrims[PRIM_ROWS * ((size_t)start[i] + k) + ROW_P0_TYPE];
            const float r = fabsf(g.scene.hostPrims[PRIM_ROWS * ((size_t)start[i] + k) + ROW_SIZE_MAT].x);
            all = ((bitsi(p.w) >> PRIM_KIND_SHIFT) & 15) == KIND_SPHERE;
            lo[0] = std::min(lo[0], p.x - r), lo[1] = std::min(lo[1], p.y - r), lo[2] = std::min(lo[2], p.z - r);
            hi[0] = std::max(hi[0], p.x + r), hi[1] = std::max(hi[1], p.y + r), hi[2] = std::max(hi[2], p.z + r);
        }
        loose = all && (a.x < lo[0] || a.y < lo[1] || a.z < lo[2] || b.x > hi[0] || b.y > hi[1] || a.w > hi[2]);
    }
    g.facts.looseSpheres = loose;
    /* (for the viewDistance of the frame prepared last, so that a host which uploads every frame has the copies made once;
     * a frame with another one has them made again: prepareScene) */
    g.facts.thinReach = thinReachWanted(g.facts.frameViewDistance);
    g.facts.deriveFromCounts(); /* sceneFeatures, primsContained, opaqueShadows */
    g.scene.retagged();
    g.scene.arena.layOutAgain();
}

/* The texel fetch (rt_device.h fetchTexel, skyboxMapping) indexes the atlas with textureOffset + index % texels
 * and reads three bytes, for the diffuse map and, at the same index, for every secondary map of the
 * material.  The reference reads whatever lies there when the tables and the atlas disagree; on this
 * device that is a memory fault which ends the process's use of the GPU.  So the tables are checked against
 * the atlas once after either was uploaded, and a frame with a material that points outside is refused. */
void checkTextureTables()
{
    if (g.textures.textureTablesChecked)
        return;
    g.textures.textureTablesChecked = true;
    for (const TextureUse &use : g.materials.textureUses)
    {
        ARGCHECK(use.texels > 0, "cudaRender: a textured material with an empty or negative texture mapping");
        ARGCHECK(g.textures.atlas.ptr != nullptr && g.textures.atlasBytes > 0,
                 "cudaRender: textured materials but no texture atlas was uploaded (h2d_textures)");
        for (int t = 0; ok() && t < 7; ++t)
            if (use.offsets[t] >= 0 || t == 0)
                ARGCHECK(use.offsets[t] >= 0 && (size_t)(use.offsets[t] + use.texels + 2) <= g.textures.atlasBytes,
                         "cudaRender: a material's texture table points outside the uploaded atlas");
        if (!ok())
        {
            g.textures.textureTablesChecked = false; /* checked again once the caller has uploaded something else */
            return;
        }
    }
}


void h2dSceneOne(BoundingBox *boundingBoxes, int nbActiveBoxes, Primitive *primitives, int nbPrimitives, Lamp *lamps,
                        int nbLamps)
{
    if (!ready("h2d_scene"))
        return;
    quiesce();
    ARGCHECK(nbActiveBoxes >= 0 && nbPrimitives >= 0 && nbLamps >= 0, "h2d_scene: negative count");
    ARGCHECK(nbActiveBoxes == 0 || boundingBoxes, "h2d_scene: null boxes");
    ARGCHECK(nbPrimitives == 0 || primitives, "h2d_scene: null primitives");
    if (!ok())
        return;
    PhaseTimer phase;
    std::vector<float4> boxes(2 * (size_t)nbActiveBoxes);
    std::vector<int> start(nbActiveBoxes);
    for (int i = 0; i < nbActiveBoxes; ++i)
    {
        const BoundingBox &b = boundingBoxes[i];
        ARGCHECK(b.nbPrimitives >= 0 && (b.nbPrimitives == 0 || (b.startIndex >= 0 &&
                                                                  (long)b.startIndex + b.nbPrimitives <= nbPrimitives)),
                 "h2d_scene: box primitive range outside the primitive array");
        /* node record, scene_layout.h: { min.xyz, max.z } { max.xy, nbPrimitives, skip } */
        boxes[2 * i] = make_float4(b.parameters[0].x, b.parameters[0].y, b.parameters[0].z, b.parameters[1].z);
        boxes[2 * i + 1] =
            make_float4(b.parameters[1].x, b.parameters[1].y, bitsf(b.nbPrimitives), bitsf(b.indexForNextBox.x));
        start[i] = b.startIndex;
    }
    if (!ok())
        return;
    phase.mark("h2d_scene: node rows");
    const int nested = validateNesting(boundingBoxes, nbActiveBoxes);
    phase.mark("h2d_scene: nesting check");
    if (!nested)
    {
        /* the general walk needs at least forward progress */
        for (int i = 0; i < nbActiveBoxes; ++i)
            ARGCHECK(boundingBoxes[i].indexForNextBox.x >= 1, "h2d_scene: skip pointer < 1");
        if (!ok())
            return;
    }

    /* the walk-order list (list_builders.cpp): chains of nodes with the same bounds collapsed ... */
    std::vector<float4> boxesC;
    std::vector<int> startC, originC;
    const int nc = collapseChains(boxes, start, nested != 0, boxesC, startC, originC, &g.scene.exact.ordered, &g.scene.walk.ordered);

    /* the order-free lists are built when the scene has stayed for a frame (maybeBuildOrderFreeLists): a host that
     * uploads the scene again for every frame - the reference's own way of animating - never pays for them */
    int freeCountdown = 0;
    if (nested && g.scene.walk.ordered && nc > 1 && g.grouping && !getenv("SOLR_HIP_NO_FREE_ORDER"))
        freeCountdown = std::max(1, getenv("SOLR_HIP_FREE_AFTER") ? atoi(getenv("SOLR_HIP_FREE_AFTER")) : 2);

    /* ... cells that do not cull pruned, siblings grouped, groups that do not cull either pruned */
    int nbWalkNodes = nc, prunedBefore = 0, prunedAfter = 0;
    if (nested && g.scene.walk.ordered && nc > 0 && g.grouping)
    {
        phase.mark("h2d_scene: chain collapse");
        nbWalkNodes = buildWalkOrderList(boxesC, startC, originC, listKnobs(), pruneDecider(), &prunedBefore, &prunedAfter,
                                         [&](const char *what) { phase.mark((std::string("h2d_scene: ") + what).c_str()); });
    }
    if (getenv("SOLR_HIP_DEBUG_TREE"))
    {
        fprintf(stderr, "solr_hip: %d nodes uploaded, %d after collapsing chains, %d in the walk list (%d + %d inner nodes that hardly cull left out)\n",
                nbActiveBoxes, nc, nbWalkNodes, prunedBefore, prunedAfter);
        if (nbWalkNodes <= 80)
            for (int i = 0; i < nbWalkNodes; ++i)
                fprintf(stderr, "  node %2d: prims %d skip %d  [%g %g %g .. %g %g %g]\n", i, bitsi(boxesC[2 * i + 1].z),
                        bitsi(boxesC[2 * i + 1].w), boxesC[2 * i].x, boxesC[2 * i].y, boxesC[2 * i].z,
                        boxesC[2 * i + 1].x, boxesC[2 * i + 1].y, boxesC[2 * i].w);
    }

    std::vector<float4> prims(8 * (size_t)nbPrimitives);
    for (int i = 0; i < nbPrimitives; ++i)
    {
        const Primitive &p = primitives[i];
        float4 *r = &prims[8 * (size_t)i];
        r[ROW_P0_TYPE] = make_float4(p.p0.x, p.p0.y, p.p0.z, bitsf(p.type & PRIM_TYPE_MASK));
        r[ROW_SIZE_MAT] = make_float4(p.size.x, p.size.y, p.size.z, bitsf(p.materialId));
        r[ROW_P1_INDEX] = make_float4(p.p1.x, p.p1.y, p.p1.z, bitsf(p.index));
        r[ROW_P2] = make_float4(p.p2.x, p.p2.y, p.p2.z, 0.f);
        r[ROW_N0] = make_float4(p.n0.x, p.n0.y, p.n0.z, p.vt0.x);
        r[ROW_N1] = make_float4(p.n1.x, p.n1.y, p.n1.z, p.vt0.y);
        r[ROW_N2] = make_float4(p.n2.x, p.n2.y, p.n2.z, p.vt1.x);
        r[ROW_UV] = make_float4(p.vt1.y, p.vt2.x, p.vt2.y, 0.f);
    }
    if (prims.empty())
        prims.assign(8, make_float4(0.f, 0.f, 0.f, 0.f)); /* inactive lanes read record 0 */
    phase.mark("h2d_scene: primitive rows");
    g.scene.exact.rows.swap(boxes);
    g.scene.exact.start.swap(start);
    g.scene.exact.nb = nbActiveBoxes;
    g.scene.walk.rows.swap(boxesC);
    g.scene.walk.start.swap(startC);
    g.scene.walk.origin.swap(originC);
    g.scene.walk.nb = nbWalkNodes;
    g.scene.hostPrims.swap(prims);
    /* the lamp's cut-off of the shadow walks rests on this (lampCutoffUsable): another host's boxes are taken at their
     * word only after the check */
    const bool encloses = nested && g.scene.walk.ordered && nbWalkNodes > 0 &&
                          listEnclosesOnHost(g.scene.walk.rows, g.scene.walk.start, g.scene.hostPrims);
    g.scene.newGeometry(nested, encloses, freeCountdown);
    phase.mark("h2d_scene: enclosure check");
    retagPrimitives();
    phase.mark("h2d_scene: tags");
    HIPCHECK(hipSetDevice(g.device));
    std::vector<int> l(lamps, lamps + (lamps ? nbLamps : 0));
    upload(g.scene.lamps, l);
    if (ok())
    {
        g.scene.nbPrimitives = nbPrimitives;
        g.scene.nbLamps = nbLamps;
        ++g.bank.nbUploads;
    }
}

/* Extension: per flattened primitive, whether GPUKernel::rotatePrimitives would move it (it sits in a
 * level-0 box, is movable and is not the camera primitive).  Valid until the next h2d_scene. */
void setMovableOne(const unsigned char *flags, int nbPrimitives)
{
    if (!ready("solr_hip_set_movable"))
        return;
    ARGCHECK(nbPrimitives >= 0 && (nbPrimitives == 0 || flags), "solr_hip_set_movable: null flags");
    if (!ok())
        return;
    g.scene.refit.nbMovable = -1;
    if (nbPrimitives != g.scene.nbPrimitives)
        return;
    quiesce();
    HIPCHECK(hipSetDevice(g.device));
    std::vector<unsigned char> f(flags, flags + nbPrimitives);
    if (f.empty())
        f.push_back(0);
    upload(g.scene.refit.movable, f);
    if (ok())
        g.scene.refit.nbMovable = nbPrimitives;
}

/* One material of the table as the device gets it - h2dMaterialsOne for every active one, editMaterialsOne
 * (solr_materials.hip) to see which of them an edit changed. */
MaterialRecord materialRecord(const Material &material, int i, MaterialHot &h, MaterialCold &c)
{
    Material m = material;
    MaterialRecord record;
    /* A diffuse texture id that was never loaded: GPUKernel::setMaterial then leaves the "computed texture"
     * mapping (40000 x 40000 at offset 0, GPUKernel.cpp:1893-1896) next to the id, and the mappers would
     * index gigabytes past the atlas (the reference reads whatever is there; a memory fault here).  Such a
     * material is untextured on the device. */
    if (m.textureIds.x >= 0 && m.textureMapping.x == 40000 && m.textureMapping.y == 40000 && m.textureOffset.x == 0)
        m.textureIds.x = TEXTURE_NONE;
    record.facts = materialTag(m);
    /* the mappers fetch only for 0 <= u < mapping.x (rt_device.h): a mapping without columns - what
     * realignTexturesAndMaterials gives a material whose texture nobody loaded - never reaches the atlas */
    record.textured = m.textureIds.x >= 0 && m.textureMapping.x > 0; /* procedural ids (Mandelbrot, Julia) are negative */
    record.use = TextureUse();
    if (record.textured)
    {
        TextureUse &use = record.use;
        use.material = i;
        use.texels = (long)m.textureMapping.x * (long)m.textureMapping.y * (long)m.textureMapping.w;
        if (m.textureMapping.y <= 0 || m.textureMapping.w <= 0 || m.textureOffset.x < 0)
            use.texels = 0; /* fetchTexel takes an index modulo this: refused by checkTextureTables */
        const int ids[7] = {m.textureIds.x, m.textureIds.y, m.textureIds.z, m.textureIds.w,
                            m.advancedTextureIds.x, m.advancedTextureIds.y, m.advancedTextureIds.z};
        const int offs[7] = {m.textureOffset.x, m.textureOffset.y, m.textureOffset.z, m.textureOffset.w,
                             m.advancedTextureOffset.x, m.advancedTextureOffset.y, m.advancedTextureOffset.z};
        for (int t = 0; t < 7; ++t)
            use.offsets[t] = ids[t] != TEXTURE_NONE ? (long)offs[t] : -1L;
    }
    record.average = (m.color.x + m.color.y + m.color.z) / 3.f; /* same expression, same rounding */
    h.innerIllumination = make_float4(m.innerIllumination.x, m.innerIllumination.y, m.innerIllumination.z,
                                      m.innerIllumination.w);
    h.color = make_float4(m.color.x, m.color.y, m.color.z, m.color.w);
    h.specular = make_float4(m.specular.x, m.specular.y, m.specular.z, m.specular.w);
    h.reflection = m.reflection;
    h.refraction = m.refraction;
    h.transparency = m.transparency;
    h.opacity = m.opacity;
    h.attributes = make_int4(m.attributes.x, m.attributes.y, m.attributes.z, m.attributes.w);
    h.ids = make_int4(m.textureIds.x, m.advancedTextureIds.z, 0, 0);
    c.textureMapping = make_int4(m.textureMapping.x, m.textureMapping.y, m.textureMapping.z, m.textureMapping.w);
    c.textureOffset = make_int4(m.textureOffset.x, m.textureOffset.y, m.textureOffset.z, m.textureOffset.w);
    c.textureIds = make_int4(m.textureIds.x, m.textureIds.y, m.textureIds.z, m.textureIds.w);
    c.advancedTextureOffset = make_int4(m.advancedTextureOffset.x, m.advancedTextureOffset.y,
                                        m.advancedTextureOffset.z, m.advancedTextureOffset.w);
    c.advancedTextureIds = make_int4(m.advancedTextureIds.x, m.advancedTextureIds.y, m.advancedTextureIds.z,
                                     m.advancedTextureIds.w);
    c.mappingOffset = make_float2(m.mappingOffset.x, m.mappingOffset.y);
    c.pad = make_float2(0.f, 0.f);
    return record;
}

void h2dMaterialsOne(Material *materials, int nbActiveMaterials)
{
    if (!ready("h2d_materials"))
        return;
    quiesce();
    ARGCHECK(nbActiveMaterials >= 0 && (nbActiveMaterials == 0 || materials), "h2d_materials: bad arguments");
    if (!ok())
        return;
    /* always NB_MAX_MATERIALS + 1 records on the device (zero beyond the
     * active ones) so that every id a primitive or the box-debug view can
     * produce stays inside the allocation */
    const int capacity = NB_MAX_MATERIALS + 1;
    const int active = std::min(nbActiveMaterials, capacity);
    /* (only the active records are built and copied: the 12.6 MB of the full table took 10 ms per call, and the
     * reference's hosts call this whenever one material changes) */
    std::vector<MaterialHot> hot((size_t)std::max(active, 1));
    std::vector<MaterialCold> cold((size_t)std::max(active, 1));
    memset(hot.data(), 0, hot.size() * sizeof(MaterialHot));
    memset(cold.data(), 0, cold.size() * sizeof(MaterialCold));
    g.materials.materialTags.assign(capacity, PRIM_FAST0 | (1 << PRIM_WIDTH_SHIFT));
    g.materials.materialAverage.assign(capacity, 0.f);
    g.materials.textureUses.clear();
    g.materials.nbImaged = -1; /* (the image is this call's records once they have landed) */
    g.textures.textureTablesChecked = false;
    ++g.materials.generation; /* (a parked scene keeps the tags of the table it was parked under: solr_bank.hip) */
    for (int i = 0; i < nbActiveMaterials && i < capacity; ++i)
    {
        const MaterialRecord record = materialRecord(materials[i], i, hot[i], cold[i]);
        g.materials.materialTags[i] = record.facts;
        if (record.textured)
            g.materials.textureUses.push_back(record.use);
        g.materials.materialAverage[i] = record.average;
    }
    HIPCHECK(hipSetDevice(g.device));
    const size_t tableBytes = 12 * (size_t)capacity * sizeof(float4);
    const bool fresh = !g.materials.table.ptr || g.materials.table.bytes < tableBytes;
    reserve(g.materials.table, tableBytes);
    if (!ok())
        return;
    char *table = (char *)g.materials.table.ptr;
    const size_t coldAt = 6 * (size_t)capacity * sizeof(float4);
    /* zeros beyond the active records: the whole table when it is new, else what the last call left behind */
    const int stale = fresh ? capacity : std::min(std::max(g.materials.nbMaterials, 0), capacity);
    if (fresh)
        HIPCHECK(hipMemsetAsync(table, 0, tableBytes, sceneStream()));
    else if (stale > active)
    {
        HIPCHECK(hipMemsetAsync(table + (size_t)active * sizeof(MaterialHot), 0, (size_t)(stale - active) * sizeof(MaterialHot),
                                sceneStream()));
        HIPCHECK(hipMemsetAsync(table + coldAt + (size_t)active * sizeof(MaterialCold), 0,
                                (size_t)(stale - active) * sizeof(MaterialCold), sceneStream()));
    }
    if (active > 0)
    {
        HIPCHECK(hipMemcpyAsync(table, hot.data(), (size_t)active * sizeof(MaterialHot), hipMemcpyHostToDevice, sceneStream()));
        HIPCHECK(hipMemcpyAsync(table + coldAt, cold.data(), (size_t)active * sizeof(MaterialCold), hipMemcpyHostToDevice,
                                sceneStream()));
    }
    HIPCHECK(hipStreamSynchronize(sceneStream())); /* pageable sources: complete for the caller when this returns */
    if (ok())
    {
        g.materials.offMatCold = 6u * (unsigned)capacity;
        g.materials.nbMaterials = nbActiveMaterials;
        /* what the table holds now, for the next edit to be compared with (editMaterialsOne) */
        g.materials.imageHot.swap(hot);
        g.materials.imageCold.swap(cold);
        g.materials.nbImaged = active;
        retagPrimitives();
    }
}

static void noteRandomsReach(const std::vector<float> &r)
{
    /* the ambient-occlusion taps read randoms[i] and randoms[i + 100], i < 256 (CRT:1146-1153) */
    float reach = 0.f;
    for (size_t i = 0; i < r.size() && i < 356; ++i)
        reach = std::max(reach, fabsf(r[i]));
    g.randoms.randomsReach = reach;
}

static void uploadRandoms(const float *randoms, long count, const char *who)
{
    if (ready(who))
    {
        quiesce();
        std::vector<float> r(randoms, randoms + count);
        HIPCHECK(hipSetDevice(g.device));
        upload(g.randoms.values, r);
        if (ok())
            g.randoms.nbRandoms = count;
        noteRandomsReach(r);
    }
    /* with a communicator rank 0's buffer is everybody's: every rank ends its upload here, in whatever state */
    shareRandoms();
}

void h2dRandomsOne(float *randoms)
{
    if (g.initialized && ok())
        ARGCHECK(randoms != nullptr, "h2d_randoms: null buffer");
    uploadRandoms(randoms, MAX_BITMAP_SIZE, "h2d_randoms");
}

/* Frames larger than the reference's 1920 x 1080 limit: its natural depth of field indexes the buffer with
 * `pixel index + timestamp % (MAX_BITMAP_SIZE - 2)` (CRT:475, the precedence as written), i.e. up to
 * W * H + 9999 + 1 - beyond MAX_BITMAP_SIZE floats as soon as the frame is larger (and by up to 9 999 floats
 * even at that size).  A host that renders such frames hands over as many values
 * as the expression can reach; reads beyond what was handed over return 0 (rt_device.h rnd()). */
void h2dRandomsSizedOne(const float *randoms, long count)
{
    if (g.initialized && ok())
        ARGCHECK(randoms != nullptr && count >= MAX_BITMAP_SIZE && count <= (1L << 30),
                 "solr_hip_h2d_randoms_sized: needs at least MAX_BITMAP_SIZE values");
    uploadRandoms(randoms, count, "solr_hip_h2d_randoms_sized");
}

void h2dTexturesOne(int activeTextures, TextureInfo *textureInfos)
{
    if (!ready("h2d_textures"))
        return;
    quiesce();
    ARGCHECK(activeTextures >= 0 && (activeTextures == 0 || textureInfos), "h2d_textures: bad arguments");
    for (int i = 0; ok() && i < activeTextures; ++i)
        if (textureInfos[i].buffer)
            ARGCHECK(textureInfos[i].offset >= 0 && textureInfos[i].size.x >= 0 && textureInfos[i].size.y >= 0 &&
                         textureInfos[i].size.z >= 0 &&
                         (double)textureInfos[i].size.x * textureInfos[i].size.y * textureInfos[i].size.z < 2147483648.0,
                     "h2d_textures: a texture with a negative offset or size, or larger than 2 GB");
    if (!ok())
        return;
    size_t total = 0, largest = 0;
    for (int i = 0; i < activeTextures; ++i)
        if (textureInfos[i].buffer)
        {
            size_t sz = (size_t)textureInfos[i].size.x * textureInfos[i].size.y * textureInfos[i].size.z;
            size_t end = (size_t)textureInfos[i].offset + sz;
            total = end > total ? end : total;
            largest = sz > largest ? sz : largest;
        }
    /* Slack: a texel fetch reads index .. index+2, and the secondary maps of a material (normal, bump,
     * specular ...) are read at the texel index of its DIFFUSE texture (TextureMapping.cuh:30-116): a map
     * smaller than the diffuse texture is read up to `largest` bytes past its own end.  Inside the atlas that
     * is the next texture, as in the reference; past the atlas the reference reads whatever follows its
     * buffer - here zeros, always. */
    std::vector<unsigned char> atlas(total + largest + 4, 0);
    for (int i = 0; i < activeTextures; ++i)
        if (textureInfos[i].buffer)
        {
            size_t sz = (size_t)textureInfos[i].size.x * textureInfos[i].size.y * textureInfos[i].size.z;
            memcpy(atlas.data() + textureInfos[i].offset, textureInfos[i].buffer, sz);
        }
    HIPCHECK(hipSetDevice(g.device));
    upload(g.textures.atlas, atlas);
    g.textures.atlasBytes = ok() ? atlas.size() : 0;
    g.textures.textureTablesChecked = false;
}

void h2dLightInformationOne(LightInformation *lightInformation, int lightInformationSize)
{
    if (!ready("h2d_lightInformation"))
        return;
    quiesce();
    ARGCHECK(lightInformationSize >= 0 && (lightInformationSize == 0 || lightInformation),
             "h2d_lightInformation: bad arguments");
    if (!ok())
        return;
    std::vector<float4> l(3 * (size_t)lightInformationSize);
    for (int i = 0; i < lightInformationSize; ++i)
    {
        const LightInformation &s = lightInformation[i];
        l[3 * i] = make_float4(s.location.x, s.location.y, s.location.z, bitsf(s.primitiveId));
        l[3 * i + 1] = make_float4(s.color.x, s.color.y, s.color.z, s.color.w);
        l[3 * i + 2] = make_float4(bitsf(s.materialId), 0.f, 0.f, 0.f);
    }
    g.lights.hostLights.swap(l);
    g.scene.arena.layOutAgain();
    g.lights.nbLights = lightInformationSize;
}

} // namespace solreng

extern "C" {
/* Diagnostics / tests: the resident arena's node lists and primitive records as the device holds them
 * now.  exact != 0: the reference's list, else the walk-order list.  Returns the number of float4 rows
 * written (2 per node, 8 per primitive), -1 if the capacity is too small. */
int solr_hip_read_nodes(int exact, float *rows, int capacityRows)
{
    if (!ready("solr_hip_read_nodes") || !g.scene.arena.geometry.ptr)
        return -1;
    flushGeometry();
    if (exact)
        refreshExactList();
    quiesce();
    const NodeList &list = exact ? g.scene.exact : g.scene.walk;
    int n = 2 * list.nb;
    unsigned at = list.offRows;
    if (exact >= 2) /* 2 ... 9: the order-free list of octant exact - 2 (0 rows when there are none) */
    {
        const bool have = exact <= 9 && g.scene.orderFree.nb > 0 && !g.scene.lists.freeStale;
        n = have ? 2 * g.scene.orderFree.nb : 0;
        at = g.scene.orderFree.rowsOf(exact - 2);
    }
    if (!rows)
        return n; /* size query */
    if (n > capacityRows)
        return -1;
    if (n)
        HIPCHECK(hipMemcpy(rows, (const char *)g.scene.arena.geometry.ptr + (size_t)at * 16, (size_t)n * 16, hipMemcpyDeviceToHost));
    return ok() ? n : -1;
}

int solr_hip_read_primitives(float *rows, int capacityRows)
{
    if (!ready("solr_hip_read_primitives") || !g.scene.arena.geometry.ptr)
        return -1;
    flushGeometry();
    quiesce();
    const int n = PRIM_ROWS * g.scene.nbPrimitives;
    if (!rows)
        return n;
    if (n > capacityRows)
        return -1;
    if (n)
        HIPCHECK(hipMemcpy(rows, (const char *)g.scene.arena.geometry.ptr + (size_t)g.scene.arena.offPrims * 16, (size_t)n * 16,
                           hipMemcpyDeviceToHost));
    return ok() ? n : -1;
}

} // extern "C"
