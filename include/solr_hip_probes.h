/*
 * solr_hip_probes.h - TEST-ONLY entry points of libsolr_hip.so (sol-r_amd/csrc/solr_probes.hip).
 *
 * Not part of the drop-in boundary (include/solr_hip.h) and not used by the product: they exist so that the
 * engine's OWN device functions - the slab test in its three forms (the reference's compare chain, the sign-free
 * form, the hand-scheduled node loop), the primitive tests as both walks dispatch them, the two walks themselves
 * over the resident scene, primitiveShader, refraction / reflection, makeColor, skyboxMapping, intersectionShader with
 * the texture mappers, the post-processing kernels - can be evaluated once per element of arrays of inputs, the arrays that oracle/ref_probes.cl feeds to
 * THE REFERENCE'S OWN functions (RayTracer.cl:847-874, 1151-1394, 1528-1591 ...), and compared with the reference's
 * outputs bit for bit WITH NO ORACLE IN BETWEEN (tests/test_engine_probes_gpu.py against
 * tests/golden/reference_probes.npz).  Every kernel calls the very functions the renderer is built from
 * (rt_device.h), in the instantiation the renderer would launch for the resident scene.
 *
 * Vectors are packed xyz floats.  `features`: 0 = the instantiation renderImpl would pick for the resident scene
 * and this SceneInfo (enum Feature of rt_device.h, F_DEEP for a list of more than 1 024 nodes), or one of the
 * masks this file instantiates.  Every function returns the mask it ran (> 0), or -1 with solr_hip_last_error set.
 * The scene probes need a resident scene (h2d_scene / h2d_materials ..., or a frame rendered through the host
 * protocol); `exactNodes` != 0 walks the reference's own node list instead of the engine's walk-order list.
 */
#ifndef SOLR_HIP_PROBES_H
#define SOLR_HIP_PROBES_H

#include "solr_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* boxIntersection (GI:52-79) behind computeRayAttributes (GI:36-44), element i = box i against ray i:
 * hitExact - the reference's compare chain (rt_device.h boxIntersectionExact); hitFast - the sign-free form
 * (boxIntersectionFast), -1 where the ray does not meet its precondition (finiteRay) */
int solr_hip_probe_box(int n, const BoundingBox *boxes, const float *origins, const float *directions, const float *t0,
                       const float *t1, int *hitExact, int *hitFast);

/* the hand-scheduled node loop (rt_device.h advanceTidy): the resident scene is a flat list of n leaf boxes; ray i
 * walks the whole list with far distance t1[i] (the loop's near distance is 0, as in both walks) and hit[i] says
 * whether it entered leaf i */
int solr_hip_probe_box_walk(const SceneInfo *sceneInfo, int n, const float *origins, const float *directions,
                            const float *t1, int features, int *hit);

/* one primitive test as the closest-hit walk (GI:712-747) or, shadows[i] != 0, the shadow walk (GI:835-864)
 * dispatches it (rt_device.h testPrimitive): element i = primitive i of the resident scene against ray i.
 * intersection / normal are in/out (the walks hand the tests whatever their locals held). */
int solr_hip_probe_primitive(const SceneInfo *sceneInfo, int n, const float *origins, const float *directions,
                             const int *shadows, int features, float *intersection, float *normal, float *areas,
                             float *shadowIntensity, int *hit);

/* intersectionWithPrimitives (GI:667-772; rt_device.h closestHitWalk) over the resident scene, 64 rays per wave */
int solr_hip_probe_closest(const SceneInfo *sceneInfo, int n, const float *origins, const float *targets,
                           const int *iteration, const int *currentMaterialId, int features, int exactNodes, int *hit,
                           int *primitive, float *intersection, float *normal, float *areas);

/* processShadows (GI:798-908; rt_device.h shadowWalk): lightId is the lamp's Primitive.index, objectId the shaded
 * primitive's (both left out of the walk, GI:829; pass an index nobody has to leave out the lamp only) */
int solr_hip_probe_shadow(const SceneInfo *sceneInfo, int n, const float *lampCenters, const float *origins,
                          const int *lightId, const int *objectId, const int *iteration, int features, int exactNodes,
                          float *result, float *color);

/* primitiveShader (GI:916-1080; rt_device.h primitiveShader) with the resident scene, lights and random buffer: element i
 * shades primitive objectId[i] (index into the flattened array) at intersections[i] as bounce iteration[i] of pixel
 * index[i], seen from origins[i].  normal, closestColor, totalBlinn (3 per element) and attributes (4) are in/out, as
 * in the reference (they persist across bounces); returned 3, shadowIntensity 1 per element.  Lamp 0's shadow rays walk
 * the resident node list (exactNodes as above). */
int solr_hip_probe_shader(const SceneInfo *sceneInfo, int n, const int *index, const float *origins, const int *objectId,
                          const float *intersections, const float *areas, const int *iteration, int features, int exactNodes,
                          float *normal, float *closestColor, float *totalBlinn, float *attributes, float *returned,
                          float *shadowIntensity);

/* The same call with the records of the hit handed over the way launchRayTracing hands them to the shader (rt_device.h
 * HitRecords): per lane the material id, the index word and the material's hot half of the shaded primitive (record 0's for
 * a negative material id, as the trace loads it), `given` by the trace's own ballot (a lane that shades a primitive with a
 * negative material id sends its wave back to the shader's own gather), in the instantiation the renderer's kernel
 * runs (F_ARGS where its trace sets it).  Returns the features, with
 * SOLR_HIP_PROBE_HANDS_OVER set where that instantiation takes the records (handsOverHit); in the others the shader gathers
 * them itself as in solr_hip_probe_shader. */
#define SOLR_HIP_PROBE_HANDS_OVER (1 << 30)
int solr_hip_probe_shader_given(const SceneInfo *sceneInfo, int n, const int *index, const float *origins, const int *objectId,
                                const float *intersections, const float *areas, const int *iteration, int features,
                                int exactNodes, float *normal, float *closestColor, float *totalBlinn, float *attributes,
                                float *returned, float *shadowIntensity);

/* the post-processing stage of cudaRender (CRT:1857-1890) over a frame buffer of the caller's (sceneInfo.size pixels):
 * k_depthOfField / k_ambientOcclusion / k_radiosity / k_filter / k_cartoon exactly as renderImpl launches them behind the
 * renderer, or, for ppe_none, the stand-alone k_default (CRT:1057-1073: the conversion the renderer otherwise fuses into
 * its epilogue).  The random buffer is the resident one (h2d_randoms).  bitmap: 3 bytes per pixel. */
int solr_hip_probe_postprocess(const SceneInfo *sceneInfo, const PostProcessingInfo *postProcessingInfo,
                               const PostProcessingBuffer *frame, unsigned char *bitmap);

/* The read-back tickets of solr_hip_d2h_image_async (include/solr_hip.h): the ticket the serial-th frame of a process
 * gets - never negative (0 once a period): (serial mod period) x ring + slot - with its slot and the period (no GPU needed); and
 * the engine's serial counter, returned, and set first when setTo >= 0 (to put a running engine just before 2^31 / 6
 * tickets - 27 hours of frames - and render across) */
int solr_hip_probe_ticket(long long serial, int *slot, long long *period);
long long solr_hip_probe_image_serial(long long setTo);

/* k_orderTiles (sol-r_amd/csrc/solr_post.hip), the tile sort of the cost-ordered launch, over n tile costs of the caller's:
 * `flights` as renderImpl passes it (0: the statistics only), and the bands of a streamed frame (bands = 0: by cost alone;
 * otherwise firstTile[0 ... bands] in tiles, and the heaviest n / heavyShare tiles first).  order (n + 3 x 256 words),
 * snapshot (n) and hostStats (8) are in/out: whatever the caller put there is what the kernel did not overwrite. */
int solr_hip_probe_order_tiles(int n, const unsigned *cost, int flights, int bands, int heavyShare, const int *firstTile,
                               unsigned *order, unsigned *snapshot, unsigned *hostStats);

/* what the frame rendered last launched: {row of the renderer's table or -1, features of the instantiation (enum Feature
 * of rt_device.h with F_DEEP, F_STACK, F_STREAM) or -1, streamed (1 / 0), its bands, cost-ordered launch (1 / 0), the
 * bands of that order} */
void solr_hip_probe_last_frame(int out[6]);

/* What the arena holds of a node list, read back as it is now (pending uploads flushed, the stream idle).  list: 0 the
 * walk-order list, 1 the reference's list, 2 the eight order-free lists one behind the other.  what: 0 the node rows, 1 the
 * thin copy (solr_arena.hip k_tightenLeaves / k_tightenInner), 2 the copy with sorted bounds and the pad record behind it
 * (k_sortNodeBounds), 3 the leaf records (k_buildLeafRecords), 4 the start indices.  Returns the number of 16-byte rows
 * (of ints for what = 4) written to out, 0 where the engine holds no such copy up to date, -1 with the error set on
 * failure; out == NULL: the size alone. */
int solr_hip_probe_list_copy(int list, int what, void *out, int capacity);

/* what a walk of the resident scene would be handed for this SceneInfo (order-free lists built when they are due):
 * out = {tightLists, sortedLists, nbBoxesFree, opaqueShadows, shortRayLists, nbBoxes (SceneArgs, scene_layout.h), the thin
 * copies' margin, the scene's extent - both as float bits}.  Returns 0, or -1 with the error set. */
int solr_hip_probe_walk_offer(const SceneInfo *sceneInfo, int exactNodes, int out[8]);

/* vectorRefraction (VU:73-87) and vectorReflection (VU:61-64) */
int solr_hip_probe_vectors(int n, const float *incident, const float *normals, const float *n1, const float *n2,
                           float *refracted, float *reflected);

/* The device math stand-ins at the top of rt_device.h, one call per element, no resident scene and no feature template
 * (tests/test_math_standins_gpu.py holds them to high-precision references of tests/golden/math_standins.npz and to the
 * numpy models of tests/math_cases.py).  Element e runs in lane e mod 64 of wave e / 64, so the caller decides which 64
 * inputs share a wave - pow_f sends a whole wave to pow_general when one lane is outside its lean domain.
 * Both return 0, or -1 with solr_hip_last_error set for an unknown op, n < 1 or a null array. */
enum SolrProbeMathOp
{
    SOLR_PROBE_POW = 0,        /* pow_f(a, b) */
    SOLR_PROBE_POW_GENERAL,    /* pow_general(a, b) */
    SOLR_PROBE_SIN,            /* sin_f(a) */
    SOLR_PROBE_COS,            /* cos_f(a) */
    SOLR_PROBE_ATAN2,          /* atan2_f(a, b) */
    SOLR_PROBE_ASIN,           /* asin_f(a) */
    SOLR_PROBE_SQRT,           /* sqrt_ieee(a) */
    SOLR_PROBE_DIVIDE,         /* a / b */
    SOLR_PROBE_RECIPROCAL,     /* 1.0f / a, as makeWalkRay and normalize write it */
    SOLR_PROBE_TO_INT,         /* (int)a as the texture mappers write it; out holds the int's bits */
    SOLR_PROBE_MATH_OPS
};
int solr_hip_probe_math(int op, int n, const float *a, const float *b, float *out);

/* u, v: 3 n floats, s: n, out: 3 n (a scalar result in x, y and z zero) */
enum SolrProbeVectorOp
{
    SOLR_PROBE_V_ADD = 0,      /* u + v */
    SOLR_PROBE_V_SUB,          /* u - v */
    SOLR_PROBE_V_SCALE,        /* u * s */
    SOLR_PROBE_V_DOT,          /* dot(u, v) */
    SOLR_PROBE_V_CROSS,        /* cross(u, v) */
    SOLR_PROBE_V_LENGTH,       /* length(u) */
    SOLR_PROBE_V_NORMALIZE,    /* normalize(u) */
    SOLR_PROBE_V_DIVIDE,       /* vdivs(u, s) */
    SOLR_PROBE_V_PROJECT,      /* project(u, v) */
    SOLR_PROBE_V_REFLECTION,   /* vectorReflection(u, v) */
    SOLR_PROBE_VECTOR_OPS
};
int solr_hip_probe_vector_math(int op, int n, const float *u, const float *v, const float *s, float *out);

/* makeColor (GS:132-165) for pixel i of an image as sceneInfo.size says; bitmap: 3 n bytes */
int solr_hip_probe_make_color(const SceneInfo *sceneInfo, int n, const float *colors, unsigned char *bitmap);

/* skyboxMapping (GI:87-151) with the resident materials and textures */
int solr_hip_probe_skybox(const SceneInfo *sceneInfo, int n, const float *origins, const float *targets, float *color);

/* intersectionShader (GS:36-124) with the mappers and maps behind it, set up as primitiveShader does (GI:933-945):
 * element i = primitive i of the resident scene.  attributes (4 per element) in/out; color 4, bump 3, specular 3,
 * ambientOcclusion 1 per element */
int solr_hip_probe_intersection_shader(const SceneInfo *sceneInfo, int n, const float *intersections, const float *areas,
                                       float *attributes, float *color, float *bump, float *specular,
                                       float *ambientOcclusion);

/* The builders of the order-free lists on a nested node list of the CALLER'S (tests/list_builder_cases.py), no resident
 * scene needed: rows[n][2][4] and start[n] as list_builders.h lays a list out; prims: nbPrims primitive records of 8 rows
 * with `margin` and `dominantShare` (build_bounds.h BuildBounds), or NULL for the boxes as uploaded; threshold:
 * pruneInnerNodes'.  route 0: the host's buildFreeOrderLists, no decider, every node its own origin - NO GPU needed;
 * 1: solrBuildOrderFreeListsOnDevice (solr_lists.hip) from the host arrays with identity origins; 2: the same with
 * origin == NULL, rows, start indices and records copied to device memory first (the arena's route).  Routes 1 and 2 run
 * on solr_hip_get_device().  Returns the length of one list with *nbPruned set and the eight lists one behind the other in
 * outRows (16 floats x 8 x length), outStart and outOrigin (8 x length), each with room for 8 x capacity nodes (outRows ==
 * NULL: the length alone); 0 where the builder DECLINED (fewer than two leaves; on the device also depth or an allocation
 * - what the engine leaves to the host), nothing written and no error set; -1 with the error set for a list that is not
 * nested, records out of range or an error of the runtime's. */
int solr_hip_probe_free_lists(int route, int n, const float *rows, const int *start, const float *prims, int nbPrims, float margin,
                              double dominantShare, double threshold, int *nbPruned, float *outRows, int *outStart, int *outOrigin,
                              int capacity);

/* pruneInnerNodes (list_builders.cpp) on a nested node list of the caller's, every node its own origin.  route 0: the
 * host's decisions (no GPU needed); 1: solrPruneDecisionsOnDevice (solr_lists.hip) as the decider, *declined = 1 where it
 * left the decisions to the host (which then made them).  Returns the new node count with *nbPruned set and the list in
 * outRows / outStart / outOrigin (room for `capacity` nodes; outRows == NULL: the count alone), or -1 with the error set. */
int solr_hip_probe_prune_list(int route, int n, const float *rows, const int *start, double threshold, int *nbPruned, int *declined,
                              float *outRows, int *outStart, int *outOrigin, int capacity);

#ifdef __cplusplus
}
#endif
#endif
