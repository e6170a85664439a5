/*
 * solr_hip.hip - the C ABI of the MI355X rendering engine (include/solr_hip.h): the reference's ten entry points
 * (CudaRayTracer.h:25-67) once per in-process device, device / stream / strip selection, the life of an engine
 * (initialize_scene ... finalize_scene).  The rest of the engine's host side: engine.h (state), solr_uploads.hip,
 * solr_arena.hip, solr_rotation.hip, solr_morph.hip, solr_moves.hip, solr_edits.hip, solr_materials.hip and solr_bank.hip (the
 * resident scene: its uploads, its arena and lists, rotation, morphing, translation, lamp moves, edited primitives and materials set
 * on the device, scenes set aside and put back),
 * solr_launch.hip (a frame), solr_post.hip, solr_image_ring.hip, solr_rccl.hip, solr_diag.hip; the kernels: rt_device.h,
 * renderer_kernel.h, rows/.  gfx950 only.
 */
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <sched.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <functional>
#include <chrono>
#include <vector>

#include "../../include/solr_hip.h"
#include "rt_device.h"
#include "device_pool.h"
#include "lists_device.h"

using namespace solrdev;

#include "renderer.h"
#include "engine.h"

using namespace solreng;

namespace solreng
{
/* (the engine's state - struct Engine, one per device of this process - and the helpers every part shares: engine.h) */
Engine gFirst;
Engine *gEngines[SOLR_MAX_GPU_COUNT] = {&gFirst};
int gDevices = 1;
int gRequested = 1;
Engine *gCurrent = &gFirst;
HostProfile gHostProfile;
} // namespace solreng

/* ======================================================================= */
/* C ABI                                                                    */
/* ======================================================================= */

extern "C" {

int solr_hip_last_error(char *buf, int len)
{
    /* the first engine in trouble speaks for the process (one engine unless occupancyParameters.x asked for more) */
    const Engine *bad = &gFirst;
    for (int d = 0; d < gDevices; ++d)
        if (gEngines[d] && gEngines[d]->errorCode != 0)
        {
            bad = gEngines[d];
            break;
        }
    if (buf && len > 0)
    {
        strncpy(buf, bad->errorText.c_str(), len - 1);
        buf[len - 1] = 0;
    }
    return bad->errorCode;
}

void solr_hip_clear_error(void)
{
    for (Engine *e : gEngines)
        if (e)
        {
            e->errorCode = 0;
            e->errorText.clear();
        }
}

int solr_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

/* (for the other translation units of the library: sol-r_amd/csrc/solr_tree.hip builds on the engine's device) */
int solr_hip_get_device(void)
{
    return g.device;
}

void solr_hip_set_device(int device)
{
    g.device = device;
}

void dropExtraStreams()
{
    for (int f = 1; f < MAX_FLIGHTS; ++f)
    {
        if (g.flight[f].stream && !g.callerStreams)
            (void)hipStreamDestroy(g.flight[f].stream);
        g.flight[f].stream = nullptr;
    }
    g.callerStreams = false;
}

void solr_hip_set_flight_streams(void *const *streams, int n)
{
    quiesce();
    g.current = 0;
    if (!streams || n < 1 || !streams[0])
        return;
    if (g.ownStream && g.flight[0].stream)
        (void)hipStreamDestroy(g.flight[0].stream);
    dropExtraStreams();
    g.ownStream = false;
    for (int f = 0; f < n && f < MAX_FLIGHTS; ++f)
        g.flight[f].stream = (hipStream_t)streams[f];
    g.callerStreams = n > 1;
    if (g.initialized && g.width > 0)
        allocateFrame();
}

void solr_hip_set_stream(void *stream)
{
    quiesce();
    g.current = 0; /* a caller's stream is the only stream: one frame in flight */
    if (g.callerStreams)
        dropExtraStreams();
    hipStream_t &mine = g.flight[0].stream;
    if (g.ownStream && mine)
    {
        (void)hipStreamSynchronize(mine);
        (void)hipStreamDestroy(mine);
        g.ownStream = false;
    }
    mine = (hipStream_t)stream;
    if (!mine && g.initialized)
    {
        HIPCHECK(hipStreamCreate(&mine));
        g.ownStream = ok();
    }
}

static void synchronizeOne()
{
    if (!ready("solr_hip_synchronize"))
        return;
    HIPCHECK(hipStreamSynchronize(g.flight[0].stream));
    for (int f = 1; f < MAX_FLIGHTS; ++f)
        if (g.flight[f].stream)
            HIPCHECK(hipStreamSynchronize(g.flight[f].stream));
}

void solr_hip_set_strip(int firstRow, int nbRows)
{
    if (gDevices > 1)
    {
        /* the frame is already shared out between this process's devices (occupancyParameters.x): a strip of the
         * multi-process split on top of that is a different program */
        setError(-1, "solr_hip_set_strip: this process renders on several devices (occupancyParameters.x > 1); strips "
                     "belong to the one-process-per-GPU model", __FILE__, __LINE__);
        return;
    }
    quiesce();
    g.firstRow = nbRows >= 0 ? firstRow : 0;
    g.nbRows = nbRows >= 0 ? nbRows : -1;
    if (g.initialized && g.width > 0)
        allocateFrame();
}

void *solr_hip_device_bitmap(void)
{
    return g.boundBitmap ? g.boundBitmap : g.flight[g.current].shown().ptr;
}
void *solr_hip_device_primitive_ids(void)
{
    return g.flight[g.current].ids.ptr;
}
void *solr_hip_device_postprocessing(void)
{
    return g.flight[g.current].pp.ptr;
}
/* the strip this process renders now (solr_hip_set_strip, solr_hip_balance_strips): rows [*firstRow, *firstRow +
 * *nbRows) of the frame; the full frame reads as (0, height of the last frame or 0 before one) */
void solr_hip_get_strip(int *firstRow, int *nbRows)
{
    if (firstRow)
        *firstRow = g.nbRows >= 0 ? g.firstRow : 0;
    if (nbRows)
        *nbRows = stripRows();
}

void solr_hip_bind_device_bitmap(void *deviceBitmap)
{
    g.boundBitmap = deviceBitmap;
}

static void initializeOne(const SceneInfo &sceneInfo)
{
    if (!ok())
        return;
    solrTuneHostAllocator();
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
    {
        setError(e != hipSuccess ? (int)e : -1,
                 "initialize_scene: no HIP device available (this engine has no CPU fallback)", __FILE__, __LINE__);
        return;
    }
    ARGCHECK(g.device >= 0 && g.device < n, "initialize_scene: device index out of range");
    if (!ok())
        return;
    HIPCHECK(hipSetDevice(g.device));
    if (!g.flight[0].stream)
    {
        HIPCHECK(hipStreamCreate(&g.flight[0].stream));
        g.ownStream = ok();
        /* the other streams right away: streams are dealt to the hardware queues in creation order, and
         * streams that share a hardware queue do not overlap (measured: created after a framework had
         * made its pool of 32, both engine streams sat on one queue and frames in flight gained nothing) */
        for (int f = 1; f < MAX_FLIGHTS && ok(); ++f)
            if (!g.flight[f].stream)
                HIPCHECK(hipStreamCreate(&g.flight[f].stream));
    }
    g.initialized = ok();
    dropParkedOne(-1); /* (an engine that was up already: its bank is of the scene before) */
    g.bank.nbSwitches = g.bank.nbUploads = 0;
    g.width = sceneInfo.size.x;
    g.height = sceneInfo.size.y;
}


static void finalizeOne()
{
    gHostProfile.report();
    if (!g.initialized)
        return;
    (void)hipSetDevice(g.device);
    for (const Flight &flight : g.flight)
        if (flight.stream)
            (void)hipStreamSynchronize(flight.stream);
    collectEvents();
    g.jpeg.release(); /* JPEG frames in flight: their slots go, outstanding tickets are void */
    /* the read-back first - the copy stream is waited for before an image goes (the ring of host images is the process's:
     * it goes with engine 0, and stays when a later engine goes alone) - then the frames' buffers, the streams but
     * flight 0's, streamed frames, the launch order */
    releaseCopies();
    if (&g == &gFirst)
        gImageRing.release();
    for (Flight &flight : g.flight)
        flight.release();
    dropExtraStreams();
    g.streaming.release();
    g.sched.release();
    g.current = 0;
    for (DeviceBuffer *b : {&g.counters, &g.tileClock, &g.haloGivenAbove, &g.haloGivenBelow})
        release(*b);
    g.recording.release();
    g.haloSuppliedAbove = g.haloSuppliedBelow = 0;
    if (g.ownStream && g.flight[0].stream)
        (void)hipStreamDestroy(g.flight[0].stream);
    g.flight[0].stream = nullptr;
    g.ownStream = false;
    g.initialized = false;
    g.allocW = g.allocRows = 0;
    g.boundBitmap = nullptr;
    /* the scene: every record back to what initialize_scene finds (the knobs stay).  The staged lists go before the
     * builders' scratch */
    g.scene.lists.dropStage(true);
    dropParkedOne(-1);
    g.bank.nbSwitches = g.bank.nbUploads = 0;
    {
        SolrScratchPool &pool = solrScratchPool(); /* the builders' scratch goes with the scene */
        std::lock_guard<std::mutex> nobodyBuilding(pool.busy);
        pool.release();
    }
    g.scene.release();
    for (int &count : g.served)
        count = 0;
    g.materials.release();
    g.textures.release();
    g.randoms.release();
    g.lights = Lights();
    g.facts = SceneFacts();
    /* no hipDeviceReset: the process may share the device with torch/RCCL */
}

static void reshapeOne(const SceneInfo &sceneInfo)
{
    if (!ready("reshape_scene"))
        return;
    quiesce();
    g.jpeg.release(); /* the slots of JPEG frames in flight were cut for the size before */
    g.width = sceneInfo.size.x;
    g.height = sceneInfo.size.y;
    allocateFrame();
}


} // extern "C"

/* ======================================================================= */
/* The boundary, once per in-process device                                  */
/* ======================================================================= */
/* CudaRayTracer.h:25-67 with occupancyParameters.x honoured as the reference honours it: that many devices of THIS
 * process (clamped to the devices there are, CudaRayTracer.cu:1413-1424), every upload repeated per device
 * (:1536-1625), the frame cut into equal row strips, device d rendering strip d (:1694-1696, 1709-1815), and
 * d2h_bitmap copying every device's strip to its place in the host arrays (:1647-1672).  One device - what every
 * caller of this library but a host that edits CudaKernel.cpp:90 asks for - is engine 0 alone and nothing below adds
 * to it.  occupancyParameters.y (streams per device; the reference's arithmetic for it is broken) is
 * accepted and not used: how a device's strip is scheduled is the engine's business, like blockSize.
 * Several devices in one process and the one-process-per-GPU model (solr_hip_set_strip, solr_hip_comm_*) do not
 * combine; either refuses the other.  Neighbourhood post-processing (ambient occlusion, depth of field, radiosity,
 * filter) stays inside a device's strip here, as in the reference (the multi-process path trades the boundary rows).
 * SOLR_HIP_VIRTUAL_DEVICES=n (tests on a one-GPU box): pretend n devices, engine d on device d mod the real ones. */
namespace
{
bool gSplit = false; /* the strips of the engines are the in-process split's */
int gAskNext = 1;    /* solr_hip_set_gpu_count: what solr_hip_initialize (the pointer form) asks for */

int devicesThereAre()
{
    int real = 0;
    if (hipGetDeviceCount(&real) != hipSuccess)
        real = 0;
    /* (read at every initialize_scene, not once per process: a test that sets it must be able to take it away again) */
    const char *const env = getenv("SOLR_HIP_VIRTUAL_DEVICES");
    const int pretend = env ? atoi(env) : 0;
    return (real > 0 && pretend > real) ? pretend : real;
}

/* engines 0 ... n - 1 exist; the later ones take the settings of engine 0 and the devices that follow its device */
void ensureEngines(int n)
{
    int real = 0;
    if (hipGetDeviceCount(&real) != hipSuccess || real < 1)
        real = 1;
    for (int d = 1; d < n && d < SOLR_MAX_GPU_COUNT; ++d)
    {
        if (!gEngines[d])
            gEngines[d] = new Engine;
        Engine &e = *gEngines[d];
        e.device = (gFirst.device + d) % real;
        e.variant = gFirst.variant;
        e.shortRayListsMode = gFirst.shortRayListsMode;
        e.grouping = gFirst.grouping;
        e.flights = gFirst.flights;
        e.sched.mode = gFirst.sched.mode;
        e.timing = gFirst.timing;
        e.bank.limitBytes = gFirst.bank.limitBytes;
    }
}

/* equal row strips, device d the d-th (the split of solr_hip_strip_rows, what the multi-process path uses too) */
void splitRows(int height)
{
    if (gDevices < 2)
    {
        if (gSplit)
        {
            gSplit = false;
            quiesce();
            gFirst.firstRow = 0;
            gFirst.nbRows = -1;
        }
        return;
    }
    gSplit = true;
    onEveryDevice([&](int d) {
        int first = 0, count = 0;
        solr_hip_strip_rows(d, gDevices, height, &first, &count, nullptr);
        if (g.firstRow != first || g.nbRows != count)
        {
            quiesce();
            g.firstRow = first;
            g.nbRows = count;
        }
    });
}

/* The reference reads occupancyParameters.x anew in every call (CudaRayTracer.cu:1647-1672, 1694 ...): a host that
 * hands initialize_scene N and a later call another count gets that call on the devices that count names.  Here the
 * engines initialize_scene set up all hold the scene and their strips of the frame, so every call runs on all of them
 * whatever it says - a frame is never missing a strip - and a count that differs is noted once, not turned into a
 * sticky error that ends the process's frames. */
bool sameOccupancy(const vec2i &occ, const char *who)
{
    if (occ.x < 1 || occ.x == gRequested || (occ.x > SOLR_MAX_GPU_COUNT && gRequested == SOLR_MAX_GPU_COUNT))
        return true;
    static bool noted = false;
    if (!noted)
        fprintf(stderr, "solr_hip: %s was handed occupancyParameters.x = %d, initialize_scene %d: the %d device(s) set up then "
                        "serve this and every later call (noted once)\n", who, occ.x, gRequested, gDevices);
    noted = true;
    return true;
}

/* A request on the resident scene (rotation, morph, translation, lamp move, primitives, their materials, an edited table of
 * materials).  Every in-process device holds the scene and changes its own copy, and every copy must be able to follow
 * before any of them changes: "0: nothing was changed" then holds on several devices as well (one engine
 * declining used to leave the others rotated).  So every engine is asked first - all of them, whatever the ones before
 * said: canRefitOne makes the refit plan as it answers - and one refusal declines the request for all.  Then every engine
 * serves.  Returns 1 when all of them did, else the first status that is not 1 (a device error past the check: the
 * engine's error state says which). */
template <class Can, class Serve>
int askThenServe(Can &&can, Serve &&serve)
{
    bool all = true;
    onEveryDevice([&](int) { all = can() && all; });
    if (!all)
        return 0;
    int status = 1;
    onEveryDevice([&](int) {
        const int mine = serve();
        if (mine != 1 && status == 1)
            status = mine;
    });
    return status;
}
} // namespace

extern "C" {

void initialize_scene(vec2i occupancyParameters, SceneInfo sceneInfo, int, int, int)
{
    if (solr_hip_last_error(nullptr, 0) != 0)
        return;
    int asked = occupancyParameters.x < 1 ? 1 : occupancyParameters.x;
    if (asked > SOLR_MAX_GPU_COUNT)
        asked = SOLR_MAX_GPU_COUNT; /* CudaRayTracer.cu:1415-1416 */
    int use = asked;
    if (asked > 1)
    {
        if (communicatorUp())
        {
            setError(-1, "initialize_scene: occupancyParameters.x > 1 asks for several devices in this process, which has "
                         "joined a communicator (one process per GPU): the two do not combine", __FILE__, __LINE__);
            return;
        }
        const int have = devicesThereAre();
        if (asked > have)
        {
            /* CudaRayTracer.cu:1419-1424: "You asked for n CUDA-capable devices, but only m are available" */
            fprintf(stderr, "solr_hip: initialize_scene was asked for %d devices (occupancyParameters.x), %d are available\n",
                    asked, have);
            use = have < 1 ? 1 : have;
        }
    }
    /* engines an earlier call set up beyond what this one uses */
    for (int d = use; d < SOLR_MAX_GPU_COUNT; ++d)
        if (d > 0 && gEngines[d] && gEngines[d]->initialized)
        {
            gCurrent = gEngines[d];
            (void)hipSetDevice(g.device);
            finalizeOne();
            gCurrent = &gFirst;
        }
    gRequested = asked;
    gDevices = use;
    ensureEngines(use);
    onEveryDevice([&](int) { initializeOne(sceneInfo); });
    splitRows(sceneInfo.size.y);
}

void solr_hip_set_gpu_count(int n)
{
    gAskNext = n < 1 ? 1 : n;
}

int solr_hip_gpu_count(void)
{
    return gDevices;
}

void solr_hip_initialize(const SceneInfo *sceneInfo)
{
    vec2i occ;
    occ.x = gAskNext;
    occ.y = 1;
    initialize_scene(occ, *sceneInfo, 0, 0, 0);
}

void finalize_scene(vec2i)
{
    /* every engine that is up, whatever occupancyParameters says by now; afterwards the process is a one-device
     * process again until initialize_scene says otherwise */
    const bool several = gDevices > 1;
    for (int d = 0; d < SOLR_MAX_GPU_COUNT; ++d)
        if (gEngines[d] && gEngines[d]->initialized)
        {
            gCurrent = gEngines[d];
            if (several)
                (void)hipSetDevice(g.device);
            finalizeOne();
        }
    gCurrent = &gFirst;
    gDevices = 1;
    gRequested = 1;
    if (several)
        (void)hipSetDevice(g.device);
}

void reshape_scene(vec2i occupancyParameters, SceneInfo sceneInfo)
{
    if (!sameOccupancy(occupancyParameters, "reshape_scene"))
        return;
    splitRows(sceneInfo.size.y);
    onEveryDevice([&](int) { reshapeOne(sceneInfo); });
}

void solr_hip_reshape(const SceneInfo *sceneInfo)
{
    vec2i occ;
    occ.x = 0;
    occ.y = 1;
    reshape_scene(occ, *sceneInfo);
}

void h2d_scene(vec2i occupancyParameters, BoundingBox *boundingBoxes, int nbActiveBoxes, Primitive *primitives,
               int nbPrimitives, Lamp *lamps, int nbLamps)
{
    if (!sameOccupancy(occupancyParameters, "h2d_scene"))
        return;
    onEveryDevice([&](int) { h2dSceneOne(boundingBoxes, nbActiveBoxes, primitives, nbPrimitives, lamps, nbLamps); });
}

void h2d_materials(vec2i occupancyParameters, Material *materials, int nbActiveMaterials)
{
    if (!sameOccupancy(occupancyParameters, "h2d_materials"))
        return;
    onEveryDevice([&](int) { h2dMaterialsOne(materials, nbActiveMaterials); });
}

void h2d_randoms(vec2i occupancyParameters, float *randoms)
{
    if (!sameOccupancy(occupancyParameters, "h2d_randoms"))
        return;
    onEveryDevice([&](int) { h2dRandomsOne(randoms); });
}

void solr_hip_h2d_randoms_sized(const float *randoms, long count)
{
    onEveryDevice([&](int) { h2dRandomsSizedOne(randoms, count); });
}

void h2d_textures(vec2i occupancyParameters, int activeTextures, TextureInfo *textureInfos)
{
    if (!sameOccupancy(occupancyParameters, "h2d_textures"))
        return;
    onEveryDevice([&](int) { h2dTexturesOne(activeTextures, textureInfos); });
}

void h2d_lightInformation(vec2i occupancyParameters, LightInformation *lightInformation, int lightInformationSize)
{
    if (!sameOccupancy(occupancyParameters, "h2d_lightInformation"))
        return;
    onEveryDevice([&](int) { h2dLightInformationOne(lightInformation, lightInformationSize); });
}

void cudaRender(vec2i occupancyParameters, vec4i, SceneInfo sceneInfo, vec4i objects, PostProcessingInfo postProcessingInfo,
                vec3f origin, vec3f direction, vec4f angles)
{
    if (!sameOccupancy(occupancyParameters, "cudaRender"))
        return;
    const float o[3] = {origin.x, origin.y, origin.z};
    const float d[3] = {direction.x, direction.y, direction.z};
    const float a[4] = {angles.x, angles.y, angles.z, angles.w};
    splitRows(sceneInfo.size.y);
    /* (asynchronous: the devices render their strips side by side) */
    onEveryDevice([&](int) { renderImpl(sceneInfo, objects, postProcessingInfo, o, d, a, false, nullptr); });
}

void solr_hip_render(const SceneInfo *sceneInfo, const vec4i *objects, const PostProcessingInfo *postProcessingInfo,
                     const float origin[3], const float direction[3], const float angles[4])
{
    splitRows(sceneInfo->size.y);
    onEveryDevice([&](int) { renderImpl(*sceneInfo, *objects, *postProcessingInfo, origin, direction, angles, false, nullptr); });
}

void d2h_bitmap(vec2i occupancyParameters, SceneInfo sceneInfo, BitmapBuffer *bitmap, PrimitiveXYIdBuffer *primitivesXYIds)
{
    if (!sameOccupancy(occupancyParameters, "d2h_bitmap"))
        return;
    if (gDevices < 2)
    {
        d2hBitmapOne(sceneInfo, bitmap, primitivesXYIds, true);
        return;
    }
    /* every device's strip to its place in the host arrays (CudaRayTracer.cu:1647-1672): enqueued on all of them,
     * then waited for */
    onEveryDevice([&](int) { d2hBitmapOne(sceneInfo, bitmap, primitivesXYIds, false); });
    onEveryDevice([&](int) { d2hBitmapWait(); });
}

void solr_hip_d2h(const SceneInfo *sceneInfo, BitmapBuffer *bitmap, PrimitiveXYIdBuffer *primitivesXYIds)
{
    vec2i occ;
    occ.x = 0;
    occ.y = 1;
    d2h_bitmap(occ, *sceneInfo, bitmap, primitivesXYIds);
}

void solr_hip_synchronize(void)
{
    onEveryDevice([&](int) { synchronizeOne(); });
}

void solr_hip_set_movable(const unsigned char *flags, int nbPrimitives)
{
    onEveryDevice([&](int) { setMovableOne(flags, nbPrimitives); });
}

/* the requests on the resident scene (askThenServe) */
int solr_hip_rotate_primitives(const float center[3], const float cosAngles[3], const float sinAngles[3], float viewDistance)
{
    return askThenServe([&] { return canRotateOne(center, cosAngles, sinAngles, viewDistance); },
                        [&] { return rotatePrimitivesOne(center, cosAngles, sinAngles, viewDistance); });
}

int solr_hip_set_morph_keys(const Primitive *first, const Primitive *last, int nbPrimitives)
{
    int status = 1;
    onEveryDevice([&](int) { status = setMorphKeysOne(first, last, nbPrimitives) && status; });
    return status;
}

/* (every in-process device holds the scene and its own slots; 1 only when all of them took the key) */
int solr_hip_set_morph_track_key(int slot, const Primitive *key, const int *rankOf, int nbPrimitives)
{
    int status = 1;
    onEveryDevice([&](int) { status = setMorphTrackKeyOne(slot, key, rankOf, nbPrimitives) && status; });
    return status;
}

int solr_hip_morph_primitives(float weight, float viewDistance)
{
    const char *const who = "solr_hip_morph_primitives";
    return askThenServe([&] { return canMorphOne(MORPH_SLOT_FIRST, MORPH_SLOT_LAST, weight, viewDistance, who); },
                        [&] { return morphKeysOne(MORPH_SLOT_FIRST, MORPH_SLOT_LAST, weight, viewDistance, who); });
}

int solr_hip_morph_between(int slotA, int slotB, float weight, float viewDistance)
{
    if (slotA < 0 || slotA >= SOLR_MORPH_TRACK_MAX_KEYS || slotB < 0 || slotB >= SOLR_MORPH_TRACK_MAX_KEYS)
        return 0;
    const char *const who = "solr_hip_morph_between";
    return askThenServe([&] { return canMorphOne(slotA, slotB, weight, viewDistance, who); },
                        [&] { return morphKeysOne(slotA, slotB, weight, viewDistance, who); });
}

int solr_hip_translate_primitives(const float translation[3], float viewDistance)
{
    return askThenServe([&] { return canTranslateOne(translation, viewDistance); },
                        [&] { return translatePrimitivesOne(translation, viewDistance); });
}

int solr_hip_move_lamp(int lamp, const float center[3])
{
    return askThenServe([&] { return canMoveLampOne(lamp, center); }, [&] { return moveLampOne(lamp, center); });
}

int solr_hip_set_primitives(const SolrPrimitiveEdit *edits, const int *slots, int n, float viewDistance)
{
    return askThenServe([&] { return canSetPrimitivesOne(edits, slots, n, viewDistance); },
                        [&] { return setPrimitivesOne(edits, slots, n, viewDistance); });
}

int solr_hip_set_primitive_materials(const int *slots, const int *materialIds, int n)
{
    return askThenServe([&] { return canSetPrimitiveMaterialsOne(slots, materialIds, n); },
                        [&] { return setPrimitiveMaterialsOne(slots, materialIds, n); });
}

/* (every engine follows the edit in its own table as well as in its own copy of the scene) */
int solr_hip_edit_materials(Material *materials, int nbActiveMaterials)
{
    return askThenServe([&] { return canEditMaterialsOne(materials, nbActiveMaterials); },
                        [&] { return editMaterialsOne(materials, nbActiveMaterials); });
}
}
