/*
 * solr_launch.hip - a frame of the MI355X rendering engine: the per-pixel buffers, the launch table (which instantiation of
 * k_standardRenderer a scene and a frame get: csrc/rows), the cost-ordered launch, cudaRender's post-processing switch
 * (CudaRayTracer.cu:1694-1890) and the read-back of d2h_bitmap (:1647-1672).
 * Part of the engine's host side (engine.h); the boundary that calls into it is solr_hip.hip.  gfx950 only.
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

/* the renderer's instantiations live in the files under csrc/rows (the rows of solrrows::ROWS, renderer.h) */
namespace solrrows
{
RendererFn renderer(int count, int features, bool volume)
{
    if (volume || (features & ~(F_DEEP | F_STACK | F_STREAM)) == F_ALL)
        return (features & (F_STACK | F_STREAM)) ? nullptr : everything(count, features, volume);
    RendererFn fn = nullptr;
    if (!(fn = spherePlane(count, features)) && !(fn = sphereTriangle(count, features)) && !(fn = sphereCylinder(count, features)) &&
        !(fn = untexturedMix(count, features)) && !(fn = textured(count, features)))
        fn = specialCameras(count, features);
    return fn;
}
WalkBoundFn walkBound(int row, int features)
{
    switch (row)
    {
    case 0: return walkBoundRow0(features);
    case 1: return walkBoundRow1(features);
    case 2: return walkBoundRow2(features);
    case 3: return walkBoundRow3(features);
    default: return nullptr;
    }
}
} // namespace solrrows

namespace solreng
{
void allocateFrame()
{
    const int rows = stripRows();
    const size_t pixels = (size_t)std::max(g.width, 1) * (size_t)std::max(rows, 1);
    /* the sets in use: flight 0's whatever happens, the others' as far as frames may be in flight */
    const int sets = g.flights >= 2 && (g.ownStream || g.callerStreams) ? std::min(g.flights, MAX_FLIGHTS) : 1;
    bool fresh = g.allocW != g.width || g.allocRows != rows;
    for (int f = 0; f < sets && (f == 0 || ok()); ++f)
    {
        Flight &set = g.flight[f];
        if (f && !set.stream)
        {
            if (g.callerStreams)
                break; /* the caller gave fewer streams */
            HIPCHECK(hipStreamCreate(&set.stream));
        }
        const bool grow = pixels * sizeof(PostProcessingBuffer) > set.pp.bytes;
        reserve(set.pp, pixels * sizeof(PostProcessingBuffer));
        reserve(set.ids, pixels * sizeof(PrimitiveXYIdBuffer));
        reserve(set.image[0], pixels * SOLR_COLOR_DEPTH);
        if (f == 0) /* (here, not in front of the loop: the order of the device calls is the one it always was) */
        {
            fresh = fresh || grow;
            /* (a buffer set's second RGB image - renderImpl makes it when a read-back still holds the first - grows with
             * the frame too, in use or not: the set may be on that side when the frame is re-shaped) */
            for (Flight &any : g.flight)
                if (any.image[1].ptr)
                    reserve(any.image[1], pixels * SOLR_COLOR_DEPTH);
#ifdef SOLR_TIMING
            if (!g.counters.ptr)
            {
                reserve(g.counters, (16 + 16 * SOLR_TIMING_SLOTS) * sizeof(unsigned long long));
                if (ok())
                    HIPCHECK(hipMemset(g.counters.ptr, 0, g.counters.bytes));
            }
#else
            reserve(g.counters, 16 * sizeof(unsigned long long));
#endif
        }
        if (ok() && (fresh || grow))
        {
            HIPCHECK(hipMemsetAsync(set.pp.ptr, 0, set.pp.bytes, set.stream));
            HIPCHECK(hipMemsetAsync(set.ids.ptr, 0, set.ids.bytes, set.stream));
            HIPCHECK(hipMemsetAsync(set.image[0].ptr, 0, set.image[0].bytes, set.stream));
        }
    }
    g.allocW = g.width;
    g.allocRows = rows;
}

/* the features a frame of the resident scene needs (rt_device.h, enum Feature): decides the kernel instantiation */
int neededFeatures(const SceneInfo &sceneInfo, bool full)
{
    int need = g.facts.sceneFeatures;
    if (!sceneInfo.extendedGeometry)
        /* every primitive is tested as a triangle, GI:743-747 - and textured as one (GI:916-931) */
        need = F_TRI | (g.facts.sceneFeatures & F_TEX);
    if (full)
        need |= F_FULL;
    /* SOLR_HIP_FORCE_FEATURES=mask (experiments, rt_device.h enum Feature): as if the scene had these features too */
    static const int forced = getenv("SOLR_HIP_FORCE_FEATURES") ? atoi(getenv("SOLR_HIP_FORCE_FEATURES")) & F_ALL : 0;
    need |= forced;
    if (sceneInfo.skyboxMaterialId >= 0 && sceneInfo.skyboxMaterialId < (int)g.materials.materialTags.size() &&
        (g.materials.materialTags[sceneInfo.skyboxMaterialId] & PRIM_TEXTURED))
        need |= F_TEX;
    return need;
}

/* The neighbourhood post-processing of a frame - the switch of cudaRender, CRT:1857-1890 - behind the renderer on `stream`,
 * over buffer set `flight`.  (Also what the test-only solr_hip_probe_postprocess runs over a frame buffer of the caller's.) */
void launchPostProcess(const SceneInfo &sceneInfo, const PostProcessingInfo &ppInfo, int flight, hipStream_t stream, int firstRow,
                       int nbRows, unsigned char *bitmap, HaloDebt &debt)
{
    const PixelRecord *const pp = (const PixelRecord *)g.flight[flight].pp.ptr;
    if (ppInfo.type == ppe_ambientOcclusion)
    {
        /* a strip's taps reach into the rows of the ranks above and below: their depths come from the host
         * (solr_hip_set_depth_halo) or, with a communicator, from the neighbours over RCCL, on this stream */
        DepthHalo halo = {nullptr, nullptr, 0, 0};
        if (g.nbRows >= 0 && nbRows > 0)
        {
            const float reach = 16.f * fabsf(ppInfo.param2) * g.randoms.randomsReach / 10.f;
            const int wanted = debt.owed ? debt.wanted : (reach < 4096.f ? (int)reach + 2 : 4096);
            g.haloWanted = wanted;
            if (g.haloSuppliedAbove || g.haloSuppliedBelow)
            {
                halo.above = (const float *)g.haloGivenAbove.ptr;
                halo.below = (const float *)g.haloGivenBelow.ptr;
                halo.nbAbove = g.haloSuppliedAbove;
                halo.nbBelow = g.haloSuppliedBelow;
            }
            else if (debt.owed)
            {
                debt.owed = false;
                exchangeDepthHalo(flight, stream, pp, sceneInfo.size.x, firstRow,
                                  nbRows, sceneInfo.size.y, wanted, &halo);
            }
        }
        if (ok())
            solrpost::ambientOcclusion(stream, sceneInfo, ppInfo, nbRows, pp,
                                       (const float *)g.randoms.values.ptr, g.randoms.values.ptr ? g.randoms.nbRandoms : 0L, bitmap, halo, firstRow,
                                       g.randoms.randomsReach, g.variant != VARIANT_AO_FIXED_STRIDE);
    }
    else if (ppInfo.type == ppe_depthOfField)
        solrpost::depthOfField(stream, sceneInfo, ppInfo, nbRows, pp,
                               (const float *)g.randoms.values.ptr, g.randoms.values.ptr ? g.randoms.nbRandoms : 0L, bitmap);
    else if (ppInfo.type == ppe_radiosity)
        solrpost::radiosity(stream, sceneInfo, ppInfo, nbRows, pp,
                            (const int4 *)g.flight[flight].ids.ptr, (const float *)g.randoms.values.ptr, g.randoms.values.ptr ? g.randoms.nbRandoms : 0L,
                            bitmap);
    else if (ppInfo.type == ppe_filter)
        solrpost::filter(stream, sceneInfo, ppInfo, nbRows, pp, bitmap);
    else
        solrpost::cartoon(stream, sceneInfo, ppInfo, nbRows, pp, bitmap);
    HIPCHECK(hipGetLastError());
}

/* ---- the stages of a frame, in the order renderImpl runs them ------------------------------------------------------ */

/* the arguments checked, the device selected, the frame's buffers sized.  False: nothing to render (the engine's error is
 * set, or this process's strip is empty: more processes than rows to share out) */
static bool frameReady(const SceneInfo &sceneInfo, const vec4i &objects)
{
    if (!ready("cudaRender"))
        return false;
    ARGCHECK(sceneInfo.size.x > 0 && sceneInfo.size.y > 0, "cudaRender: empty image");
    ARGCHECK(objects.x <= g.scene.exact.nb && objects.y <= g.scene.nbPrimitives, "cudaRender: more objects than were uploaded");
    ARGCHECK(objects.w <= g.lights.nbLights, "cudaRender: more lights than were uploaded");
    ARGCHECK(g.materials.table.ptr != nullptr, "cudaRender: no materials uploaded");
    ARGCHECK(sceneInfo.skyboxMaterialId <= NB_MAX_MATERIALS, "cudaRender: skybox material beyond the material table");
    if (!ok())
        return false;
    checkTextureTables();
    if (!ok())
        return false;
    HIPCHECK(hipSetDevice(g.device));
    g.width = sceneInfo.size.x;
    g.height = sceneInfo.size.y;
    g.frameBufferType = (int)sceneInfo.frameBufferType;
    allocateFrame();
    return ok() && stripRows() != 0;
}

/* The buffer set (and stream) of the frame: first-pass frames alternate when two frames may be in flight; a refinement or
 * accumulation pass reads what the previous pass wrote and stays where that is (so does the 3D-vision camera: it reads a
 * depth of the frame before).  And the set's RGB image: an asynchronous read-back (solr_hip_d2h_image_async) may still be
 * reading the image this set rendered last - the frame then goes to the set's other image; only the copy of the frame
 * before last - long done - is waited for.  -1: an allocation failed. */
static int takeFlight(const SceneInfo &sceneInfo, bool counting)
{
    int flight = g.current;
    if (twoFlights() && !counting && sceneInfo.pathTracingIteration == 0 && sceneInfo.cameraType != ctVR)
        flight = (int)(g.frameSerial++ % (unsigned)activeFlights());
    else if (!twoFlights())
        flight = 0;
    g.current = flight;
    Flight &set = g.flight[flight];
    if (!g.boundBitmap && set.copy[set.side] >= 0)
    {
        const int side = set.side ^ 1;
        reserve(set.image[1], set.shown().bytes);
        if (!ok())
            return -1;
        set.side = side;
        if (set.copy[side] >= 0)
        {
            HIPCHECK(hipStreamWaitEvent(set.stream, g.copyLane.imageDone[set.copy[side]], 0));
            set.copy[side] = -1;
        }
    }
    return flight;
}

/* The resident scene as this frame walks it, with the caller's counts of objects.  (The census, the box-debug view, a
 * frame of fewer nodes than were uploaded and the volume camera walk the reference's own list: the volume camera keeps
 * every hit, nearest first, ties in the order it met them.)  False: the engine's error is set. */
static bool frameScene(const SceneInfo &sceneInfo, const vec4i &objects, bool counting, SceneArgs &S)
{
    const bool exactNodes = counting || sceneInfo.renderBoxes != 0 || objects.x != g.scene.exact.nb || g.variant == VARIANT_EXACT_LIST ||
                            sceneInfo.cameraType == ctVolumeRendering;
    S = prepareScene(sceneInfo, exactNodes);
    if (!ok())
        return false;
    if (exactNodes)
        S.nbBoxes = objects.x;
    S.nbPrimitives = objects.y;
    S.nbLamps = objects.z;
    S.nbLights = objects.w;
    return true;
}

/* the box-debug view, the census and the special cameras count every node of the original tree (F_FULL) */
static bool fullFeatures(const SceneInfo &sceneInfo)
{
    return sceneInfo.renderBoxes != 0 || sceneInfo.advancedIllumination == aiBasic || sceneInfo.advancedIllumination == aiFull ||
           sceneInfo.cameraType == ctAntialiazed || sceneInfo.cameraType == ctAnaglyph || sceneInfo.cameraType == ctPanoramic ||
           sceneInfo.cameraType == ctVR || sceneInfo.cameraType == ctVolumeRendering;
}

/* the post-processing reads the pixels around each pixel: a pass of its own behind the renderer (launchPostProcess) */
static bool neighbourhoodPass(const PostProcessingInfo &ppInfo)
{
    return ppInfo.type == ppe_ambientOcclusion || ppInfo.type == ppe_depthOfField || ppInfo.type == ppe_radiosity ||
           ppInfo.type == ppe_filter || ppInfo.type == ppe_cartoon;
}

/* colour-stack slots of a lane: one per bounce the frame may take */
static int bounceSlots(const SceneInfo &sceneInfo)
{
    int maxIt = (sceneInfo.graphicsLevel < glReflectionsAndRefractions)
                    ? 1
                    : sceneInfo.nbRayIterations + sceneInfo.pathTracingIteration;
    maxIt = maxIt > NB_MAX_ITERATIONS ? NB_MAX_ITERATIONS : maxIt;
    return maxIt < 1 ? 1 : maxIt;
}

static size_t ldsBytesFor(int stackSlots)
{
    return ((size_t)stackSlots * 4 + COLD_FIELDS) * WAVE * sizeof(float);
}

static int tileRows(const FrameArgs &F)
{
    return (F.nbRows + TILE_H - 1) / TILE_H;
}

/* The reciprocal of tilesX for the kernel's tile -> (column, row): tile / tilesX = (tile * magic) >> (32 + shift) for every
 * tile below `tiles`.  shift = ceil(log2 tilesX) - 1: the multiplier ceil(2^(32 + shift) / tilesX) has 32 bits and is exact
 * for every index below 2^31; one tile per row (magic 0) needs no division.  False: not exact for every tile. */
static bool tileReciprocal(int tilesX, int tiles, unsigned *magic, int *shift)
{
    int s = 0;
    while ((2 << s) < tilesX)
        ++s;
    const unsigned long long m =
        tilesX == 1 ? 0ull : ((1ull << (32 + s)) + (unsigned long long)tilesX - 1) / (unsigned long long)tilesX;
    bool exact = m <= 0xffffffffull;
    for (int t = 0; t < tiles && exact && m; ++t)
        exact = (int)(((unsigned long long)(unsigned)t * m) >> (32 + s)) == t / tilesX;
    *magic = (unsigned)m;
    *shift = s;
    return exact;
}

/* The frame's arguments as the camera, the strip and the bounce limit decide them (the stages that follow add the rest).
 * The tile reciprocal is verified once per frame geometry and kept in g.  False: there is none (the error is set). */
static bool frameArgs(const SceneInfo &sceneInfo, const PostProcessingInfo &ppInfo, const float origin[3],
                      const float direction[3], const float angles[4], FrameArgs &F)
{
    memset(&F, 0, sizeof(F));
    F.si = sceneInfo;
    F.ppi = ppInfo;
    F.ox = origin[0];
    F.oy = origin[1];
    F.oz = origin[2];
    F.dx = direction[0];
    F.dy = direction[1];
    F.dz = direction[2];
    F.ax = angles[0];
    F.ay = angles[1];
    F.az = angles[2];
    F.aw = angles[3];
    {
        const float ratio = (float)sceneInfo.size.x / (float)sceneInfo.size.y;
        F.stepx = ratio * F.aw / (float)sceneInfo.size.x;
        F.stepy = F.aw / (float)sceneInfo.size.y;
    }
    /* VectorUtils.cuh:108-114 evaluates these per pixel; they are uniform */
    F.trig.cx = cosf(angles[0]);
    F.trig.cy = cosf(angles[1]);
    F.trig.cz = cosf(angles[2]);
    F.trig.sx = sinf(angles[0]);
    F.trig.sy = sinf(angles[1]);
    F.trig.sz = sinf(angles[2]);
    F.firstRow = g.nbRows >= 0 ? g.firstRow : 0;
    F.nbRows = stripRows();
    F.tilesX = (sceneInfo.size.x + TILE_W - 1) / TILE_W;
    const int tiles = F.tilesX * tileRows(F);
    if (g.tileCheckedX != F.tilesX || g.tileCheckedTiles < tiles)
    {
        unsigned magic = 0;
        int shift = 0;
        const bool exact = tileReciprocal(F.tilesX, tiles, &magic, &shift);
        ARGCHECK(exact, "cudaRender: no exact reciprocal for this frame width");
        if (!exact)
            return false; /* (cannot happen below 2^31 tiles; nothing is cached, the next frame checks again) */
        g.tileCheckedX = F.tilesX;
        g.tileCheckedTiles = tiles;
        g.tileCheckedMagic = magic;
        g.tileCheckedShift = shift;
    }
    F.tileMagic = g.tileCheckedMagic;
    F.tileShift = g.tileCheckedShift;
    F.fuseDefault = neighbourhoodPass(ppInfo) ? 0 : 1;
    F.stackSlots = bounceSlots(sceneInfo);
    if (sceneInfo.cameraType == ctVolumeRendering)
        F.stackSlots = 11; /* the ten layers of launchVolumeRendering and the element behind them */
    return true;
}

/* ctVR: the focus pixel of k_3DVisionRenderer (CRT:973, integer expression as written there) as the frame before left it; a
 * strip that does not hold it reads 0 */
static void readFocusDepth(FrameArgs &F, int flight, hipStream_t stream)
{
    const long focusIndex = (long)(F.si.size.x / 2 * F.si.size.y / 2);
    const long focusRow = focusIndex / F.si.size.x - F.firstRow;
    if (focusRow >= 0 && focusRow < F.nbRows && g.flight[flight].pp.ptr)
    {
        const PostProcessingBuffer *at =
            (const PostProcessingBuffer *)g.flight[flight].pp.ptr + focusRow * F.si.size.x + focusIndex % F.si.size.x;
        HIPCHECK(hipMemcpyAsync(&F.focusDepth, &at->colorInfo.w, sizeof(float), hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
    }
}

/* diagnostics (solr_hip_enable_tile_clocks): {start, end} of every tile of the frame.  False: the allocation failed */
static bool armTileClocks(FrameArgs &F, unsigned tiles)
{
    reserve(g.tileClock, (size_t)tiles * 2 * sizeof(unsigned long long));
    if (!ok())
        return false;
    F.tileClock = (unsigned long long *)g.tileClock.ptr;
    g.nbTilesTimed = (int)tiles;
    return true;
}

/* ImageStreaming (renderer.h): the bands, in tiles, this frame's image would leave in; bands = 0: it is not streamed.  Asked
 * for (solr_hip_stream_next_image), and a frame whose image the kernel itself writes, whole, on one device, one frame at a
 * time.  (Is there an instantiation that counts tiles for the kernel this scene takes?  Asked of the frame before: the
 * launch order, made further up than the choice of the kernel, has to know.)  The request is used up; *withIds: it was
 * for the primitive ids too. */
static BandCuts decideStreamCuts(const FrameArgs &F, bool counting, bool *withIds)
{
    g.streaming.valid = false;
    BandCuts cuts = {};
    int rows[SOLR_STREAM_BANDS_MAX + 1];
    if (g.streaming.next && !counting && !g.recording.recordNext && F.fuseDefault && F.si.frameBufferType != ftBGR && !twoFlights() &&
        g.nbRows < 0 && gDevices == 1 && !g.boundBitmap && !gImageRing.sharedRing && g.lastMask >= 0 &&
        solrrows::renderer(0, g.lastMask | F_STREAM, false) != nullptr &&
        imageStreamingCuts(tileRows(F), rows, &cuts.bands, g.streaming.next == 2))
    {
        for (int b = 0; b <= cuts.bands; ++b)
            cuts.firstTile[b] = rows[b] * F.tilesX;
        /* the heaviest eighth of the tiles first, wherever they lie (k_orderTiles; with none first the molecule's frame is
         * 0.412 ms against 0.385, with half of them 0.42 and the Cornell box's 0.54: profiles/r6/stream_frame.txt) */
        cuts.heavyShare = 8;
    }
    *withIds = g.streaming.next == 2;
    g.streaming.next = 0;
    return cuts;
}

/* The cost-ordered launch (g.sched, engine.h TileSchedule): the frame records what its tiles cost, and takes the launch
 * order made from the costs of the frames before it.  Statistics (and, in cost order, a fresh order) every
 * SORT_PERIOD-th frame, and at once when the decision has just changed; in between the last order is reused.
 * *streamCandidate: a frame whose longest tile would be rendered by four quadrant waves is not streamed.  False: an
 * allocation failed. */
static bool scheduleTiles(FrameArgs &F, unsigned tiles, int flight, hipStream_t stream, const BandCuts &streamCuts,
                          bool *streamCandidate)
{
    TileSchedule &s = g.sched;
    const long key[6] = {(long)tiles, F.tilesX, F.firstRow, F.nbRows, F.si.size.x, F.si.size.y};
    if (!s.hostStats)
    {
        HIPCHECK(hipHostMalloc((void **)&s.hostStats, 8 * sizeof(unsigned), hipHostMallocMapped));
        if (ok())
        {
            memset(s.hostStats, 0, 8 * sizeof(unsigned));
            HIPCHECK(hipHostGetDevicePointer((void **)&s.hostStatsDev, s.hostStats, 0));
        }
    }
    if (memcmp(key, s.key, sizeof(key)) != 0 || !s.cost.ptr)
    {
        memcpy(s.key, key, sizeof(key));
        s.reset();
        /* none of them is read before a sort has written it; a fresh allocation still gets a defined
         * content (a buffer that is kept may be in use by a frame in flight and is left alone) */
        for (DeviceBuffer *b : {&s.cost, &s.costSnapshot, &s.order[0], &s.order[1]})
        {
            const void *before = b->ptr;
            reserve(*b, ((size_t)tiles + (SPLIT_PARTS - 1) * SPLIT_TILES_MAX) * sizeof(unsigned));
            if (ok() && b->ptr != before)
                HIPCHECK(hipMemset(b->ptr, 0, b->bytes));
        }
        s.orderBuffer = 0;
        for (bool &w : s.orderWait)
            w = false;
    }
    if (!ok())
        return false;
    /* decision of the automatic mode from the newest frame the host can see (no synchronisation:
     * the figures are one or two frames old, which is as good for a scheduling hint) */
    if (s.frames > 0 && s.hostStats[4] != 0 && s.hostStats[3] == tiles)
    {
        const unsigned long long sum = (unsigned long long)s.hostStats[1] | ((unsigned long long)s.hostStats[2] << 32);
        const unsigned long long mx = s.hostStats[0];
        if (mx * tiles > 2ull * sum)
            s.reorder = true;
        else if (2ull * mx * tiles < 3ull * sum)
            s.reorder = false;
        /* a frame whose longest tile would be rendered by four quadrant waves (k_orderTiles' criterion, for one frame
         * in flight) keeps the order that puts those first: it is not streamed */
        const float mean = (float)sum / (float)tiles;
        const float critical = fmaxf(2.f * mean, (float)sum / 5120.f);
        if (s.reorder && (unsigned)(critical * (64.f / ((float)mx + 1.f))) < 63u)
            *streamCandidate = false;
    }
    F.tileCost = (unsigned *)s.cost.ptr;
    const bool ordered = s.frames > 0 && (s.mode == 2 || s.reorder);
    /* a streamed frame takes its tiles band after band (k_orderTiles), any other by cost alone: the order is re-made
     * at once when the frame at hand is of the other kind */
    const BandCuts cuts = *streamCandidate ? streamCuts : BandCuts();
    if (ordered && s.orderValid && memcmp(&s.orderCuts, &cuts, sizeof(cuts)) != 0)
        s.orderValid = false;
    const bool refresh = s.frames > 0 && (s.frames % SORT_PERIOD == 1 || (ordered && !s.orderValid));
    const bool sort = ordered && refresh;
    if (!ordered)
        s.orderValid = false;
    if (refresh)
    {
        /* a new order goes to the buffer no frame in flight is reading; the other stream waits for
         * the sort before its next frame picks that buffer up */
        const int target = sort ? (s.orderBuffer ^ 1) : s.orderBuffer;
        solrpost::orderTiles(stream, (const unsigned *)s.cost.ptr, (unsigned *)s.costSnapshot.ptr, (unsigned *)s.order[target].ptr,
                             (int)tiles, (volatile unsigned *)s.hostStatsDev, sort ? activeFlights() : 0, cuts);
        HIPCHECK(hipGetLastError());
        if (sort)
        {
            s.orderValid = true;
            s.orderCuts = cuts;
            s.orderBuffer = target;
            if (twoFlights())
            {
                if (!s.orderEvent)
                    HIPCHECK(hipEventCreateWithFlags(&s.orderEvent, hipEventDisableTiming));
                if (ok())
                    HIPCHECK(hipEventRecord(s.orderEvent, stream));
                for (int f = 0; f < MAX_FLIGHTS; ++f)
                    s.orderWait[f] = (f != flight);
            }
        }
    }
    if (s.orderWait[flight] && s.orderEvent)
    {
        HIPCHECK(hipStreamWaitEvent(stream, s.orderEvent, 0));
        s.orderWait[flight] = false;
    }
    if (ordered && s.orderValid)
        F.tileOrder = (const unsigned *)s.order[s.orderBuffer].ptr;
    s.frames++;
    return true;
}

void TileSchedule::release()
{
    for (DeviceBuffer *b : {&cost, &costSnapshot, &order[0], &order[1]})
        solreng::release(*b);
    if (orderEvent)
        (void)hipEventDestroy(orderEvent);
    if (hostStats)
        (void)hipHostFree(hostStats);
    const int keep = mode;
    *this = TileSchedule();
    mode = keep;
}

/* every g.timing-th frame's kernel between two events (solr_hip_enable_timing, collectEvents); {null, null}: not this one */
static std::pair<hipEvent_t, hipEvent_t> startKernelTimer(bool counting, hipStream_t stream)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (g.timing > 0 && !counting && (g.timer.timingTick++ % (unsigned)g.timing) == 0)
    {
        HIPCHECK(hipEventCreate(&e0));
        HIPCHECK(hipEventCreate(&e1));
        HIPCHECK(hipEventRecord(e0, stream));
    }
    return std::make_pair(e0, e1);
}

/* the kernel a frame takes: the function; the row of solrrows::ROWS and the features of its instantiation (-1: the census
 * or the all-features kernel); the colour-stack slots of the frame kept in HBM (F_STACK) */
struct KernelChoice
{
    RendererFn fn;
    int row, mask, deepSlots;
};
static KernelChoice chooseKernel(const SceneInfo &sceneInfo, bool full, bool deepList, bool counting)
{
    const bool volumeCamera = sceneInfo.cameraType == ctVolumeRendering;
    if (counting)
        return {solrrows::renderer(1, F_ALL, volumeCamera), -1, -1, 0};
    KernelChoice k = {solrrows::renderer(0, F_ALL | F_DEEP, volumeCamera), -1, -1, 0};
    if (volumeCamera || g.variant == VARIANT_ALL_FEATURES)
        return k;
    /* smallest instantiation that covers the scene (rt_device.h, enum Feature) */
    const int need = neededFeatures(sceneInfo, full);
    for (int row = 0; row < solrrows::NB_ROWS; ++row)
        if ((need & ~solrrows::ROWS[row].features) == 0)
        {
            k.row = row;
            k.mask = solrrows::rowMask(row, deepList);
            k.fn = solrrows::renderer(0, k.mask, false);
            /* more bounces than colour-stack slots fit the LDS of 16 waves per CU: the lean rows have an
             * instantiation that keeps the deeper slots in HBM (rt_device.h ColorStack, F_STACK) */
            const int slots = bounceSlots(sceneInfo);
            if (slots > SOLR_LDS_STACK_SLOTS && !g.recording.recordNext && g.variant != VARIANT_STACK_IN_LDS)
                if (RendererFn spilling = solrrows::renderer(0, k.mask | F_STACK, false))
                {
                    k.fn = spilling;
                    k.deepSlots = slots - SOLR_LDS_STACK_SLOTS;
                }
            break;
        }
    return k;
}

/* This frame leaves a record of its walks (rt_device.h recordWalk; solr_hip_walk_bound): the same kernel with COUNT == 2,
 * launched exactly as it would have been - grid, order, LDS - with the record buffer in place of the counters.  Only the
 * lean rows of the table have such an instantiation.  Null: none, or an allocation failed (the error is set). */
static RendererFn recordingKernel(const KernelChoice &k, const SceneArgs &S, unsigned grid, size_t ldsBytes, hipStream_t stream)
{
    g.recording.recordNext = false;
    ARGCHECK(k.row >= 0 && k.row < solrrows::LEAN_ROWS,
             "solr_hip_walk_bound: the kernel this scene needs has no recording instantiation (untextured spheres, "
             "planes, triangles, cylinders only)");
    if (!ok())
        return nullptr;
    reserve(g.recording.walkRecords, (size_t)grid * SOLR_WALK_SLOT_BYTES);
    reserve(g.recording.walkVisits, (size_t)grid * WAVE * sizeof(unsigned) + 64);
    if (!ok())
        return nullptr;
    HIPCHECK(hipMemsetAsync(g.recording.walkRecords.ptr, 0, (size_t)grid * SOLR_WALK_SLOT_BYTES, stream));
    const RendererFn fn = solrrows::renderer(2, k.mask, false);
    ARGCHECK(fn != nullptr, "solr_hip_walk_bound: no recording instantiation");
    if (!ok())
        return nullptr;
    g.recording.recordGrid = grid;
    g.recording.recordLds = ldsBytes;
    g.recording.recordDeep = (k.mask & F_DEEP) != 0;
    g.recording.recordScene = S;
    g.recording.recorded = true;
    return fn;
}

/* An F_STACK instantiation: SOLR_LDS_STACK_SLOTS slots in LDS - 16 waves per CU whatever the bounce limit - and the rest of
 * this buffer set's frame in HBM, a plane of the strip per slot (3840 x 2160 x 7 slots: 0.9 GB of the 288; touched only by
 * the rays that go that deep).  False: the allocation failed. */
static bool armDeepStack(FrameArgs &F, int deepSlots, int flight, hipStream_t stream)
{
    F.stackSlots = SOLR_LDS_STACK_SLOTS;
    F.deepStride = (long)F.si.size.x * F.nbRows;
    reserve(g.flight[flight].deepStack, (size_t)deepSlots * (size_t)F.deepStride * sizeof(float4));
    if (!ok())
        return false;
    F.deepStack = (float4 *)g.flight[flight].deepStack.ptr;
    /* the deep slots are never zeroed: every slot a lane reads was written by the trip that made it (rt_device.h
     * launchRayTracing).  VARIANT_NAN_DEEP_STACK proves it: NaNs in every slot before the launch, the same frame after */
    if (g.variant == VARIANT_NAN_DEEP_STACK)
        HIPCHECK(hipMemsetAsync(F.deepStack, 0xff, (size_t)deepSlots * (size_t)F.deepStride * sizeof(float4), stream));
    return true;
}

/* ImageStreaming: the instantiation of the frame's row that counts its tiles, when there is one and the counters are armed
 * (tiles in launch order, or band after band: an order by cost alone completes every band at the end; the epilogue that
 * counts tiles is in instantiations of its own - the lean rows have them, rt_device.h F_STREAM).  False: the frame is not
 * streamed. */
static bool armStreamedFrame(FrameArgs &F, const KernelChoice &k, const BandCuts &cuts, hipStream_t stream, bool withIds,
                             RendererFn *fn)
{
    if (k.mask < 0 || (F.tileOrder && memcmp(&g.sched.orderCuts, &cuts, sizeof(cuts)) != 0))
        return false;
    const RendererFn streaming = solrrows::renderer(0, k.mask | (k.deepSlots > 0 ? F_STACK : 0) | F_STREAM, false);
    if (!streaming || !armImageStreaming(F, tileRows(F), stream, withIds))
        return false;
    *fn = streaming;
    F.fuseDefault |= withIds ? 6 : 2;
    if (g.variant == VARIANT_NO_BAND_WORDS) /* (tests: the waves write no band's word - the host goes by the end of the kernel) */
        F.streamSerial = 0x7fffff00u;
    return true;
}

void renderImpl(const SceneInfo &sceneInfo, const vec4i &objects, const PostProcessingInfo &ppInfo,
                const float origin[3], const float direction[3], const float angles[4], bool counting,
                unsigned long long counts[8])
{
    HostSpan whole("cudaRender (whole)");
    HaloDebt debt;
    if (ppInfo.type == ppe_ambientOcclusion && haveCommunicator())
    {
        /* (every rank, before anything rank-local can end the call: an all-reduce when the figure is stale) */
        debt.wanted = agreedHaloRows(ppInfo);
        debt.width = sceneInfo.size.x;
        debt.frameRows = sceneInfo.size.y;
        debt.owed = !(g.haloSuppliedAbove || g.haloSuppliedBelow);
    }
    if (!frameReady(sceneInfo, objects))
        return;
    const int flight = takeFlight(sceneInfo, counting);
    if (flight < 0)
        return;
    const hipStream_t stream = g.flight[flight].stream;
    SceneArgs S;
    if (!frameScene(sceneInfo, objects, counting, S))
        return;
    FrameArgs F;
    if (!frameArgs(sceneInfo, ppInfo, origin, direction, angles, F))
        return;
    const unsigned tiles = (unsigned)(F.tilesX * tileRows(F));
    if (sceneInfo.cameraType == ctVR)
        readFocusDepth(F, flight, stream);
    if (g.tileClocks && !armTileClocks(F, tiles))
        return;
    bool streamIds = false;
    const BandCuts streamCuts = decideStreamCuts(F, counting, &streamIds);
    bool streamCandidate = streamCuts.bands > 0;
    if (g.sched.mode > 0 && !counting && !scheduleTiles(F, tiles, flight, stream, streamCuts, &streamCandidate))
        return;
    const std::pair<hipEvent_t, hipEvent_t> timer = startKernelTimer(counting, stream);

    const KernelChoice k = chooseKernel(sceneInfo, fullFeatures(sceneInfo), deepNodeList(S), counting);
    if (!counting)
        g.recording.recordVariant = k.row;
    ARGCHECK(k.fn != nullptr, "cudaRender: no instantiation of the renderer for this scene (csrc/rows)");
    if (!ok())
        return;
    /* (the census kernel adds into them; a frame's own kernel does not touch them: zeroing them on the stream of EVERY frame
     * was a fill kernel of 3.6 us - and a launch - in front of every renderer, 1.4 % of the GPU's time in the profile) */
    if (counting)
        HIPCHECK(hipMemsetAsync(g.counters.ptr, 0, 8 * sizeof(unsigned long long), stream));
    /* the ordered launch has a fixed number of extra workgroups for the quadrant waves of split tiles
     * (k_orderTiles); the ones the order does not use return at once */
    F.nbTiles = (int)tiles;
    const dim3 grid(F.tileOrder ? tiles + (unsigned)(SPLIT_PARTS - 1) * SPLIT_TILES_MAX : tiles);
    RendererFn fn = k.fn;
    const bool recording = g.recording.recordNext && !counting;
    if (recording && !(fn = recordingKernel(k, S, grid.x, ldsBytesFor(F.stackSlots), stream)))
        return;
    unsigned long long *cntPtr = (unsigned long long *)(recording ? g.recording.walkRecords.ptr : g.counters.ptr);
    if (k.deepSlots > 0 && !armDeepStack(F, k.deepSlots, flight, stream))
        return;
    unsigned char *bitmap = (unsigned char *)(g.boundBitmap ? g.boundBitmap : g.flight[flight].shown().ptr);
    const bool streamed = streamCandidate && !recording && armStreamedFrame(F, k, streamCuts, stream, streamIds, &fn);
    g.lastMask = k.mask;
    g.streaming.ids = streamed && streamIds;
    if (!counting)
    {
        const int features = k.mask < 0 ? -1 : k.mask | (k.deepSlots > 0 ? F_STACK : 0) | (streamed ? F_STREAM : 0);
        const int last[6] = {k.row, features, streamed ? 1 : 0, streamed ? streamCuts.bands : 0, F.tileOrder ? 1 : 0,
                             F.tileOrder ? g.sched.orderCuts.bands : 0};
        memcpy(g.lastFrame, last, sizeof(last));
    }
    {
        HostSpan launch("  of which the kernel launch");
        hipLaunchKernelGGL(fn, grid, dim3(WAVE), ldsBytesFor(F.stackSlots), stream, S, F, (PixelRecord *)g.flight[flight].pp.ptr,
                           (int4 *)g.flight[flight].ids.ptr, bitmap, cntPtr);
    }
    HIPCHECK(hipGetLastError());
    if (timer.first)
    {
        HIPCHECK(hipEventRecord(timer.second, stream));
        g.timer.events.push_back(timer);
    }
    if (streamed)
    {
        markStreamedFrame(stream);
        g.streaming.valid = ok();
        g.streaming.bitmap = bitmap;
    }

    g.haloWanted = 0;
    if (neighbourhoodPass(ppInfo))
        launchPostProcess(sceneInfo, ppInfo, flight, stream, F.firstRow, F.nbRows, bitmap, debt);
    if (counting && counts)
    {
        HIPCHECK(hipMemcpyAsync(counts, g.counters.ptr, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                stream));
        HIPCHECK(hipStreamSynchronize(stream));
    }
}

void collectEvents()
{
    hipEvent_t before = nullptr;
    for (auto &ev : g.timer.events)
    {
        float ms = 0.f, gap = 0.f;
        if (hipEventSynchronize(ev.second) == hipSuccess && hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess)
        {
            g.timer.timedMs += ms;
            g.timer.timedLaunches++;
            if (g.timer.kernelSamples.size() < 65536)
            {
                g.timer.kernelSamples.push_back(ms);
                /* end of the launch before to the end of this one: what a step of a pipelined loop takes */
                g.timer.intervalSamples.push_back((before && hipEventElapsedTime(&gap, before, ev.second) == hipSuccess) ? gap : -1.f);
            }
        }
        if (before)
            (void)hipEventDestroy(before);
        (void)hipEventDestroy(ev.first);
        before = ev.second;
    }
    if (before)
        (void)hipEventDestroy(before);
    g.timer.events.clear();
}
/* wait == false: the copies are enqueued and d2hBitmapWait() is owed (several devices copy side by side) */
void d2hBitmapOne(const SceneInfo &sceneInfo, BitmapBuffer *bitmap, PrimitiveXYIdBuffer *primitivesXYIds, bool wait)
{
    if (!ready("d2h_bitmap"))
        return;
    HIPCHECK(hipSetDevice(g.device));
    const int rows = stripRows();
    const int first = g.nbRows >= 0 ? g.firstRow : 0;
    const size_t pixels = (size_t)sceneInfo.size.x * rows;
    const size_t offset = (size_t)sceneInfo.size.x * first;
    /* the frame rendered last: its buffer set, on its stream */
    const hipStream_t stream = g.flight[g.current].stream;
    const void *src = g.boundBitmap ? g.boundBitmap : g.flight[g.current].shown().ptr;
    if (bitmap && src)
        HIPCHECK(hipMemcpyAsync(bitmap + offset * SOLR_COLOR_DEPTH, src, pixels * SOLR_COLOR_DEPTH,
                                hipMemcpyDeviceToHost, stream));
    if (primitivesXYIds && g.flight[g.current].ids.ptr)
        HIPCHECK(hipMemcpyAsync(primitivesXYIds + offset, g.flight[g.current].ids.ptr,
                                pixels * sizeof(PrimitiveXYIdBuffer), hipMemcpyDeviceToHost, stream));
    if (wait)
        HIPCHECK(hipStreamSynchronize(stream));
}
void d2hBitmapWait()
{
    if (g.initialized && ok())
        HIPCHECK(hipStreamSynchronize(g.flight[g.current].stream));
}

} // namespace solreng

extern "C" {
/* the float frame buffer of the strip rendered last (strip-sized host buffer; with several in-process devices the
 * whole frame: every device's rows at their place) */
void solr_hip_d2h_postprocessing(PostProcessingBuffer *hostBuffer)
{
    onEveryDevice([&](int) {
        if (!ready("solr_hip_d2h_postprocessing"))
            return;
        ARGCHECK(hostBuffer != nullptr && g.flight[g.current].pp.ptr != nullptr, "solr_hip_d2h_postprocessing: no buffer");
        if (!ok())
            return;
        const size_t pixels = (size_t)g.width * stripRows();
        const size_t offset = gDevices > 1 ? (size_t)g.width * (g.nbRows >= 0 ? g.firstRow : 0) : 0;
        HIPCHECK(hipMemcpyAsync(hostBuffer + offset, g.flight[g.current].pp.ptr, pixels * sizeof(PostProcessingBuffer),
                                hipMemcpyDeviceToHost, g.flight[g.current].stream));
        HIPCHECK(hipStreamSynchronize(g.flight[g.current].stream));
    });
}

void solr_hip_h2d_postprocessing(const PostProcessingBuffer *hostBuffer, const PrimitiveXYIdBuffer *ids)
{
    if (!ready("solr_hip_h2d_postprocessing"))
        return;
    quiesce();
    allocateFrame();
    if (!ok())
        return;
    /* into the set the next refinement / accumulation pass will read: the current one */
    const size_t pixels = (size_t)g.width * stripRows();
    const hipStream_t stream = g.flight[g.current].stream;
    if (hostBuffer)
        HIPCHECK(hipMemcpyAsync(g.flight[g.current].pp.ptr, hostBuffer, pixels * sizeof(PostProcessingBuffer),
                                hipMemcpyHostToDevice, stream));
    if (ids)
        HIPCHECK(hipMemcpyAsync(g.flight[g.current].ids.ptr, ids, pixels * sizeof(PrimitiveXYIdBuffer),
                                hipMemcpyHostToDevice, stream));
    HIPCHECK(hipStreamSynchronize(stream));
}


void solr_hip_render_counting(const SceneInfo *sceneInfo, const vec4i *objects,
                              const PostProcessingInfo *postProcessingInfo, const float origin[3],
                              const float direction[3], const float angles[4], unsigned long long counts[8])
{
    if (gDevices < 2)
    {
        renderImpl(*sceneInfo, *objects, *postProcessingInfo, origin, direction, angles, true, counts);
        return;
    }
    /* several in-process devices: the census of the frame is the sum over their strips */
    unsigned long long sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    onEveryDevice([&](int) {
        unsigned long long mine[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        renderImpl(*sceneInfo, *objects, *postProcessingInfo, origin, direction, angles, true, mine);
        for (int i = 0; i < 8; ++i)
            sum[i] += mine[i];
    });
    if (counts)
        memcpy(counts, sum, sizeof(sum));
}

} // extern "C"
