/*
 * engine.h - the state of the MI355X rendering engine and the helpers every part of its host side uses: what
 * solr_hip.hip (the boundary), solr_uploads.hip (the h2d_* uploads), solr_arena.hip (the arena and the node lists; their
 * host builders: list_builders.h), solr_rotation.hip (rotation and refit on the device), solr_morph.hip (key-frame
 * morphing on the device), solr_moves.hip (translation and lamp moves on the device), solr_edits.hip (primitives set anew on
 * the device), solr_materials.hip (primitives' materials set on the device), solr_bank.hip (resident scenes set aside
 * and put back), solr_launch.hip (the renderer's
 * launch), solr_diag.hip (knobs and diagnostics), solr_image_ring.hip (the pipelined read-back), solr_rccl.hip (strips,
 * communicator, gather, halo) and solr_post.hip (the post-processing kernels) share.
 * One Engine per device this process renders on; `g` is the engine a function works on.  The records an Engine is made of:
 * NodeList (a node list of the resident scene), Scene with Arena, OrderFreeState, Refit and Morph, Lights, Materials, Textures,
 * Randoms and SceneFacts (the resident scene, cut by who writes them; what a request on it changes: RequestKind and
 * Scene::requestServed, how many an engine has served: Engine::served), KernelTimer, WalkRecording, TileSchedule (the
 * cost-ordered launch), Flight (a frame in flight: its stream and per-pixel buffers; Engine::flight[0] is the one of a
 * process that renders one frame at a time), CopyLane (the device's part of the pipelined read-back), ImageStreaming (a
 * frame read back in bands) and JpegStream with JpegSlot (JPEG frames in flight: resident buffers and tickets); ImageRing - the page-locked host images of the pipelined read-back and their tickets - exists
 * once per process (gImageRing), whatever the number of
 * engines.  gfx950 only.
 */
#ifndef SOLR_ENGINE_H
#define SOLR_ENGINE_H

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/solr_hip.h"
#include "renderer.h"
#include "lists_device.h"
#include "list_builders.h"

namespace solreng
{
/* SOLR_HIP_DEBUG_TIMING=1: where the host side of an upload spends its time (stderr) */
/* SOLR_HIP_HOST_PROFILE=1 (diagnostics): what the HOST spends per call inside the entry points of a frame - at eight
 * GPUs a strip takes 0.04 ms and the host's own 0.04-0.05 ms per step is what bounds the frame rate.  Totals go to stderr
 * at finalize_scene. */
struct HostProfile
{
    const bool on = getenv("SOLR_HIP_HOST_PROFILE") != nullptr;
    struct Entry
    {
        const char *name;
        double seconds;
        long calls;
    } entries[16] = {};
    int used = 0;
    Entry *find(const char *name)
    {
        for (int i = 0; i < used; ++i)
            if (entries[i].name == name)
                return &entries[i];
        if (used < 16)
        {
            entries[used].name = name;
            return &entries[used++];
        }
        return nullptr;
    }
    void report()
    {
        if (!on)
            return;
        for (int i = 0; i < used; ++i)
            fprintf(stderr, "solr_hip host: %-34s %9.3f us per call over %ld calls\n", entries[i].name,
                    1e6 * entries[i].seconds / (entries[i].calls ? entries[i].calls : 1), entries[i].calls);
        used = 0;
    }
    ~HostProfile() { report(); } /* (a host that never finalizes: at exit) */
};
extern HostProfile gHostProfile; /* (solr_hip.hip) */
struct HostSpan
{
    const char *name;
    std::chrono::steady_clock::time_point t0;
    explicit HostSpan(const char *n) : name(n)
    {
        if (gHostProfile.on)
            t0 = std::chrono::steady_clock::now();
    }
    ~HostSpan()
    {
        if (!gHostProfile.on)
            return;
        if (HostProfile::Entry *e = gHostProfile.find(name))
        {
            e->seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            e->calls++;
        }
    }
};

struct PhaseTimer
{
    const bool on = getenv("SOLR_HIP_DEBUG_TIMING") != nullptr;
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    void mark(const char *what)
    {
        if (!on)
            return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "solr_hip: %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - last).count());
        last = now;
    }
};

struct DeviceBuffer
{
    void *ptr = nullptr;
    size_t bytes = 0;
};
inline void release(DeviceBuffer &b)
{
    if (b.ptr)
        (void)hipFree(b.ptr);
    b.ptr = nullptr;
    b.bytes = 0;
}

/* frames in flight at most (per-pixel buffer sets and streams).  Whole 1080p frames gain nothing beyond three, a
 * 1/8 strip - one round of waves, as slow as its longest - up to four; six and eight were tried (the mesh's
 * slowest strip: 0.114 ms with three, 0.089 with four, 0.12 and 0.11 with six and eight). */
const int MAX_FLIGHTS = 4;
/* A frame in flight (solr_hip_set_frames_in_flight): with n > 1, consecutive first-pass frames rotate over n streams and
 * n sets of per-pixel buffers, so that the tail of one frame - a few long waves on an otherwise idle chip - overlaps the
 * start of the next.  Engine::flight[0] is the set of a process that renders one frame at a time. */
struct Flight
{
    hipStream_t stream = nullptr; /* the engine's own or the caller's (Engine::ownStream, callerStreams) */
    DeviceBuffer pp, ids;         /* per-pixel buffers of the strip */
    /* two RGB images, the second ("side" 1) for the time a copy still reads the first: a refinement or accumulation pass
     * stays on the set of the pass before it, and would otherwise wait for that pass's copy (made when first needed) */
    DeviceBuffer image[2];
    int side = 0;           /* the image the set's frames go to */
    int copy[2] = {-1, -1}; /* slot of the image ring whose copy reads that image, or -1 */
    DeviceBuffer deepStack; /* F_STACK frames: the colour-stack slots beyond the LDS ones */
    /* ambient occlusion across strips: the depths of the neighbours' rows next to this rank's strip */
    DeviceBuffer haloAbove, haloBelow, haloSendTop, haloSendBottom;

    DeviceBuffer &shown() { return image[side]; }
    /* no copy reads an image any more (the image ring is gone): back to the first image, the second given back */
    void forgetCopies()
    {
        copy[0] = copy[1] = -1;
        side = 0;
        solreng::release(image[1]);
    }
    /* every buffer given back; the stream stays */
    void release()
    {
        for (DeviceBuffer *b : {&pp, &ids, &image[0], &deepStack, &haloAbove, &haloBelow, &haloSendTop, &haloSendBottom})
            solreng::release(*b);
        forgetCopies();
    }
};
/* head of the shared segment of solr_hip_image_share; the images follow, page-aligned.  done[r][slot]: the serial of
 * the last copy of rank r into that slot that has landed; consumed: the last serial the root has handed to its host. */
struct SharedRing
{
    std::atomic<long> done[64][MAX_FLIGHTS + 2];
    std::atomic<long> consumed;
    long frameBytes, imageStride;
};
/* The pipelined read-back (solr_hip_d2h_image_async), the process's part: a ring of page-locked host images - every
 * in-process device copies its strip into the same image - and the tickets handed out for them.  One per process
 * (gImageRing); what an engine adds is its CopyLane. */
struct ImageRing
{
    static const int IMAGE_RING = MAX_FLIGHTS + 2; /* MAX_FLIGHTS tickets outstanding, the image on show, one spare */
    BitmapBuffer *pinnedImage[IMAGE_RING] = {};
    size_t pinnedBytes = 0;
    /* a ticket is (serial mod TICKET_PERIOD) * IMAGE_RING + slot - a positive int whatever the age of the process (the
     * serial itself is 64 bits, counts every ticket this process ever handed out and is never reset or reduced: 0.04 ms
     * per frame of an eight-rank job is 2^31 / 6 tickets in four hours) - and the serial tells a ticket whose slot has
     * been handed out again (or whose ring was re-allocated for a larger frame, or shared / unshared since) from a live
     * one: two tickets of one process are alike only 357 million tickets apart */
    static const long TICKET_PERIOD = ((long)0x7fffffff / IMAGE_RING / IMAGE_RING - 1) * IMAGE_RING;
    static int ticketOf(long serial, int slot) { return (int)((serial % TICKET_PERIOD) * IMAGE_RING + slot); }
    long imageSerial = 0;
    long slotSerial[IMAGE_RING] = {};
    /* A ring the ranks of a job share (solr_hip_image_share) is addressed by a sequence number of its own, counted
     * from the share on every rank alike (the ranks run the same program): it picks the slot and is what `done` /
     * `consumed` of the segment's head hold; the ticket's generation stays this process's own serial */
    long shareSeq = 0;
    long slotShareSeq[IMAGE_RING] = {};
    long lastWaitedSeq = 0;               /* sequence number of the newest ticket solr_hip_image_wait was asked for */
    long sharePublished[IMAGE_RING] = {}; /* the sequence number this rank has reported as landed, per slot */
    /* the ring in memory that several processes share (solr_hip_image_share): every rank's strip lands, over that
     * rank's own PCIe link, at its rows of ONE host image */
    struct SharedRing *sharedRing = nullptr;
    size_t sharedBytes = 0;
    std::string sharedName;
    int shareRank = 0, shareWorld = 0;
    bool slotOfStrips[IMAGE_RING] = {}; /* that slot's ticket was for every rank's strip (not the root's gathered frame) */
    long lastHandedOut = 0;             /* root: the serial of the image its last solr_hip_image_wait returned */
    bool copyOnRenderStream = false;    /* solr_hip_set_copy_route */
    /* the images given back, the shared segment left: outstanding tickets are void (their serial no longer matches).
     * Nothing to do, and harmless, when there is no ring (solr_image_ring.hip) */
    void release();
};
extern ImageRing gImageRing; /* (solr_image_ring.hip) */
/* ... and an engine's part: a copy stream, and per slot of the ring the event that says this device's copy has landed */
struct CopyLane
{
    hipStream_t stream = nullptr;
    hipEvent_t frameRendered = nullptr;
    hipEvent_t imageDone[ImageRing::IMAGE_RING] = {};
    void release(); /* waits for the stream first (solr_image_ring.hip) */
};
/* ImageStreaming (renderer.h): the next frame counts its tiles if it can (solr_hip_stream_next_image), and
 * solr_hip_d2h_streamed_image then sends its image off band by band as the bands' words come */
struct ImageStreaming
{
    int next = 0;                  /* 0 no, 1 the image, 2 the image and the primitive ids */
    bool ids = false;              /* the frame rendered last stored its ids for the bands too */
    bool valid = false;            /* the frame rendered last counted its tiles: serial, image and bands below */
    const void *bitmap = nullptr;
    unsigned serial = 0;           /* streamed frames since the counters were zeroed */
    long key[3] = {0, 0, 0};       /* tilesX, tile rows (+ 100000 x the number of bands), image width the counters belong to */
    DeviceBuffer counters;         /* rowDone | bandDone | the StreamPlan */
    StreamPlan plan = {};          /* host image of the plan */
    int bands = 0;
    unsigned *hostWords = nullptr; /* StreamPlan::hostWord, the host's address */
    hipEvent_t rendered = nullptr; /* behind the kernel of the streamed frame rendered last */
    long delivered = 0;            /* images that left in bands */
    int support = -1;              /* 1 / 0; -1: not asked yet (SOLR_HIP_NO_IMAGE_STREAMING) */
    /* at finalize only: a ring that is re-made for a larger frame must leave the counters alone - the frame that is being
     * read back may still be counting into them (solr_image_ring.hip) */
    void release();
};
/* Frames between two sorts of the tiles by cost (k_orderTiles: one workgroup, 46 us for the 32 400 tiles of a 1080p frame, on the
 * frame's own stream: 2.9 us of every Cornell frame at sixteen, which it was until round 6; 64: delivered frames 0.2442 ->
 * 0.2419 ms, one at a time 0.2734 -> 0.2712.  A decision that changes - cost order on / off, a streamed frame's bands - is
 * still acted on at once.  On a stream of its own the sort cost the delivered frames a third: one stream more, and the
 * runtime's four hardware queues are dealt out differently; on the copy stream it delays the images). */
const int SORT_PERIOD = 64;

/* The cost-ordered launch (renderer.h FrameArgs::tileCost / tileOrder; k_orderTiles in solr_post.hip): what the tiles of
 * the frames cost, the statistics the host decides by, and the launch order made from them.  renderImpl's scheduling
 * stage (solr_launch.hip) is the only code that advances it. */
struct TileSchedule
{
    int mode = 1;                 /* 0 off, 1 automatic (default), 2 always (solr_hip_set_tile_scheduling) */
    DeviceBuffer cost, costSnapshot;
    DeviceBuffer order[2];        /* the launch order; order[orderBuffer] holds the valid one */
    int orderBuffer = 0;
    hipEvent_t orderEvent = nullptr;  /* completion of the last tile sort */
    bool orderWait[MAX_FLIGHTS] = {}; /* that stream has not yet waited for it */
    unsigned *hostStats = nullptr;    /* mapped host memory, 8 words */
    unsigned *hostStatsDev = nullptr; /* its device address */
    long key[6] = {0, 0, 0, 0, 0, 0}; /* the frame geometry the recorded costs belong to */
    int frames = 0;                   /* frames rendered with that geometry */
    bool reorder = false;             /* current decision of the automatic mode */
    bool orderValid = false;          /* the order is one for the current geometry */
    BandCuts orderCuts = {};          /* ... band after band (ImageStreaming); bands = 0: by cost alone */
    /* the decision and the order forgotten: the next frames measure again (buffers, and an order a frame in flight reads,
     * stay as they are) */
    void reset()
    {
        frames = 0;
        reorder = false;
        orderValid = false;
    }
    void release(); /* everything given back, the mode kept (solr_launch.hip) */
};

/* solr_hip_set_variant (include/solr_hip.h): the A/B switches, by the numbers the C ABI takes.  Every one renders the same
 * frame. */
enum Variant
{
    VARIANT_AUTOMATIC = 0,
    VARIANT_EXACT_LIST = 3,      /* walk the node list exactly as uploaded */
    VARIANT_ALL_FEATURES = 4,    /* always the all-features kernel */
    VARIANT_NO_GROUPING = 5,     /* no grouping nodes (at the next h2d_scene) */
    VARIANT_NO_ORDER_FREE = 6,   /* no order-free lists */
    VARIANT_STACK_IN_LDS = 7,    /* the whole colour stack in LDS however deep a frame may bounce */
    VARIANT_REFERENCE_LEAVES = 8, /* no thin copies of the leaves that hold plain axis planes */
    VARIANT_AO_FIXED_STRIDE = 9, /* k_ambientOcclusion with a fixed stride of tiles per workgroup */
    VARIANT_NAN_DEEP_STACK = 10, /* NaNs in the colour-stack slots an F_STACK frame keeps in HBM, before every launch */
    VARIANT_UNSORTED_LISTS = 12, /* no walk takes the copies of the order-free lists with sorted bounds */
    VARIANT_NO_BAND_WORDS = 13,  /* a streamed frame's waves write no band's word */
    VARIANT_ZERO_STREAM_COUNTERS = 14, /* the tile counters of streamed frames zeroed every third frame */
    VARIANT_NO_LAMP_CUTOFF = 15, /* shadow walks in the reference's order keep the reference's cut-off alone */
    VARIANT_ALL_TRIPS = 16,      /* the trace makes the trips no lane takes: the deferred-reflection trip of a wave without
                                  * one, the gather and the shader call of a trip in which every lane missed */
    VARIANT_UPLOADED_BUILD_BOXES = 17, /* the order-free hierarchy is built on the leaves' boxes as uploaded, no leaf set
                                        * apart (build_bounds.h); the lists are built again with the next frame */
    VARIANT_UPLOADED_SPHERE_LEAVES = 18 /* the thin copies keep the boxes of sphere leaves as uploaded (the lamps' cell:
                                         * +-viewDistance); the copies are made again with the next frame */
};

/* ---- what a primitive's type and the facts of its material (materialTag, solr_uploads.hip) say about it.  Stated once:
 * retagPrimitives joins them into every tag on the host, k_setPrimitiveMaterials (solr_materials.hip) into the tags of a batch
 * on the device, and canSetPrimitiveMaterialsOne asks them what a batch would change. */
/* PrimKind (scene_layout.h): the short path the walks may take through the primitive */
__host__ __device__ inline int primitiveKind(int type, int facts)
{
    if (!(facts & PRIM_FAST0))
        return KIND_GENERAL; /* the closest-hit walk lets every lane of the leaf test a primitive with a kind */
    if (type == ptSphere && !(facts & PRIM_PROCEDURAL))
        return KIND_SPHERE;
    if ((type == ptXYPlane || type == ptYZPlane || type == ptXZPlane) && !(facts & (PRIM_TEXTURED | PRIM_WIRE2)) &&
        !(type == ptYZPlane && (facts & PRIM_EMISSIVE)))
        return type == ptXYPlane ? KIND_PLANE_XY : (type == ptYZPlane ? KIND_PLANE_YZ : KIND_PLANE_XZ);
    if (type == ptTriangle)
        return KIND_TRIANGLE;
    if (type == ptCylinder || type == ptCone)
        return KIND_CYLINDER;
    return KIND_GENERAL;
}
/* the tag word; noKinds (SOLR_HIP_NO_KINDS, tests): every primitive through the general tests */
__host__ __device__ inline int primitiveTag(int type, int facts, bool noKinds)
{
    return type | facts | ((noKinds ? (int)KIND_GENERAL : primitiveKind(type, facts)) << PRIM_KIND_SHIFT);
}
/* inside the box the reference's builder gives its leaf (GPUKernel.cpp:762-830: the vertices of a triangle, p0 +- radius of
 * a sphere, min / max (p0, p1) +- radius of a cylinder, p0 +- size of a plane; a cone's box is built around p0 alone, a
 * procedural sphere's surface is displaced, the others are not bounded by their size) */
inline bool primitiveContained(int type, int facts)
{
    return type == ptTriangle || type == ptCylinder || (type == ptSphere && !(facts & PRIM_PROCEDURAL)) || type == ptXYPlane ||
           type == ptYZPlane || type == ptXZPlane;
}
/* every occluder saturates a shadow (GI:880: intensity 1 x sceneInfo.shadowIntensity) unless it is transparent (GI:881-892
 * scales and tints) or a textured plane (its texel's alpha is the intensity, GI:553-558) */
inline bool primitiveShadowOpaque(int type, int facts)
{
    return !(facts & PRIM_TRANSPARENT) && !(facts & PRIM_TEXTURED) && type != ptCamera;
}
/* the features (rt_device.h enum Feature) a frame needs for it */
inline int primitiveFeatures(int type, int facts)
{
    int features = (facts & PRIM_TEXTURED) ? F_TEX : 0;
    switch (type)
    {
    case ptSphere:
    case ptEnvironment:
        return features | ((facts & PRIM_PROCEDURAL) ? F_PROC : F_SPHERE);
    case ptCylinder:
    case ptCone:
        return features | F_CYL;
    case ptEllipsoid:
        return features | F_ELL;
    case ptTriangle:
        return features | F_TRI;
    case ptCamera:
        return features | F_PLANE | F_TEX;
    default:
        return features | F_PLANE;
    }
}

/* A node list of the resident scene: its host image, the count a frame is told, where the arena holds it (the layout
 * itself is scene_layout.h's), and what is known about it.  Behind its rows the arena holds one pad record - the walk
 * requests the record after the node it tests (rt_device.h advanceTidy), after the last node too - then, for a list
 * kept in more than one copy, the thin copy (tightenList; rt_device.h tightRay) and the copy with sorted bounds
 * (k_sortNodeBounds), each padded alike: the functions below are the only place that knows where. */
struct NodeList
{
    int copies, lists; /* how often the arena holds the rows (1 ... 3); lists one behind the other (eight order-free ones) */
    explicit NodeList(int copies_ = 1, int lists_ = 1) : copies(copies_), lists(lists_) {}
    std::vector<float4> rows;       /* host image: two rows a node (list_builders.h) */
    std::vector<int> start, origin; /* ... its first primitive, the node of the reference's list it is (-1: ours) */
    int nb = 0;                     /* nodes per list, as a frame is told */
    unsigned offRows = 0, offLeaf = 0; /* float4 rows of the arena: node rows, leaf records (64 bytes a node) */
    unsigned offStart = 0;             /* ints of the arena: start indices */
    int ordered = 0;                /* sign-free slab test allowed on it */
    bool tight = false;             /* the thin copy behind it is up to date */
    std::vector<int> refitLevels;   /* [offset, count] per height, offsets into Refit::refitPlan (ints) */

    void reset() { *this = NodeList(copies, lists); }
    unsigned nodes() const { return (unsigned)lists * (unsigned)nb; }
    unsigned rowsOf(int list) const { return solrdev::listRows(offRows, (unsigned)nb, (unsigned)list); }
    unsigned offThin() const { return solrdev::listThin(offRows, nodes()); }
    unsigned offSorted() const { return solrdev::listSorted(offRows, nodes()); }
    /* the three parts of the layout: each takes the first free row and returns the next */
    unsigned layRows(unsigned row)
    {
        offRows = row;
        return row + (unsigned)copies * solrdev::listCopyRows(nodes());
    }
    unsigned layStart(unsigned row)
    {
        offStart = row * 4;
        return row + (nodes() + 3u) / 4u;
    }
    unsigned layLeaf(unsigned row)
    {
        row = (row + 3u) & ~3u; /* one 64-byte line per node */
        offLeaf = row;
        return row + 4u * nodes() + 4u;
    }
};

/* ---- the resident scene: what the device holds of it and what may be done with it ------------------------------------
 * Records cut by who writes them.  Every validity flag is assigned in the record's named transitions below and in the
 * three functions that derive state from the scene (retagPrimitives, deriveList, buildRefitPlan), nowhere else; a
 * default-constructed record is the state after initialize_scene, and release() gives the buffers back and returns to it. */

/* The arena of the geometry (scene_layout.h) against its host images.  Written by flushGeometry / appendFreeLists; told
 * that it is out of date by whoever changes a host image (retagPrimitives, h2d_lightInformation).  Part of Scene: no
 * transition moves its flags without moving the lists' or the refit's. */
struct Arena
{
    DeviceBuffer geometry;
    unsigned offPrims = 0, offLights = 0; /* float4 rows of the arena */
    unsigned rowsFixed = 0;               /* rows of the arena in front of the order-free lists */
    bool geometryDirty = true;            /* a host image changed: laid out and uploaded again by the next flushGeometry */
    bool deviceAhead = false;             /* the arena has moved on from the host images (rotations on the device) */
    void layOutAgain() { geometryDirty = true; }
};
/* The state of the order-free lists (Scene::orderFree).  Lists built on the device stay there and go into the arena with
 * a device-to-device copy (freeStage, until the next flushGeometry); orderFree's host image is filled from the arena
 * when somebody needs it (ensureHostFreeLists: the refit plan of a rotated scene, a second layout). */
struct OrderFreeState
{
    int freeCountdown = 0;     /* renders until the order-free lists are built (0: not scheduled) */
    bool freeHostValid = true; /* orderFree's host image is the lists (false: they are staged or in the arena alone) */
    bool freeDirty = false;    /* the staged lists are to be added to an arena that is otherwise up to date */
    SolrDeviceLists freeStage;
    bool freeStale = false;    /* rotated on the device since it was built: not refitted, not walked */
    bool sortedFree = false;   /* the copy of the order-free lists with sorted bounds is up to date (deriveList) */
    /* the buffers the device builder left its lists in: rows and start indices until they are in the arena, the origins
     * (only the refit plan reads them) until the host has them or the lists go */
    void dropStage(bool originToo)
    {
        if (freeStage.rows)
            (void)hipFree(freeStage.rows);
        if (freeStage.start)
            (void)hipFree(freeStage.start);
        freeStage.rows = nullptr;
        freeStage.start = nullptr;
        if (originToo && freeStage.origin)
        {
            (void)hipFree(freeStage.origin);
            freeStage.origin = nullptr;
        }
    }
};
/* The refit of the node lists behind primitives that moved on the device (refitMovedScene, solr_rotation.hip): which
 * primitives move, what to refit, in which order.  Written by solr_hip_set_movable, buildRefitPlan and the transitions of
 * Scene. */
struct Refit
{
    DeviceBuffer movable, refitPlan;
    DeviceBuffer enclosesFlag;     /* k_listEncloses' answer */
    int nbMovable = -1;            /* flags uploaded for that many primitives, -1: none */
    bool refitReady = false;       /* refitPlan is the plan of the lists as they are (buildRefitPlan) */
    bool refitPlanPending = false; /* the lists changed: the plan is made when the first request asks (canRefitOne) */
    bool exactStale = false;       /* the exact list has not been refitted since the last move */
    float exactStaleViewDistance = 0.f;
};
/* The requests a host makes on the resident scene in place of a new upload, and what each of them does to the scene's
 * record when it has been served (Scene::requestServed reads the table; the engine counts them: Engine::served).
 * movesBounds: primitives moved and refitMovedScene refitted the lists - the walk-order list was checked again and the arena
 * is ahead of the host images.  barsMorph: a morph on that scene would undo part of it, and is declined until the next
 * h2d_scene - a moved lamp's p0 would go back to the keys' place and leave its light record behind (the host route makes
 * the record from p0 again), set primitives would lose their texture coordinates and movable flags, set materials would
 * stay where the host's morph takes its first key's.  A lamp move and a batch of materials are written to the arena and
 * the host images alike: nothing is ahead of anything by them. */
enum RequestKind
{
    REQUEST_ROTATION = 0,
    REQUEST_TRANSLATION,
    REQUEST_LAMP_MOVE,
    REQUEST_EDIT,          /* primitives set anew (solr_edits.hip) */
    REQUEST_MATERIAL_SETS, /* primitives' materials set (solr_materials.hip) */
    REQUEST_MORPH,         /* through the two-key interface */
    REQUEST_TRACK_MORPH,   /* between two slots of a track */
    REQUEST_KINDS
};
struct RequestFacts
{
    bool movesBounds, barsMorph;
};
constexpr RequestFacts REQUEST_FACTS[REQUEST_KINDS] = {
    {true, false},  /* rotation */
    {true, false},  /* translation */
    {false, true},  /* lamp move */
    {true, true},   /* edit */
    {false, true},  /* material sets */
    {true, false},  /* morph */
    {true, false}}; /* track morph */
/* Key-frame morphing on the device (solr_morph.hip): the key frames of the resident scene the engine holds, one per slot -
 * the slots of a track (solr_hip_set_morph_track_key, solr_hip_morph_between), then the two of the two-key interface
 * (solr_hip_set_morph_keys, solr_hip_morph_primitives).  Written by the transitions of Scene only; an h2d_scene drops the keys. */
enum MorphSlot
{
    MORPH_SLOT_FIRST = SOLR_MORPH_TRACK_MAX_KEYS, /* solr_hip_set_morph_keys' first key frame */
    MORPH_SLOT_LAST,                              /* ... and its last */
    MORPH_SLOTS
};
struct MorphKey
{
    DeviceBuffer planes;   /* seven planes of nbPrimitives float4 each: p0 p1 p2 n0 n1 n2 size (the buffer stays for the next key) */
    int nbPrimitives = -1; /* the key is for that many primitives, -1: the slot holds none */
};
/* the lamp rule's answer for an ordered pair of slots: a primitive tagged PRIM_EMISSIVE has rows that differ between them */
struct MorphLampAnswer
{
    int slotA, slotB;
    bool moves;
};
struct Morph
{
    MorphKey keys[MORPH_SLOTS];
    int nbTrackKeys = 0;                      /* of the track's slots, those that hold a key */
    std::vector<MorphLampAnswer> lampAnswers; /* as asked since the slots last changed, by the tags of ... */
    long lampChecked = -1;                    /* ... that Scene::retags */
    DeviceBuffer lampFlag;                    /* k_lampKeysDiffer's answer */
};
/* The scene proper: what h2d_scene replaces and finalize_scene drops, with the arena it is resident in. */
struct Scene
{
    /* the node lists: the reference's as uploaded; the walk-order list (chains collapsed, siblings grouped, inner nodes
     * that hardly cull pruned) with its thin copy; the eight order-free lists, one per direction octant - the leaves of
     * the scene under a surface-area hierarchy of our own (buildFreeOrderLists) - with thin and sorted copies */
    NodeList exact = NodeList(1, 1), walk = NodeList(2, 1), orderFree = NodeList(3, solrdev::ORDER_FREE_LISTS);
    std::vector<float4> hostPrims; /* host image of the primitive records */
    int nbPrimitives = 0;
    DeviceBuffer lamps;
    int nbLamps = 0;
    int nested = 1;
    /* the walk-order list as the arena holds it: every inner node contains its children, every leaf its primitives
     * (checked at h2d_scene and again after every rotation on the device; lampCutoffUsable, tightListsFor) */
    bool walkEncloses = false;
    OrderFreeState lists;
    Refit refit;
    Morph morph;
    unsigned morphBarredBy = 0; /* the kinds (1 << RequestKind) served since h2d_scene that bar a morph (REQUEST_FACTS) */
    /* the batches as uploaded last: of primitives set anew (solr_edits.hip: its planes), of materials set (solr_materials.hip) */
    DeviceBuffer editBatch, materialSetBatch;
    long retags = 0; /* how often retagPrimitives has run: what was derived from the tags is as old as that */
    Arena arena;

    /* every byte of device memory the record owns (the staged order-free lists by what the builder leaves per node:
     * lists_device.h) */
    size_t deviceBytes() const
    {
        size_t bytes = arena.geometry.bytes + lamps.bytes + refit.movable.bytes + refit.refitPlan.bytes +
                       refit.enclosesFlag.bytes + editBatch.bytes + materialSetBatch.bytes + morph.lampFlag.bytes;
        for (const MorphKey &key : morph.keys)
            bytes += key.planes.bytes;
        const size_t nodes = orderFree.nodes();
        bytes += (lists.freeStage.rows ? nodes * 32 : 0) + (lists.freeStage.start ? nodes * 4 : 0) +
                 (lists.freeStage.origin ? nodes * 4 : 0);
        return bytes;
    }

    /* h2d_scene has new host images of the lists and the primitives (swapped in by the caller): nothing that was made
     * from the old ones holds.  The movable flags and the morph keys go, and nothing bars a morph any more; the arena
     * follows with retagPrimitives (layOutAgain) */
    void newGeometry(int nested_, bool walkEncloses_, int freeCountdown_)
    {
        nested = nested_;
        walkEncloses = walkEncloses_;
        refit.refitReady = false;
        refit.exactStale = false;
        refit.refitPlanPending = true;
        refit.nbMovable = -1;
        morphBarredBy = 0;
        morphKeysDropped();
        arena.deviceAhead = false;
        orderFree.reset();
        lists.freeCountdown = freeCountdown_;
        lists.freeHostValid = true;
        lists.freeDirty = false;
        lists.dropStage(true);
        lists.freeStale = false;
    }
    /* a frame has been rendered: true when the order-free lists are due now (maybeBuildOrderFreeLists) */
    bool orderFreeDue() { return lists.freeCountdown > 0 && --lists.freeCountdown == 0; }
    /* ... and no walk would take them yet (orderFreeListsUsable): asked again with the next frame */
    void orderFreeAskAgain() { lists.freeCountdown = 1; }
    /* what the lists are built on has changed (VARIANT_UPLOADED_BUILD_BOXES set or taken back): lists that exist are built
     * again with the next frame; a scene that is still waiting for its own goes on waiting */
    void orderFreeBuildAgain()
    {
        if (orderFree.nb > 0 && lists.freeCountdown == 0)
            lists.freeCountdown = 1;
    }
    /* maybeBuildOrderFreeLists has built them; stayed: on the device (lists.freeStage), fromArena: made from an arena
     * that is up to date.  They join the arena with the next flushGeometry: added behind what it holds when both, else
     * laid out and uploaded again */
    void orderFreeBuilt(const NodeList &built, bool stayed, bool fromArena)
    {
        orderFree = built;
        lists.freeHostValid = !stayed;
        lists.freeStale = false;
        refit.refitReady = false;
        refit.refitPlanPending = true; /* 8-12 ms for 100 k primitives: only scenes that are rotated on the device pay them */
        if (stayed && fromArena)
            lists.freeDirty = true;
        else
            arena.layOutAgain();
    }
    /* appendFreeLists / flushGeometry: the arena holds the staged lists / everything the host images hold */
    void listsAppended()
    {
        lists.dropStage(false);
        lists.freeDirty = false;
    }
    void arenaFlushed()
    {
        arena.geometryDirty = false;
        lists.freeDirty = false;
    }
    /* ensureHostFreeLists / pullGeometry: the host images are what the device holds again (the next layout takes the
     * lists from their host image) */
    void hostListsPulled()
    {
        lists.freeHostValid = true;
        lists.dropStage(true);
    }
    void hostImagesPulled() { arena.deviceAhead = false; }
    /* refitMovedScene - behind a request that moves primitives - has queued the refit of the walk-order list (listsFollow:
     * of the order-free lists too; without a plan for them, moved scenes walk the reference's order until the next upload);
     * the reference's own list follows when somebody needs it (refreshExactList) */
    void refitQueued(bool listsFollow, float viewDistance)
    {
        if (!listsFollow)
            lists.freeStale = orderFree.nb > 0;
        refit.exactStale = true;
        refit.exactStaleViewDistance = viewDistance;
    }
    void exactRefitted() { refit.exactStale = false; }
    /* a ...One (solr_rotation.hip, solr_moves.hip, solr_edits.hip, solr_materials.hip, solr_morph.hip) has served a request
     * of that kind.  walkHolds - asked of a kind that moves bounds only -: the refitted walk-order list passed the check
     * again, and that is taken whether or not the request landed; landed: without an error.  The engine counts it
     * (finishRequest).  A batch of materials also retags: whoever derived something from the tags hears through retagged() */
    void requestServed(RequestKind kind, bool walkHolds, bool landed)
    {
        const RequestFacts &facts = REQUEST_FACTS[kind];
        if (facts.movesBounds)
            walkEncloses = walkHolds;
        if (!landed)
            return;
        if (facts.movesBounds)
            arena.deviceAhead = true;
        if (facts.barsMorph)
            morphBarredBy |= 1u << kind;
    }
    /* retagPrimitives has joined the materials' facts into the primitives' tags again (setPrimitiveMaterialsOne: into some) */
    void retagged() { ++retags; }
    /* the morph keys: every slot empty (the buffers stay for the next keys) / one slot empty / one slot packed for
     * nbPrimitives primitives.  What was answered about lamps held for the slots as they were */
    void morphKeysDropped()
    {
        for (MorphKey &key : morph.keys)
            key.nbPrimitives = -1;
        morph.nbTrackKeys = 0;
        morph.lampAnswers.clear();
    }
    void morphKeyDropped(int slot)
    {
        if (slot < SOLR_MORPH_TRACK_MAX_KEYS && morph.keys[slot].nbPrimitives >= 0)
            --morph.nbTrackKeys;
        morph.keys[slot].nbPrimitives = -1;
        morph.lampAnswers.clear();
    }
    void morphKeySet(int slot, int nbPrimitives_)
    {
        morphKeyDropped(slot);
        morph.keys[slot].nbPrimitives = nbPrimitives_;
        if (slot < SOLR_MORPH_TRACK_MAX_KEYS)
            ++morph.nbTrackKeys;
    }
    /* canMorphOne has asked the tags as they are now whether a lamp's rows differ between the two slots */
    void morphLampNoted(int slotA, int slotB, bool moves)
    {
        if (morph.lampChecked != retags)
            morph.lampAnswers.clear();
        morph.lampChecked = retags;
        morph.lampAnswers.push_back({slotA, slotB, moves});
    }
    /* finalize_scene */
    void release()
    {
        lists.dropStage(true);
        for (DeviceBuffer *b : {&arena.geometry, &lamps, &refit.movable, &refit.refitPlan, &refit.enclosesFlag, &editBatch,
                                &materialSetBatch, &morph.lampFlag})
            solreng::release(*b);
        for (MorphKey &key : morph.keys)
            solreng::release(key.planes);
        *this = Scene();
    }
};
/* Where the arena holds the leaf records of the resident node lists, for a kernel that patches them in place behind a
 * change of some primitives' words (solr_moves.hip k_moveLamp, solr_materials.hip k_followLeafRecords): one thread per node,
 * one list behind the other. */
struct LeafRecordsOf
{
    unsigned offRows, offStart, offLeaf; /* of a node list (NodeList) */
    int nodes;                           /* 0: the arena holds no leaf records of that list */
};
/* ... of the exact, the walk-order and the order-free lists of `scene`; returns the nodes in all */
inline int leafRecordsOfLists(const Scene &scene, LeafRecordsOf out[3])
{
    int total = 0, l = 0;
    for (const NodeList *list : {&scene.exact, &scene.walk, &scene.orderFree})
    {
        const bool none = list == &scene.orderFree && scene.lists.freeStale; /* (deriveList: a stale list has none) */
        out[l].offRows = list->offRows;
        out[l].offStart = list->offStart;
        out[l].offLeaf = list->offLeaf;
        out[l].nodes = none ? 0 : (int)list->nodes();
        total += out[l].nodes;
        ++l;
    }
    return total;
}
/* Lights (h2d_lightInformation): their records lie in the arena behind the primitives'.  h2d_scene keeps them,
 * finalize_scene drops them. */
struct Lights
{
    std::vector<float4> hostLights;
    int nbLights = 0;
};
/* texture tables of a textured material: checked against the atlas (checkTextureTables) */
struct TextureUse
{
    int material;
    long texels;     /* bytes of the diffuse map: x * y * depth */
    long offsets[7]; /* diffuse, normal, bump, specular, reflection, transparency, ambient occlusion; -1 unused */
};
/* Materials (h2d_materials) */
struct Materials
{
    DeviceBuffer table; /* NB_MAX_MATERIALS + 1 hot records, then as many cold ones (offMatCold, float4 rows) */
    unsigned offMatCold = 0;
    int nbMaterials = 0;
    std::vector<int> materialTags;      /* PRIM_* bits per material id */
    std::vector<float> materialAverage; /* (r + g + b) / 3.f per material id (plane colour key, GI:561) */
    std::vector<TextureUse> textureUses;
    long generation = 0; /* how often h2dMaterialsOne has run: a scene's tags are those of one table (ParkedScene) */
    /* host image of the active records as the table holds them (h2dMaterialsOne, editMaterialsOne: solr_materials.hip),
     * zero-filled before it was filled; nbImaged records of each, -1: no image */
    std::vector<solrdev::MaterialHot> imageHot;
    std::vector<solrdev::MaterialCold> imageCold;
    int nbImaged = -1;
    /* materials edited in the table and on the resident scene (solr_materials.hip): the batch of changed materials as
     * uploaded last; requests served since initialize_scene, and those among them that launched k_retagMaterials */
    DeviceBuffer editBatch;
    int nbDeviceEdits = 0, nbDeviceRetags = 0;
    void release()
    {
        solreng::release(table);
        solreng::release(editBatch);
        *this = Materials();
    }
};
/* what h2d_materials makes of one material (solr_uploads.hip materialRecord): its two records of the table, the facts its
 * primitives' tags carry, their colour key, and - textured: the tables checkTextureTables holds against the atlas */
struct MaterialRecord
{
    int facts;
    float average;
    bool textured;
    TextureUse use;
};
/* Textures (h2d_textures): the atlas, and whether the materials' texture tables have been checked against it - before the
 * first frame that follows either upload (checkTextureTables; kept here: the atlas is what the check protects) */
struct Textures
{
    DeviceBuffer atlas;
    size_t atlasBytes = 0;
    bool textureTablesChecked = false;
    void release()
    {
        solreng::release(atlas);
        *this = Textures();
    }
};
/* Randoms (h2d_randoms, solr_hip_h2d_randoms_sized; with a communicator rank 0's: shareRandoms) */
struct Randoms
{
    DeviceBuffer values;
    long nbRandoms = 0;
    float randomsReach = 0.f; /* max |randoms[i]|, i < 356: what the 256 taps can read */
    void release()
    {
        solreng::release(values);
        *this = Randoms();
    }
};
/* What retagPrimitives derives from the primitives and the materials, after every upload of either */
struct SceneFacts
{
    bool primsContained = false; /* every primitive lies inside its leaf's box */
    bool opaqueShadows = false;  /* no transparent primitive, no textured plane */
    bool plainPlanes = false;    /* the scene holds a plain axis plane: thin copies are worth making (tightenList) */
    float sceneExtent = 1.f;     /* max |coordinate| + |size| over the primitives, at least 1 */
    bool looseSpheres = false;   /* a leaf of nothing but KIND_SPHEREs is boxed larger than they are (the lamps' cell) */
    /* the reach the thin boxes of sphere leaves are made for (build_bounds.h sphereBuildExtent; solr_arena.hip
     * thinReachWanted): the scene's extent, or the viewDistance beyond it of the frame that last walked them (prepareScene
     * has the copies made again); 0: such leaves keep their boxes */
    float thinReach = 0.f;
    float frameViewDistance = 0.f; /* of the frame prepared last (prepareScene), 0: none yet - the reach a retag starts from */
    int sceneFeatures = F_ALL & ~F_FULL; /* rt_device.h enum Feature */
    /* the counts behind primsContained, opaqueShadows and sceneFeatures, kept by retagPrimitives: a batch of materials set
     * on the resident scene (solr_materials.hip) takes its primitives out with their old facts and in with their new ones,
     * and the three are exact again without a pass over the primitives */
    static const int FEATURE_BITS = 7; /* F_SPHERE ... F_TEX */
    int nbCounted = 0, nbUncontained = 0, nbShadowTinting = 0;
    int featureUsers[FEATURE_BITS] = {};
    void forgetCounts()
    {
        nbCounted = nbUncontained = nbShadowTinting = 0;
        for (int &users : featureUsers)
            users = 0;
    }
    /* by: +1 a primitive of that type and those facts joins the scene, -1 it leaves */
    void count(int type, int facts, int by)
    {
        nbCounted += by;
        nbUncontained += primitiveContained(type, facts) ? 0 : by;
        nbShadowTinting += primitiveShadowOpaque(type, facts) ? 0 : by;
        const int features = primitiveFeatures(type, facts);
        for (int bit = 0; bit < FEATURE_BITS; ++bit)
            if (features & (1 << bit))
                featureUsers[bit] += by;
    }
    void deriveFromCounts()
    {
        primsContained = nbUncontained == 0 && nbCounted > 0;
        opaqueShadows = nbShadowTinting == 0 && nbCounted > 0;
        sceneFeatures = 0;
        for (int bit = 0; bit < FEATURE_BITS; ++bit)
            if (featureUsers[bit] > 0)
                sceneFeatures |= 1 << bit;
    }
};
/* A resident scene set aside (solr_hip_park_scene, solr_bank.hip): the three records h2d_scene, h2d_lightInformation and
 * retagPrimitives write, moved - a DeviceBuffer is a plain pointer, the vectors move - with everything made from them or
 * applied to them since.  Nothing is copied, launched, freed or waited for: a frame in flight that still reads the arena
 * finishes, because the arena stays allocated.  (The counts of requests served are the engine's - Engine::served - and no
 * scene's: nothing of them moves.) */
struct ParkedScene
{
    int key = -1;
    Scene scene;
    Lights lights;
    SceneFacts facts;
    long materialsGeneration = 0; /* Materials::generation the tags were joined under */
    size_t bytes = 0;             /* Scene::deviceBytes when it was parked */
    /* the resident records move in; the engine holds no scene, as after initialize_scene */
    void park(int key_, Scene &resident, Lights &residentLights, SceneFacts &residentFacts, long generation)
    {
        key = key_;
        bytes = resident.deviceBytes();
        materialsGeneration = generation;
        scene = std::move(resident);
        lights = std::move(residentLights);
        facts = residentFacts;
        resident = Scene();
        residentLights = Lights();
        residentFacts = SceneFacts();
    }
    /* ... and out again, over records that hold no buffer (the caller has released them) */
    void resume(Scene &resident, Lights &residentLights, SceneFacts &residentFacts)
    {
        resident = std::move(scene);
        residentLights = std::move(lights);
        residentFacts = facts;
        scene = Scene();
        lights = Lights();
        facts = SceneFacts();
        bytes = 0;
        key = -1;
    }
};
/* The scene bank (solr_bank.hip): the parked scenes of this engine, its limit - a knob - and what it has counted since
 * initialize_scene */
struct SceneBank
{
    std::vector<ParkedScene> parked;
    unsigned long long limitBytes = 0; /* solr_hip_set_scene_bank_bytes; 0: every park is declined */
    int nbSwitches = 0;                /* resumes served */
    int nbUploads = 0;                 /* h2d_scene calls served */
    int find(int key) const
    {
        for (size_t i = 0; i < parked.size(); ++i)
            if (parked[i].key == key)
                return (int)i;
        return -1;
    }
    unsigned long long bytes() const
    {
        unsigned long long sum = 0;
        for (const ParkedScene &p : parked)
            sum += p.bytes;
        return sum;
    }
};
/* The kernel timer (solr_hip_enable_timing: Engine::timing; solr_launch.hip, solr_diag.hip) */
struct KernelTimer
{
    unsigned timingTick = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    double timedMs = 0.0;
    int timedLaunches = 0;
    std::vector<float> kernelSamples, intervalSamples; /* per timed launch: its duration; end-to-end gap to the one before */
};
/* The walk's own ceiling (solr_hip_walk_bound): the next frame records its walks; how that frame was launched
 * (solr_launch.hip, solr_diag.hip) */
struct WalkRecording
{
    DeviceBuffer walkRecords, walkVisits;
    bool recordNext = false;
    bool recorded = false;
    unsigned recordGrid = 0;
    size_t recordLds = 0;
    int recordVariant = -1; /* row of solrrows::ROWS (renderer.h) */
    bool recordDeep = false;
    SceneArgs recordScene = {};
    void release()
    {
        solreng::release(walkRecords);
        solreng::release(walkVisits);
        *this = WalkRecording();
    }
};

/* JPEG frames in flight (solr_jpeg_entropy.hip; solr_hip_frame_to_jpeg_async, solr_hip_jpeg_wait): a slot is everything
 * one frame's JPEG takes on the device, allocated at the first use for a number of blocks and kept - until reshape_scene,
 * finalize_scene or a frame of more blocks - so that a submission allocates nothing and waits for nothing.  One device
 * allocation, cut into: the pixel stage's tables and the coefficient blocks; the bit items and their offsets; hipcub's
 * temporaries for both scans; the unstuffed stream, the chunks' 0xFF counts and their offsets, the stuffed output (stream
 * and output sized for the worst frame the tables allow: jpn::maxStreamBytes, jpn::maxStuffedBytes - nothing overflows);
 * histogram and tables of the optimised mode; and the small record the steps hand each other, whose page-locked host copy
 * is all that comes back with the event.  Tickets carry their generation as the image ring's do. */
const int JPEG_SLOTS = MAX_FLIGHTS;
struct JpegSlot
{
    DeviceBuffer block;
    long capacityBlocks = 0;                   /* coefficient blocks the cuts below were made for */
    size_t scanBytes = 0, chunkScanBytes = 0;  /* hipcub's temporaries */
    size_t streamBytes = 0;                    /* of the unstuffed stream's buffer */
    unsigned char *encodeTables = nullptr, *coefficients = nullptr, *bits = nullptr, *offsets = nullptr, *scanTemp = nullptr,
                  *stream = nullptr, *counts = nullptr, *before = nullptr, *chunkScanTemp = nullptr, *out = nullptr,
                  *histogram = nullptr, *tables = nullptr, *record = nullptr;
    void *hostRecord = nullptr; /* page-locked: flag, total bits, stuffed size, the optimised tables */
    hipEvent_t done = nullptr;  /* behind the read-back of the record */
    bool used = false;          /* `done` has been recorded */
    bool clean = false;         /* the stream's buffer is zero once the work before `done` is through */
    long serial = -1;           /* of the ticket that holds the slot, -1: none */
    long nbBlocks = 0;
    bool optimised = false, fromFrame = false, collected = false;
};
/* what a slot held before it was made anew for a frame of more blocks: given back once `done` has come (asked, never
 * waited for, by the submissions that follow; waited for by JpegStream::release) */
struct JpegRetired
{
    DeviceBuffer block;
    void *hostRecord = nullptr;
    hipEvent_t done = nullptr;
};
struct JpegStream
{
    JpegSlot slot[JPEG_SLOTS];
    std::vector<JpegRetired> retired;
    static const size_t RETIRED_MOST = 2 * JPEG_SLOTS; /* beyond that a submission waits for the oldest, and counts it */
    long issued = 0;                    /* tickets handed out since the library was loaded: never reset */
    hipStream_t probeStream = nullptr;  /* solr_hip_probe_jpeg_stream_blocks uploads and runs here */
    hipStream_t copyStream = nullptr;   /* solr_hip_jpeg_wait's copy of the segment */
    unsigned long long allocations = 0, hostWaits = 0, bytesDelivered = 0;
    /* a ticket is (serial mod TICKET_PERIOD) * JPEG_SLOTS + slot, the slot serial mod JPEG_SLOTS (ImageRing::ticketOf) */
    static const long TICKET_PERIOD = ((long)0x7fffffff / JPEG_SLOTS / JPEG_SLOTS - 1) * JPEG_SLOTS;
    static int ticketOf(long serial) { return (int)((serial % TICKET_PERIOD) * JPEG_SLOTS + serial % JPEG_SLOTS); }
    void release(); /* every slot's last use waited for, its memory given back, its ticket void (solr_jpeg_entropy.hip) */
};

struct Engine
{
    bool initialized = false;
    int device = 0;
    int errorCode = 0;
    std::string errorText;

    /* the knobs: set by the host, they outlive finalize_scene (no release() resets them; initialize_scene hands engine
     * 0's to the engines of further devices) */
    int variant = VARIANT_AUTOMATIC; /* enum Variant */
    bool grouping = true; /* groupSiblings(); VARIANT_NO_GROUPING turns it off for A/B measurements */
    /* bounce rays on the order-free lists, checked (rt_device.h closestHitWalk): -1 the engine decides per frame
     * (shortRayListsChoice: with frames in flight), 0 / 1 forced */
    int shortRayListsMode = -1;
    int flights = 1;         /* how many frames in flight were asked for (solr_hip_set_frames_in_flight; in use: activeFlights) */
    bool tileClocks = false; /* diagnostics, solr_hip_enable_tile_clocks */
    int timing = 0;          /* 0 off, n: every n-th launch is bracketed with events (KernelTimer) */
    /* (and sched.mode, TileSchedule) */

    /* the resident scene */
    Scene scene;
    Lights lights;
    Materials materials;
    Textures textures;
    Randoms randoms;
    SceneFacts facts;
    SceneBank bank; /* the scenes set aside (its limit is a knob) */
    /* the requests on the resident scene this engine has served, per RequestKind (solr_hip_device_rotations and its
     * siblings): counted by finishRequest, zeroed by finalize_scene and by nothing else - not by a second initialize_scene
     * on an engine that is up, not by h2d_scene, not when scenes change places in the bank */
    int served[REQUEST_KINDS] = {};

    DeviceBuffer counters, tileClock;
    /* ambient occlusion across strips: the depths of the neighbours' rows a host hands over itself (the ones traded over
     * RCCL: Flight) */
    DeviceBuffer haloGivenAbove, haloGivenBelow; /* solr_hip_set_depth_halo */
    int haloSuppliedAbove = 0, haloSuppliedBelow = 0; /* rows handed over by solr_hip_set_depth_halo (0: none) */
    int haloWanted = -1; /* rows beyond a strip the last frame's post-processing reached (0: none; -1: no frame here) */
    /* the frames in flight: their streams and per-pixel buffers.  flight[0]'s stream is also the one uploads and list
     * kernels run on (sceneStream) */
    Flight flight[MAX_FLIGHTS];
    bool ownStream = false;     /* flight[0]'s stream is the engine's own (else the caller's: solr_hip_set_stream) */
    bool callerStreams = false; /* the streams of the other flights belong to the caller (solr_hip_set_flight_streams) */
    int current = 0;            /* flight of the last render */
    unsigned frameSerial = 0;
    TileSchedule sched;
    unsigned lastSerial = 0;
    int nbTilesTimed = 0;
    void *boundBitmap = nullptr;
    int width = 0, height = 0;       /* full image */
    int frameBufferType = -1;        /* the channel order of the frame rendered last (-1: none yet); solr_hip_frame_to_jpeg_scan */
    int firstRow = 0, nbRows = -1;   /* strip; nbRows < 0 -> full frame, 0 -> this process renders no row */
    int allocW = 0, allocRows = 0;

    KernelTimer timer;
    WalkRecording recording;

    CopyLane copyLane;        /* this device's part of the pipelined read-back (the ring of host images: gImageRing) */
    ImageStreaming streaming; /* the read-back of a frame taken one at a time, in bands */
    JpegStream jpeg;          /* JPEG frames in flight: the resident slots and their tickets */
    /* the reciprocal of tilesX that was verified for a frame geometry (renderImpl) */
    int tileCheckedX = 0, tileCheckedTiles = 0, tileCheckedShift = 0;
    unsigned tileCheckedMagic = 0;
    int lastMask = -1;                  /* features of the lean row the frame before took (-1: another kernel, or none yet) */
    /* what the frame rendered last launched (solr_hip_probe_last_frame): its row of solrrows::ROWS (-1: none), the features of
     * its instantiation with F_DEEP / F_STACK / F_STREAM, streamed (1 / 0) and in how many bands, cost-ordered (1 / 0) and
     * the bands of that order */
    int lastFrame[6] = {-1, -1, 0, 0, 0, 0};
};

/* One Engine per device this process renders on.  The reference drives occupancyParameters.x devices from ONE host
 * thread - per-device allocations and uploads (CudaRayTracer.cu:1404-1480, 1536-1625), one launch per device on an
 * equal row strip (:1694-1696, 1709-1815), every device's strip copied to its place in the host arrays (:1647-1672) -
 * and so does this library when initialize_scene is handed occupancyParameters.x > 1: the ten entry points of the
 * boundary then run once per engine (the wrappers at the end of the C ABI), each engine on its own device with its
 * own streams, buffers and error state, the scene replicated, the frame shared out in equal row strips.  Engine 0
 * always exists and is the engine of every one-device process (all the multi-process machinery: strips, RCCL).
 * `g` is the engine a function works on. */
extern Engine gFirst;
extern Engine *gEngines[SOLR_MAX_GPU_COUNT];
extern int gDevices;   /* engines in use since initialize_scene: min(occupancyParameters.x, devices visible) */
extern int gRequested; /* occupancyParameters.x as initialize_scene was given it */
extern Engine *gCurrent;
#define g (*gCurrent)
template <class F>
void onEveryDevice(F &&f)
{
    for (int d = 0; d < gDevices; ++d)
    {
        gCurrent = gEngines[d];
        if (gDevices > 1)
            (void)hipSetDevice(g.device); /* (allocations and launches go to the calling thread's device) */
        f(d);
    }
    gCurrent = &gFirst;
    if (gDevices > 1)
        (void)hipSetDevice(g.device);
}

/* how many frames may really be in flight: what was asked for, as far as streams exist */
inline int activeFlights()
{
    if (g.flights < 2 || !(g.ownStream || g.callerStreams))
        return 1;
    int n = 1;
    while (n < g.flights && n < MAX_FLIGHTS && g.flight[n].stream)
        ++n;
    return n;
}
inline bool twoFlights() { return activeFlights() > 1; }
/* the stream uploads, list kernels and everything else that is not a frame run on */
inline hipStream_t sceneStream() { return g.flight[0].stream; }
/* nothing may touch scene or frame buffers while a frame is still in flight on the other stream */
inline void quiesce()
{
    for (int f = 1; f < MAX_FLIGHTS; ++f)
        if (g.flight[f].stream)
            (void)hipStreamSynchronize(g.flight[f].stream);
    if (g.flight[0].stream)
        (void)hipStreamSynchronize(g.flight[0].stream);
    if (g.copyLane.stream)
        (void)hipStreamSynchronize(g.copyLane.stream);
}

inline void setError(int code, const char *what, const char *file, int line)
{
    if (g.errorCode != 0)
        return;
    g.errorCode = code;
    char buf[512];
    snprintf(buf, sizeof(buf), "%s (%s:%d)", what, file, line);
    g.errorText = buf;
    fprintf(stderr, "solr_hip: error %d: %s\n", code, buf);
    const char *fatal = getenv("SOLR_HIP_FATAL");
    if (fatal && fatal[0] == '1')
        exit(EXIT_FAILURE); /* the reference's behaviour, helper_cuda.h:749-763 */
}

#define HIPCHECK(expr)                                                                                           \
    do                                                                                                           \
    {                                                                                                            \
        hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess)                                                                                    \
        {                                                                                                        \
            std::string m_ = std::string(#expr) + ": " + hipGetErrorString(e_);                                  \
            setError((int)e_, m_.c_str(), __FILE__, __LINE__);                                                   \
        }                                                                                                        \
    } while (0)

#define ARGCHECK(cond, msg)                                                                                      \
    do                                                                                                           \
    {                                                                                                            \
        if (!(cond))                                                                                             \
            setError(-1, msg, __FILE__, __LINE__);                                                               \
    } while (0)

inline bool ok()
{
    return g.errorCode == 0;
}

inline bool ready(const char *who)
{
    if (!ok())
        return false;
    if (!g.initialized)
    {
        setError(-1, (std::string(who) + ": initialize_scene has not been called").c_str(), __FILE__, __LINE__);
        return false;
    }
    return true;
}

/* grow-only device allocation */
inline void reserve(DeviceBuffer &b, size_t bytes)
{
    if (bytes < 16)
        bytes = 16;
    if (b.ptr && b.bytes >= bytes)
        return;
    release(b);
    HIPCHECK(hipMalloc(&b.ptr, bytes));
    if (ok())
        b.bytes = bytes;
}

template <class T>
void upload(DeviceBuffer &b, const std::vector<T> &host)
{
    reserve(b, host.size() * sizeof(T));
    if (ok() && !host.empty())
    {
        /* pageable source: the copy is complete for the caller when this returns */
        HIPCHECK(hipMemcpyAsync(b.ptr, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, sceneStream()));
        HIPCHECK(hipStreamSynchronize(sceneStream()));
    }
}

inline int stripRows()
{
    return g.nbRows >= 0 ? g.nbRows : g.height;
}


/* ---- what the parts ask of each other (defined in the file named) ---------------------------------------------------- */
/* solr_uploads.hip: one engine's share of the boundary's h2d_* calls */
void h2dSceneOne(BoundingBox *boundingBoxes, int nbActiveBoxes, Primitive *primitives, int nbPrimitives, Lamp *lamps, int nbLamps);
void h2dMaterialsOne(Material *materials, int nbActiveMaterials);
/* material i of a table as the device gets it: `hot` and `cold` (zero-filled by the caller) filled in, the rest returned */
MaterialRecord materialRecord(const Material &material, int i, solrdev::MaterialHot &hot, solrdev::MaterialCold &cold);
void h2dRandomsOne(float *randoms);
void h2dRandomsSizedOne(const float *randoms, long count);
void h2dTexturesOne(int activeTextures, TextureInfo *textureInfos);
void h2dLightInformationOne(LightInformation *lightInformation, int lightInformationSize);
void setMovableOne(const unsigned char *flags, int nbPrimitives);
void retagPrimitives();
void checkTextureTables();
/* solr_arena.hip: the arena the scene is resident in, its lists, what a frame is told of them */
void maybeBuildOrderFreeLists();
void flushGeometry();
void pullGeometry();
void ensureHostFreeLists();
void buildLeafRecords();
void tightenListsAgain();
float thinReachWanted(float viewDistance);
bool listEnclosesInArena(const NodeList &list);
ListKnobs listKnobs();
PruneDecider pruneDecider();
bool orderFreeListsUsable();
bool lampCutoffUsable();
bool shortRayListsChoice();
SceneArgs prepareScene(const SceneInfo &sceneInfo, bool exactNodes);
bool deepNodeList(const SceneArgs &S);
/* solr_rotation.hip: rotation and refit on the device */
/* (who: the entry point that asks - a rotation, a translation, an edit and a morph all move primitives - for the error and
 * debug texts) */
bool canRefitOne(float viewDistance, const char *who);
bool canRotateOne(const float center[3], const float cosAngles[3], const float sinAngles[3], float viewDistance);
int rotatePrimitivesOne(const float center[3], const float cosAngles[3], const float sinAngles[3], float viewDistance);
bool refitMovedScene(float viewDistance);
void refreshExactList();
/* solr_morph.hip: key-frame morphing on the device */
/* (slots: MorphSlot; who: the entry point that asks) */
int setMorphKeysOne(const Primitive *first, const Primitive *last, int nbPrimitives);
int setMorphTrackKeyOne(int slot, const Primitive *key, const int *rankOf, int nbPrimitives);
bool canMorphOne(int slotA, int slotB, float weight, float viewDistance, const char *who);
int morphKeysOne(int slotA, int slotB, float weight, float viewDistance, const char *who);
/* solr_moves.hip: translation and lamp moves on the device */
bool canTranslateOne(const float translation[3], float viewDistance);
int translatePrimitivesOne(const float translation[3], float viewDistance);
bool canMoveLampOne(int lamp, const float center[3]);
int moveLampOne(int lamp, const float center[3]);
/* solr_edits.hip: a batch of primitives set anew on the device */
bool canSetPrimitivesOne(const SolrPrimitiveEdit *edits, const int *slots, int n, float viewDistance);
int setPrimitivesOne(const SolrPrimitiveEdit *edits, const int *slots, int n, float viewDistance);
/* solr_materials.hip: a batch of primitives' materials set on the device */
bool canSetPrimitiveMaterialsOne(const int *slots, const int *materialIds, int n);
int setPrimitiveMaterialsOne(const int *slots, const int *materialIds, int n);
/* ... and an edited table of materials followed in the table and on the resident scene */
bool canEditMaterialsOne(const Material *materials, int nbActiveMaterials);
int editMaterialsOne(const Material *materials, int nbActiveMaterials);
/* ---- what every request on the resident scene shares.  A ...One runs: its can...One, beginRequest, its own work - the
 * batch, the launch, refitMovedScene where primitives moved, the host images' follow-up - and finishRequest. */
/* SOLR_HIP_DEBUG_TREE=1: why an entry point declined a request, on stderr */
__attribute__((format(printf, 2, 3))) inline void noteRefusal(const char *who, const char *why, ...)
{
    if (!getenv("SOLR_HIP_DEBUG_TREE"))
        return;
    char text[256];
    va_list args;
    va_start(args, why);
    vsnprintf(text, sizeof text, why, args);
    va_end(args);
    fprintf(stderr, "%s refused: %s\n", who, text);
}
/* the engine's device current, the arena up to date with the host images, no frame in flight that reads what is about to
 * change.  False: an error is pending, nothing was changed.  (The pointer cannot be null behind a flush that left no
 * error, whatever the scene: Arena::geometryDirty is true from the record's birth and false only after arenaFlushed,
 * which follows a reserve of at least 16 bytes that succeeded, and only Scene::release - back to a new record, dirty -
 * gives the arena back.  It is asked all the same: the launches below write through it.) */
inline bool beginRequest()
{
    HIPCHECK(hipSetDevice(g.device));
    flushGeometry();
    if (!ok() || !g.scene.arena.geometry.ptr)
        return false;
    quiesce();
    return true;
}
/* the scene's transition, the engine's count, and the status a ...One returns: 1 served, 0 an error is pending */
inline int finishRequest(RequestKind kind, bool walkHolds = false)
{
    g.scene.requestServed(kind, walkHolds, ok());
    if (!ok())
        return 0;
    ++g.served[kind];
    return 1;
}
/* solr_bank.hip: resident scenes set aside and put back */
void dropParkedOne(int key); /* (-1: all of them; waits for the frames in flight first, the only call of the bank that frees) */
/* solr_launch.hip: a frame - buffers, the launch, post-processing, read-back */
void allocateFrame();
int neededFeatures(const SceneInfo &sceneInfo, bool full);
void renderImpl(const SceneInfo &sceneInfo, const vec4i &objects, const PostProcessingInfo &ppInfo, const float origin[3],
                const float direction[3], const float angles[4], bool counting, unsigned long long counts[8]);
void collectEvents();
void d2hBitmapOne(const SceneInfo &sceneInfo, BitmapBuffer *bitmap, PrimitiveXYIdBuffer *primitivesXYIds, bool wait);
void d2hBitmapWait();
/* solr_image_ring.hip: the ring of page-locked host images behind solr_hip_d2h_image_async */
void releaseCopies(); /* the current engine's copy lane, and what its flights know of copies (engine 0: before gImageRing.release()) */
bool imageStreamingCuts(int tileRows, int firstRow[SOLR_STREAM_BANDS_MAX + 1], int *bands, bool withIds);
bool armImageStreaming(FrameArgs &F, int tileRows, hipStream_t stream, bool withIds);
void markStreamedFrame(hipStream_t stream);
void ensureCopyStream();
bool ensureImageRing();
int nextTicket(int *slot);
/* solr_rccl.hip */
bool haveCommunicator();
bool communicatorUp(); /* a communicator of any size exists (initialize_scene refuses several in-process devices then) */
int agreedHaloRows(const PostProcessingInfo &ppInfo);
void exchangeDepthHalo(int flight, hipStream_t stream, const PixelRecord *pp, int W, int firstRow, int nbRows, int frameRows,
                       int wanted, DepthHalo *halo);
bool shareRandoms(); /* every rank takes rank 0's seed for the random sequence (solr_hip_comm_shared_seed) */

/* A frame with the ambient-occlusion post-process on a rank of a communicator owes its neighbours the boundary rows
 * of its strip, whatever becomes of the frame on this rank: when renderImpl leaves before it got there (an argument
 * check, an error state, a strip it holds no row of), the exchange is posted with zeros on the way out. */
struct HaloDebt
{
    bool owed = false;
    int wanted = 0, width = 0, frameRows = 0;
    ~HaloDebt()
    {
        if (owed)
            exchangeDepthHalo(g.current, g.flight[g.current].stream, nullptr, width, 0, 0, frameRows, wanted, nullptr);
    }
};
/* solr_launch.hip: the neighbourhood post-processing of a frame (also what the test-only solr_hip_probe_postprocess runs) */
void launchPostProcess(const SceneInfo &sceneInfo, const PostProcessingInfo &ppInfo, int flight, hipStream_t stream, int firstRow,
                       int nbRows, unsigned char *bitmap, HaloDebt &debt);
} // namespace solreng

/* solr_morph.hip: k_packMorphKeys behind a plain launcher, as setMorphTrackKeyOne calls it (also what the test-only
 * solr_hip_probe_pack_morph_key runs) */
namespace solrmorph
{
void packMorphKeys(hipStream_t stream, const Primitive *key, const int *rankOf, int nbPrimitives, float4 *planes);
} // namespace solrmorph

/* solr_post.hip: the post-processing kernels of cudaRender (CRT:1057-1358) and the tile sort, behind plain launchers */
namespace solrpost
{
void defaultConversion(hipStream_t stream, const SceneInfo &si, int nbPixels, const PixelRecord *pp, unsigned char *bitmap);
void ambientOcclusion(hipStream_t stream, const SceneInfo &si, const PostProcessingInfo &ppi, int nbRows, const PixelRecord *pp,
                      const float *randoms, long nbRandoms, unsigned char *bitmap, const DepthHalo &halo, int firstRow,
                      float randomsReach, bool heavyFirst);
void depthOfField(hipStream_t stream, const SceneInfo &si, const PostProcessingInfo &ppi, int nbRows, const PixelRecord *pp,
                  const float *randoms, long nbRandoms, unsigned char *bitmap);
void radiosity(hipStream_t stream, const SceneInfo &si, const PostProcessingInfo &ppi, int nbRows, const PixelRecord *pp,
               const int4 *ids, const float *randoms, long nbRandoms, unsigned char *bitmap);
void filter(hipStream_t stream, const SceneInfo &si, const PostProcessingInfo &ppi, int nbRows, const PixelRecord *pp,
            unsigned char *bitmap);
void cartoon(hipStream_t stream, const SceneInfo &si, const PostProcessingInfo &ppi, int nbRows, const PixelRecord *pp,
             unsigned char *bitmap);
void orderTiles(hipStream_t stream, const unsigned *cost, unsigned *snapshot, unsigned *order, int nbTiles,
                volatile unsigned *hostStats, int flights, const BandCuts &cuts);
void packDepthRows(hipStream_t stream, const PixelRecord *pp, int W, int row0, int n, float *out);
} // namespace solrpost

#endif
