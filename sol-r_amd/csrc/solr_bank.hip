/*
 * solr_bank.hip - the scene bank of the MI355X rendering engine: resident scenes set aside under a key and put back
 * (include/solr_hip.h: solr_hip_park_scene, solr_hip_resume_scene ...).  The reference's AnimationScene holds one mesh per
 * frame and shows them with setFrame + compactBoxes(false) (AnimationScene.cpp:55-109): every displayed frame flattens the
 * scene, builds its walk-order list and uploads the arena again, and the order-free lists, thin copies and sorted copies are
 * thrown away before they are ever made.  With the bank a frame the engine has been given once stays on the device -
 * engine.h ParkedScene: Scene + Lights + SceneFacts, moved - and a switch back to it is a swap of records on the host:
 * no kernel, no copy, no allocation, no wait.  Only dropping a parked scene frees memory, and waits for the frames in
 * flight first.
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
/* the resident scene: something h2d_scene has left (its arena may still be waiting for the first frame's flushGeometry) */
static bool sceneResident()
{
    return g.initialized && !g.scene.hostPrims.empty() && g.scene.exact.nb + g.scene.nbPrimitives > 0;
}

/* the resident scene's buffers given back as finalize_scene gives them back */
static void dropResident()
{
    quiesce();
    g.scene.release();
    g.lights = Lights();
    g.facts = SceneFacts();
}

void dropParkedOne(int key)
{
    bool waited = false;
    for (size_t i = 0; i < g.bank.parked.size();)
    {
        if (key >= 0 && g.bank.parked[i].key != key)
        {
            ++i;
            continue;
        }
        if (!waited)
        {
            (void)hipSetDevice(g.device);
            quiesce(); /* a frame in flight may still read the arena that goes */
        }
        waited = true;
        g.bank.parked[i].scene.release();
        g.bank.parked.erase(g.bank.parked.begin() + (long)i);
    }
}

/* would this engine park the resident scene under `key`?  (asked of every in-process device before any of them parks) */
static bool canParkOne(int key)
{
    if (key < 0 || !ok() || !sceneResident())
        return false;
    const int held = g.bank.find(key);
    const unsigned long long others = g.bank.bytes() - (held >= 0 ? g.bank.parked[held].bytes : 0);
    return others + g.scene.deviceBytes() <= g.bank.limitBytes;
}

static void parkOne(int key)
{
    dropParkedOne(key);
    g.bank.parked.emplace_back();
    g.bank.parked.back().park(key, g.scene, g.lights, g.facts, g.materials.generation);
}

static void resumeOne(int key)
{
    const int at = g.bank.find(key);
    if (at < 0)
        return;
    if (g.scene.deviceBytes() > 0 || !g.scene.hostPrims.empty())
        dropResident(); /* as h2d_scene would drop it; a host that wants to keep it parks it first */
    ParkedScene &record = g.bank.parked[at];
    const long generation = record.materialsGeneration;
    record.resume(g.scene, g.lights, g.facts);
    g.bank.parked.erase(g.bank.parked.begin() + at);
    ++g.bank.nbSwitches;
    /* h2d_materials since it was parked: the tags, the colour keys and the facts are those of another table.  Pulled,
     * retagged and laid out again as h2d_materials does it for the resident scene - slower than a plain resume, still no
     * flatten and no list build */
    if (generation != g.materials.generation)
    {
        (void)hipSetDevice(g.device);
        retagPrimitives();
    }
}
} // namespace solreng

extern "C" {

int solr_hip_park_scene(int key)
{
    bool all = true;
    onEveryDevice([&](int) { all = canParkOne(key) && all; });
    if (!all)
        return 0;
    /* every engine said it would, and parking moves records - it allocates nothing and asks the device nothing: none can
     * decline any more, so "all or none" is decided above and there is nothing to undo */
    onEveryDevice([&](int) { parkOne(key); });
    return 1;
}

int solr_hip_resume_scene(int key)
{
    bool all = key >= 0;
    onEveryDevice([&](int) { all = all && g.initialized && ok() && g.bank.find(key) >= 0; });
    if (!all)
        return 0;
    onEveryDevice([&](int) { resumeOne(key); });
    return solr_hip_last_error(nullptr, 0) == 0 ? 1 : 0;
}

void solr_hip_drop_parked_scenes(int key)
{
    onEveryDevice([&](int) { dropParkedOne(key < 0 ? -1 : key); });
}

void solr_hip_set_scene_bank_bytes(unsigned long long bytes)
{
    /* (a knob: it outlives finalize_scene, and engines of further devices take engine 0's) */
    for (Engine *e : gEngines)
        if (e)
            e->bank.limitBytes = bytes;
}

int solr_hip_parked_scenes(void)
{
    return (int)g.bank.parked.size();
}

unsigned long long solr_hip_parked_bytes(void)
{
    return g.bank.bytes();
}

int solr_hip_scene_switches(void)
{
    return g.bank.nbSwitches;
}

int solr_hip_scene_uploads(void)
{
    return g.bank.nbUploads;
}
}
