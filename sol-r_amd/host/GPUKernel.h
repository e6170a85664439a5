/*
 * GPUKernel.h - host-side scene store and box-tree builder in front of the
 * rendering engine.
 *
 * Mirrors the public interface of the reference's solr::GPUKernel
 * (reference: solr/engines/GPUKernel.h:79-444) for everything that feeds the
 * per-pixel rendering path: primitives, materials, textures, camera, scene
 * and post-processing settings, the box-grid build (compactBoxes) and the
 * render_begin / render_end / getBitmap frame protocol.  Method names,
 * argument order and the dirty-flag protocol (GPUKernel.h:371-374,387) are the
 * reference's, so code written against the reference class reads the same
 * here.  Out of scope (and absent): fake-GL vertex assembly, Kinect/Oculus
 * hooks.
 *
 * The flattened arrays this class produces (BoundingBox[], Primitive[],
 * Lamp[], LightInformation[], Material[]) are bit-for-bit what the reference
 * builder would hand to its device layer for the same calls: same grid hash,
 * same std::map key order, same depth-first flattening with subtree sizes as
 * skip pointers (reference: GPUKernel.cpp:741-1281).  Storage differs (vectors
 * sized to the scene instead of NB_MAX_* arrays).
 */
#pragma once

#include <algorithm>
#include <map>
#include <numeric>
#include <unordered_map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/solr_hip.h"
#include "../../include/solr_types.h"

namespace solr
{
/* The number of atoms from which the HIP engine searches for a molecule's sticks on the device (GPUKernel::
 * setStickDeviceFrom).  A call of solr_hip_stick_pairs has a fixed cost - a stream, two allocations, four copies, two
 * kernels, a scan, three waits - measured on an MI355X at 4.6 - 5.6 ms from 486 to 5 000 atoms alike, while the loops
 * over csrc/stick_pairs.h on that machine's CPU grow with the square of the atoms: 2.7 ms at 2 500 atoms against the
 * device's 5.0, 5.5 ms at 3 000 against 5.0 (tools/molecule_load_time.py with each route forced;
 * profiles/r27/molecule_sticks.txt) */
const int DEFAULT_STICK_DEVICE_FROM = 2500;

/* reference: GPUKernel.h:46-65 */
struct CPUPrimitive
{
    bool belongsToModel;
    bool movable;
    vec3f p0, p1, p2;
    vec3f n0, n1, n2;
    vec3f size;
    int type;
    int materialId;
    vec2f vt0, vt1, vt2;
    vec3f speed0, speed1, speed2;
};

/* reference: GPUKernel.h:67-73 */
struct CPUBoundingBox
{
    vec3f parameters[2];
    vec3f center;
    std::vector<long> primitives; /* primitive ids (level 0) or child box keys (level > 0) */
    /* level > 0: where each child box sits in the level below (OrderedMap::at), filled next to `primitives`
     * by processOutterBoxes so that the refit and the flattening need not hash 500 k keys per pass.  Only
     * trusted while it has one entry per key: the light cell also lists light ids (GPUKernel.cpp:1189-1215)
     * and goes the hashed way. */
    std::vector<unsigned int> childAt;
    long indexForNextBox;
};

/* Ordered associative container with the slice of std::map's interface the builder uses (find,
 * operator[], insert, ascending iteration, size, clear) and the same observable behaviour, built for
 * the builder's access pattern: hundreds of thousands of inserts and look-ups per level, then ONE
 * ordered sweep.  Values live in a vector in insertion order, look-ups go through a hash index, and
 * the ascending key order is produced by one sort when iteration starts (and kept until the next
 * insertion).  The reference uses std::map<unsigned, CPUBoundingBox> per level
 * (GPUKernel.h:52-53 there); on 100k primitives the red-black trees made compactBoxes(true) 1.3 s. */
/* key -> position, open addressing with linear probing (the node-based std::unordered_map spent most of a
 * rebuild allocating: nine levels, 900 k insertions for 100 k primitives) */
class FlatIndex
{
public:
    static constexpr unsigned int NONE = 0xffffffffu;
    void clear()
    {
        m_keys.clear();
        m_positions.clear();
        m_count = 0;
        m_shift = 32;
    }
    void reserve(size_t n)
    {
        size_t wanted = 16;
        while (wanted < 2 * n)
            wanted *= 2;
        if (wanted > m_positions.size())
            rehash(wanted);
    }
    unsigned int find(unsigned int key) const
    {
        if (m_positions.empty())
            return NONE;
        const size_t mask = m_positions.size() - 1;
        for (size_t slot = home(key);; slot = (slot + 1) & mask)
        {
            if (m_positions[slot] == NONE)
                return NONE;
            if (m_keys[slot] == key)
                return m_positions[slot];
        }
    }
    /* the key must not be present */
    void insert(unsigned int key, unsigned int position)
    {
        if (2 * (m_count + 1) > m_positions.size())
            rehash(m_positions.empty() ? 16 : 2 * m_positions.size());
        place(key, position);
        ++m_count;
    }

private:
    size_t home(unsigned int key) const { return (size_t)((key * 0x9E3779B1u) >> m_shift); }
    void place(unsigned int key, unsigned int position)
    {
        const size_t mask = m_positions.size() - 1;
        size_t slot = home(key);
        while (m_positions[slot] != NONE)
            slot = (slot + 1) & mask;
        m_keys[slot] = key;
        m_positions[slot] = position;
    }
    void rehash(size_t capacity)
    {
        std::vector<unsigned int> keys, positions;
        keys.swap(m_keys);
        positions.swap(m_positions);
        m_keys.assign(capacity, 0u);
        m_positions.assign(capacity, NONE);
        m_shift = 32;
        for (size_t c = capacity; c > 1; c /= 2)
            --m_shift;
        for (size_t i = 0; i < positions.size(); ++i)
            if (positions[i] != NONE)
                place(keys[i], positions[i]);
    }
    std::vector<unsigned int> m_keys, m_positions;
    size_t m_count = 0;
    unsigned int m_shift = 32;
};

template <typename V>
class OrderedMap
{
public:
    typedef std::pair<unsigned int, V> value_type;
    class iterator
    {
    public:
        iterator() : m_owner(nullptr), m_rank(0) {}
        iterator(OrderedMap *owner, size_t rank) : m_owner(owner), m_rank(rank) {}
        value_type &operator*() const { return m_owner->m_items[m_owner->m_order[m_rank]]; }
        value_type *operator->() const { return &m_owner->m_items[m_owner->m_order[m_rank]]; }
        /* where the element lives: stable until clear(), see OrderedMap::at */
        unsigned int position() const { return m_owner->m_order[m_rank]; }
        iterator &operator++()
        {
            ++m_rank;
            return *this;
        }
        bool operator==(const iterator &o) const { return m_rank == o.m_rank; }
        bool operator!=(const iterator &o) const { return m_rank != o.m_rank; }

    private:
        OrderedMap *m_owner;
        size_t m_rank;
    };
    typedef iterator const_iterator;

    size_t size() const { return m_items.size(); }
    bool empty() const { return m_items.empty(); }
    void clear()
    {
        m_items.clear();
        m_order.clear();
        m_index.clear();
        m_sorted = true;
    }
    iterator begin() const
    {
        sortOrder();
        return iterator(const_cast<OrderedMap *>(this), 0);
    }
    iterator end() const { return iterator(const_cast<OrderedMap *>(this), m_items.size()); }
    /* like std::map::find, but the iterator is only good for comparison with end() and dereference */
    iterator find(unsigned int key) const
    {
        if (m_index.find(key) == FlatIndex::NONE)
            return end();
        sortOrder();
        /* rank of the key in ascending order */
        size_t lo = 0, hi = m_order.size();
        while (lo < hi)
        {
            const size_t mid = (lo + hi) / 2;
            if (m_items[m_order[mid]].first < key)
                lo = mid + 1;
            else
                hi = mid;
        }
        return iterator(const_cast<OrderedMap *>(this), lo);
    }
    bool contains(unsigned int key) const { return m_index.find(key) != FlatIndex::NONE; }
    /* the element at a position an iterator reported: no hashing (positions survive insertions) */
    V &at(unsigned int position) { return m_items[position].second; }
    /* ... provided it still is the element with that key (a level may have been cleared and refilled since) */
    V *atIfKey(unsigned int position, unsigned int key)
    {
        return (position < m_items.size() && m_items[position].first == key) ? &m_items[position].second : nullptr;
    }
    V *lookup(unsigned int key)
    {
        if (key < m_items.size() && m_items[key].first == key) /* dense ids: position == key */
            return &m_items[key].second;
        const unsigned int at = m_index.find(key);
        return at == FlatIndex::NONE ? nullptr : &m_items[at].second;
    }
    V &operator[](unsigned int key)
    {
        if (key < m_items.size() && m_items[key].first == key)
            return m_items[key].second;
        const unsigned int at = m_index.find(key);
        if (at != FlatIndex::NONE)
            return m_items[at].second;
        return append(key, V());
    }
    std::pair<iterator, bool> insert(const value_type &kv)
    {
        if (m_index.find(kv.first) != FlatIndex::NONE)
            return std::make_pair(end(), false);
        append(kv.first, kv.second);
        return std::make_pair(end(), true);
    }
    void reserve(size_t n)
    {
        m_items.reserve(n);
        m_index.reserve(n);
    }

private:
    V &append(unsigned int key, const V &value)
    {
        if (m_sorted && !m_items.empty() && key < m_items[m_order.empty() ? m_items.size() - 1 : m_order.back()].first)
            m_sorted = false;
        m_index.insert(key, (unsigned int)m_items.size());
        m_items.push_back(value_type(key, value));
        if (m_sorted)
            m_order.push_back((unsigned int)m_items.size() - 1);
        return m_items.back().second;
    }
    void sortOrder() const
    {
        if (m_sorted && m_order.size() == m_items.size())
            return;
        m_order.resize(m_items.size());
        for (size_t i = 0; i < m_order.size(); ++i)
            m_order[i] = (unsigned int)i;
        std::sort(m_order.begin(), m_order.end(),
                  [this](unsigned int a, unsigned int b) { return m_items[a].first < m_items[b].first; });
        m_sorted = true;
    }
    std::vector<value_type> m_items;
    mutable std::vector<unsigned int> m_order; /* item indices by ascending key, valid when m_sorted */
    FlatIndex m_index;
    mutable bool m_sorted = true;
};

typedef OrderedMap<CPUBoundingBox> BoxContainer;
typedef OrderedMap<CPUPrimitive> PrimitiveContainer;

inline vec2i make_vec2i(int x = 0, int y = 0) { vec2i v; v.x = x; v.y = y; return v; }
inline vec4i make_vec4i(int x = 0, int y = 0, int z = 0, int w = 0) { vec4i v; v.x = x; v.y = y; v.z = z; v.w = w; return v; }
inline vec2f make_vec2f(float x = 0.f, float y = 0.f) { vec2f v; v.x = x; v.y = y; return v; }
inline vec3f make_vec3f(float x = 0.f, float y = 0.f, float z = 0.f) { vec3f v; v.x = x; v.y = y; v.z = z; return v; }
inline vec4f make_vec4f(float x = 0.f, float y = 0.f, float z = 0.f, float w = 0.f) { vec4f v; v.x = x; v.y = y; v.z = z; v.w = w; return v; }

/* What the host knows about the scene its engine keeps resident: whether the store and that scene are the same one, and by
 * what the store lags behind it.  Read everywhere, written through the transitions and the two scoped guards below only -
 * by convention, as csrc/engine.h Scene is.  A default-constructed record: nothing uploaded. */
struct ResidentScene
{
    /* a move the engine applied to the resident scene and the store has not replayed */
    struct Move
    {
        enum Kind
        {
            ROTATION,    /* v: the centre, cosA, sinA */
            TRANSLATION, /* v: the translation */
            LAMP_MOVE,   /* v: the centre of primitive `index` */
            EDIT,        /* a batch of primitives set anew: editBatches[index] */
            MATERIALS,   /* a batch of primitives' materials set: materialBatches[index] */
            NB_KINDS
        } kind;
        vec3f v, cosA, sinA;
        unsigned int index;
    };
    /* an animation that runs for hours: past this many the moves are only counted - the store then catches up from the
     * device's primitives, which it does for more than a handful of rotations anyway */
    static constexpr size_t MAX_RECORDED_MOVES = 100000;

    bool primitivesTransfered = false; /* the reference's m_primitivesTransfered: no upload of the scene is due */
    bool touched = true;               /* the scene store was accessed since the last upload */
    long frame = -1;                   /* the frame the resident scene was uploaded from, -1: none */
    unsigned long uploads = 0;         /* the serial of its upload (one counter per kernel, 0: none): what was made from the flattened order is as old as that */
    bool resumed = false;              /* put back from the frame bank, neither touched nor uploaded since (compactBoxes) */
    bool lampMoved = false;            /* a lamp was moved over there since the upload (morphFrame) */
    bool edited = false;               /* primitives were set anew over there since the upload (morphFrame) */
    /* the frames the engine holds as keys of that scene since the upload: in the slots of a track (morphBetween; the slot is
     * the frame's number), and the two of its two-key interface (morphFrame; -1: it has none) */
    std::vector<unsigned int> trackKeys;
    long pairKeys[2] = {-1, -1};
    bool buildingLevels = false; /* the lazy build of the level maps reads the store as it is: what is pending stays pending */
    /* the journal: the moves served over there since the upload - or since the morph that superseded what was before
     * it -, in order, up to the cap; the rotations among them; per kind those beyond the cap */
    std::vector<Move> journal;
    size_t journalRotations = 0;
    size_t unrecorded[Move::NB_KINDS] = {}; /* by Move::Kind */
    /* the batches of the journal's edits, as given, and how many edits the journal holds.  What the engine hands back
     * (primitivesFromDevice) carries neither sizes nor texture coordinates and leaves out what the store believes unmovable,
     * so it cannot restore an edit: a journal that holds one is always replayed, and is therefore never merely counted -
     * at the cap an edit is declined (recordsEdits), and behind an edit so is every other move (offers) */
    std::vector<std::vector<SolrPrimitiveEdit>> editBatches;
    size_t journalEdits = 0;
    /* ... and the records in them: a scene that edits a thousand triangles a frame for hours must not grow the journal
     * without bound.  Past this many (120 MB of records) the store catches up before the next batch is offered
     * (GPUKernel::setPrimitives) - a replay, which leaves the fast path open */
    static constexpr size_t MAX_JOURNALLED_EDIT_RECORDS = size_t(1) << 20;
    size_t journalEditRecords = 0;
    /* the batches of the journal's material sets, as given, and how many the journal holds.  What the engine hands back
     * carries no material either: like an edit, a material set is always replayed and never merely counted, and its
     * records count towards the same cap.  No box follows a material: such a journal alone refits nothing (refits) */
    struct MaterialSet
    {
        unsigned int index;
        int materialId;
    };
    std::vector<std::vector<MaterialSet>> materialBatches;
    size_t journalMaterialSets = 0;
    /* ... and per primitive the material the journal's sets leave it with, for whoever asks what a primitive's material is
     * now without waking the store (getPrimitiveMaterial, editSlots) */
    std::map<unsigned int, int> pendingMaterials;
    bool materialsSet = false; /* materials were set over there since the upload (morphFrame) */
    bool morphPending = false;
    unsigned int pendingMorphKeys[2] = {0, 0}; /* the two key frames of the pending morph */
    float pendingMorphWeight = 0.f;

    /* The one offer rule: a move on frame `f` of the store may be offered to the engine when the scene over there was
     * uploaded, nothing has accessed the store since, and it was uploaded from that frame (a frame switch without a
     * flatten leaves the device with another frame than the current one) */
    bool offers(unsigned int f) const
    {
        return primitivesTransfered && !touched && frame == (long)f && !(nbReplayedOnly() && journal.size() >= MAX_RECORDED_MOVES);
    }
    /* the moves of the journal that only a replay restores: edits and material sets */
    size_t nbReplayedOnly() const { return journalEdits + journalMaterialSets; }
    /* ... and a batch of edits only while the journal records: an edit is never merely counted */
    bool recordsEdits() const { return journal.size() < MAX_RECORDED_MOVES; }
    bool holdsTrackKey(unsigned int f) const { return std::find(trackKeys.begin(), trackKeys.end(), f) != trackKeys.end(); }
    bool holdsPairKeys(unsigned int a, unsigned int b) const { return pairKeys[0] == (long)a && pairKeys[1] == (long)b; }
    size_t nbUnrecorded() const { return std::accumulate(unrecorded, unrecorded + Move::NB_KINDS, (size_t)0); }
    size_t nbPendingMoves() const { return journal.size() + nbUnrecorded(); }
    size_t nbPendingRotations() const { return journalRotations + unrecorded[Move::ROTATION]; }
    bool pendingMorph() const { return morphPending; }
    bool lags() const { return nbPendingMoves() > 0 || morphPending; }
    /* the recorded rotations and translations: a pass over the primitives each to replay; a lamp move is one assignment,
     * an edit a few per primitive of its batch */
    size_t nbHeavy() const
    {
        return std::count_if(journal.begin(), journal.end(),
                             [](const Move &m) { return m.kind == Move::ROTATION || m.kind == Move::TRANSLATION; });
    }
    /* do the boxes follow what is pending?  Lamp moves alone refit nothing, as on the host route: setPrimitiveCenter +
     * compactBoxes(false) leaves every box as it is, the stale box of another primitive whose centre was set included */
    bool refits() const
    {
        return morphPending || nbHeavy() || journalEdits || unrecorded[Move::ROTATION] || unrecorded[Move::TRANSLATION];
    }

    /* the engine has uploaded the scene from frame `f` (render_begin, when an upload was due): device and host hold the same
     * scene, the engine's morph keys are gone, the lamps are where the store has them */
    void uploaded(unsigned int f, unsigned long serial)
    {
        primitivesTransfered = true;
        touched = false;
        resumed = false;
        trackKeys.clear();
        pairKeys[0] = pairKeys[1] = -1;
        frame = (long)f;
        lampMoved = false;
        edited = false;
        materialsSet = false;
        uploads = serial;
    }
    void setTransfered(bool value)
    {
        primitivesTransfered = value;
        resumed = resumed && value;
    }
    /* the scene store was accessed (GPUKernel::frame): the fast path ends until the next upload */
    void touch()
    {
        touched = true;
        resumed = false;
    }
    /* the record has come back from the frame bank with its flattened arrays, and the engine holds its scene again
     * (GPUKernel::switchFrame): both sides are what compactBoxes(false) and an upload would produce */
    void resumedFromBank() { resumed = true; }
    bool asResumed(unsigned int f) const { return resumed && primitivesTransfered && !touched && frame == (long)f; }
    void trackKeyTaken(unsigned int f) { trackKeys.push_back(f); }
    void pairKeysTaken(unsigned int a, unsigned int b) { pairKeys[0] = (long)a, pairKeys[1] = (long)b; }
    /* the engine has served `move`: into the journal, or past the cap into the counts */
    void record(const Move &move)
    {
        if (move.kind == Move::LAMP_MOVE)
            lampMoved = true;
        if (journal.size() >= MAX_RECORDED_MOVES)
        {
            ++unrecorded[move.kind];
            return;
        }
        journal.push_back(move);
        journalRotations += move.kind == Move::ROTATION;
    }
    /* the engine has set these primitives anew (offered only while recordsEdits): the batch as given, into the journal */
    void recordEdit(const SolrPrimitiveEdit *edits, int n)
    {
        edited = true;
        editBatches.emplace_back(edits, edits + n);
        journal.push_back({Move::EDIT, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, (unsigned int)editBatches.size() - 1});
        ++journalEdits;
        journalEditRecords += (size_t)n;
    }
    /* the engine has set these primitives' materials (offered only while recordsEdits): the batch as given, into the journal */
    void recordMaterials(const int *indices, const int *materialIds, int n)
    {
        materialsSet = true;
        materialBatches.emplace_back();
        for (int i = 0; i < n; ++i)
        {
            materialBatches.back().push_back({(unsigned int)indices[i], materialIds[i]});
            pendingMaterials[(unsigned int)indices[i]] = materialIds[i];
        }
        journal.push_back({Move::MATERIALS, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, (unsigned int)materialBatches.size() - 1});
        ++journalMaterialSets;
        journalEditRecords += (size_t)n;
    }
    /* the store has been set anew, here (morphFrame's host route): nothing is pending */
    void clear()
    {
        journal.clear();
        journalRotations = 0;
        std::fill(unrecorded, unrecorded + Move::NB_KINDS, (size_t)0);
        editBatches.clear();
        journalEdits = 0;
        journalEditRecords = 0;
        materialBatches.clear();
        journalMaterialSets = 0;
        pendingMaterials.clear();
        morphPending = false;
    }
    /* ... or over there, by a morph of those two key frames at that weight: it supersedes what was pending before it */
    void morphServed(unsigned int frameA, unsigned int frameB, float weight)
    {
        clear();
        morphPending = true;
        pendingMorphKeys[0] = frameA, pendingMorphKeys[1] = frameB;
        pendingMorphWeight = weight;
    }
    /* syncHost: what is pending is handed over - the record as it was, its journal moved out - and the record is caught up */
    ResidentScene take()
    {
        ResidentScene pending = std::move(*this);
        clear();
        return pending;
    }
    /* While syncHost() brings the store to what the device holds already: its helpers go through frame(), setPrimitive and
     * streamDataToGPU like any caller and flip `primitivesTransfered` and `touched`; both are put back when the scope ends */
    struct Replaying
    {
        ResidentScene &scene;
        const bool primitivesTransfered, touched, resumed;
        explicit Replaying(ResidentScene &s)
            : scene(s), primitivesTransfered(s.primitivesTransfered), touched(s.touched), resumed(s.resumed)
        {
        }
        ~Replaying() { scene.primitivesTransfered = primitivesTransfered, scene.touched = touched, scene.resumed = resumed; }
    };
    /* While buildLevelsOnHost() makes the level maps, which may nest: it reads the store as it is (buildingLevels) */
    struct BuildingLevels
    {
        ResidentScene &scene;
        const bool nested;
        explicit BuildingLevels(ResidentScene &s) : scene(s), nested(s.buildingLevels) { s.buildingLevels = true; }
        ~BuildingLevels() { scene.buildingLevels = nested; }
    };
};

class GPUKernel
{
public:
    GPUKernel();
    virtual ~GPUKernel();

    /* reference: GPUKernel.h:85-87 */
    virtual void initBuffers();
    virtual void cleanup();
    virtual void reshape();

    /* reference: GPUKernel.h:90-96,289 (engine selection hooks) */
    virtual void setPlatformId(const int) {}
    virtual void setDeviceId(const int) {}
    virtual void setKernelFilename(const std::string &) {}
    virtual void queryDevice() {}
    virtual void recompileKernels() {}
    virtual std::string getGPUDescription() { return m_gpuDescription; }

    /* ---------- Rendering (GPUKernel.h:100-102) ---------- */
    virtual void render_begin(const float timer);
    virtual void render_end() = 0;
    /* the image of the frame render_end delivered last (with frames in flight - setFramesInFlight - that is the
     * engine's page-locked copy of it, not m_bitmap: nothing is copied twice) */
    BitmapBuffer *getBitmap()
    {
        fetchBitmap();
        return m_bitmapView ? m_bitmapView : (m_bitmap.empty() ? nullptr : m_bitmap.data());
    }
    /* render_end with the frame's image delivered into the CALLER'S array instead of m_bitmap (what SolR_RunKernel is
     * for, SolRStub.cpp:154-164: the reference copies m_bitmap to the caller afterwards).  An engine with a device
     * copies from the device straight into `image` and leaves m_bitmap to the next getBitmap() (fetchBitmap); the
     * default is the reference's two steps. */
    virtual void render_end(BitmapBuffer *image);
    /* Extension (no reference equivalent; the reference's render_end waits for the frame and then copies it,
     * CudaKernel.cpp:304-312).  n > 1: render_begin also starts the read-back of its frame's image, and render_end
     * delivers the image of the frame n - 1 calls back - the one whose copy has had n - 1 frames' time to land -
     * while the newer ones render; flushFrames() waits for all of them and delivers the newest.  1 (default): the
     * reference's protocol.  Engines without a device ignore it. */
    virtual void setFramesInFlight(int n) { (void)n; }
    virtual int getFramesInFlight() const { return 1; }
    virtual void flushFrames() {}
    /* devices of this process the frame is shared out over (m_occupancyParameters.x, which the reference leaves at 1
     * with no way to set it: CudaKernel.cpp:90); engines without a device keep 1 */
    virtual void setGpuCount(int n) { (void)n; }
    virtual int getGpuCount() const { return 1; }
    /* 0 = ok, otherwise the engine's pending error (no reference equivalent:
     * the reference exits the process on a device error) */
    virtual int lastError(std::string *message = nullptr) { (void)message; return 0; }

protected:
    BitmapBuffer *m_bitmapView = nullptr; /* see getBitmap */
    bool m_jpegFrame = false;             /* render_begin is renderJpeg's: the frame's image stays whole on the device */
    bool m_jpegStreamFrame = false;       /* ... renderJpegBegin's, for a JPEG in flight: no image-ring copy either */
    /* JPEG frames in flight (renderJpegBegin / renderJpegEnd): what a ticket stands for - the engine's ticket, or, where
     * the engine declined, the file itself - four deep, as the engine's slots are.  A ticket is
     * (serial mod JPEG_TICKET_PERIOD) * JPEG_TICKETS + slot, the slot serial mod JPEG_TICKETS: one whose slot has been
     * handed out again is told from a live one by its generation */
    static const int JPEG_TICKETS = 4;
    static const long JPEG_TICKET_PERIOD = ((long)0x7fffffff / JPEG_TICKETS / JPEG_TICKETS - 1) * JPEG_TICKETS;
    struct JpegTicket
    {
        long serial = -1;      /* -1: the slot holds none */
        int engineTicket = -1; /* >= 0: the segment is collected from the engine at the first renderJpegEnd */
        SolrJpegSource source = {};
        bool optimise = false;
        std::vector<unsigned char> file; /* once it exists: renderJpegEnd hands it over as often as it is asked */
    };
    JpegTicket m_jpegTickets[JPEG_TICKETS];
    long m_jpegIssued = 0;
    std::string m_jpegTicketError; /* why the last renderJpegEnd failed, empty when it did not */

public:

    /* ---------- Primitives (GPUKernel.h:108-149) ---------- */
    int addPrimitive(PrimitiveType type, bool belongsToModel = false);
    void setPrimitive(const int &index, float x0, float y0, float z0, float w, float h, float d, int materialId);
    void setPrimitive(const int &index, float x0, float y0, float z0, float x1, float y1, float z1, float w, float h,
                      float d, int materialId);
    void setPrimitive(const int &index, float x0, float y0, float z0, float x1, float y1, float z1, float x2, float y2,
                      float z2, float w, float h, float d, int materialId);
    unsigned int getPrimitiveAt(int x, int y);
    void setPrimitiveIsMovable(const int &index, bool movable);
    void setPrimitiveBellongsToModel(const int &index, bool bellongsToModel);
    void setPrimitiveMaterial(unsigned int index, int materialId);
    int getPrimitiveMaterial(unsigned int index);
    vec4f getPrimitiveCenter(unsigned int index);
    void setPrimitiveCenter(unsigned int index, const vec3f &center);
    void setPrimitiveTextureCoordinates(const unsigned int index, const vec2f &vt0, const vec2f &vt1,
                                        const vec2f &vt2);
    void setPrimitiveNormals(unsigned int index, vec3f n0, vec3f n1, vec3f n2);
    CPUPrimitive *getPrimitive(const unsigned int index);
    /* extension: a batch of primitives of the store set anew - what a scene that animates its own vertices does per frame
     * with the three setters (the reference's WaterScene::doAnimate: 1152 triangles).  Every index is looked up first: one
     * that is not in the store refuses the batch, -1, nothing changed.  Then per record, in order: setPrimitive(index, p0,
     * p1, p2, size, materialId), with SOLR_EDIT_NORMALS setPrimitiveNormals, with SOLR_EDIT_TEXTURE_COORDINATES
     * setPrimitiveTextureCoordinates; then the box updates a rotation or a translation runs (refitBoxes).  The caller
     * flattens with compactBoxes(false), as after translatePrimitives.  An engine that keeps the scene resident may set the
     * primitives there (deviceSetPrimitives); the host copy then lags behind by that batch, in the journal with the other
     * moves, and syncHost() catches it up.  Returns 0 when done; n == 0 is done and records nothing */
    int setPrimitives(const SolrPrimitiveEdit *edits, int n);
    /* extension: a batch of primitives given another material - what a scene that marks or recolours some of its primitives
     * does per frame with setPrimitiveMaterial (the reference's SwcScene::doAnimate: the sample before gets its material back,
     * the next one the light material).  Every index is looked up first: one that is not in the store refuses the batch,
     * -1, nothing changed.  Then per record, in order, setPrimitiveMaterial(index, materialId): of several records for one
     * index the last one wins.  No box follows a material.  The caller flattens with compactBoxes(false), as after
     * setPrimitives.  An engine that keeps the scene resident may set the materials there (deviceSetPrimitiveMaterials); the
     * host copy then lags behind by that batch, in the journal with the other moves, and syncHost() catches it up;
     * getPrimitiveMaterial answers what is pending.  Returns 0 when done; n == 0 is done and records nothing */
    int setPrimitiveMaterials(const int *indices, const int *materialIds, int n);
    /* extension: the iso-surface of a field of metaballs appended as triangles - what the reference's MetaballsScene makes
     * per frame with two host loops and the fake-GL entry points (apps/scenes/animation/MetaballsScene.cpp:247-400).
     * balls: nbBalls records of x, y, z, squared radius.  The triangles come from the engine (the isoSurface hook) and are
     * appended as the reference's GL_TRIANGLES branch appends them (GPUKernel.cpp:2538-2563): addPrimitive(ptTriangle),
     * setPrimitive, setPrimitiveTextureCoordinates, setPrimitiveNormals.  The number of triangles added; -1 when an
     * argument is out of range (include/solr_hip.h) or the engine failed - nothing is added then */
    int addMetaballs(const SolrIsoGrid &grid, const float *balls, int nbBalls, int materialId);
    /* the engine's two halves alone (the isoField / isoTriangles hooks), for the tests */
    bool isoFieldOf(const SolrIsoGrid &grid, const float *balls, int nbBalls, float *field)
    {
        return isoField(grid, balls, nbBalls, field);
    }
    int isoTrianglesOf(const SolrIsoGrid &grid, const float *field, SolrIsoTriangle *triangles, int capacity)
    {
        return isoTriangles(grid, field, triangles, capacity);
    }
    /* extension: which atoms of a molecule are joined by a stick (csrc/stick_pairs.h, include/solr_hip.h) - what the PDB
     * reader asks between reading a file and adding its primitives.  atoms: n records of x, y, z, spare, an atom's rank its
     * place there; backbone: n flags.  The pairs come from the engine (the stickPairs hook) as a list: start has n + 1
     * entries, atom i's partners are partners[start[i] ... start[i + 1] - 1], ranks ascending.  false when an argument is
     * out of range - nothing is written then */
    bool stickPairsOf(const float *atoms, const unsigned char *backbone, int n, float reachPlain, float reachBackbone,
                      std::vector<long long> &start, std::vector<int> &partners)
    {
        return stickPairs(atoms, backbone, n, reachPlain, reachBackbone, start, partners);
    }
    /* searches served since the library was loaded: out[0] by a device, out[1] by the loops on the CPU */
    static void stickSearches(long long out[2]);
    /* the rank count from which an engine with a device searches there (below it the loops are quicker than a call's fixed
     * cost; DEFAULT_STICK_DEVICE_FROM).  0: always on the device.  Returns the value before.  Process-wide */
    static int setStickDeviceFrom(int n);
    static int stickDeviceFrom();
    int getLight(int index);

    /* rotation of the whole scene about a centre (GPUKernel.h:122-125) */
    void rotatePrimitives(const vec3f &rotationCenter, const vec4f &angles);
    void translatePrimitives(const vec3f &translation);
    void scalePrimitives(float scale, unsigned int from, unsigned int to);

    /* ---------- Complex objects (GPUKernel.h:162-164) ---------- */
    int addCube(float x, float y, float z, float radius, int materialId);
    int addRectangle(float x, float y, float z, float w, float h, float d, int materialId);

    /* ---------- Materials (GPUKernel.h:168-190) ---------- */
    int addMaterial();
    void setMaterial(unsigned int index, const Material &material);
    void setMaterial(unsigned int index, float r, float g, float b, float noise, float reflection, float refraction,
                     bool procedural, bool wireframe, int wireframeWidth, float transparency, float opacity,
                     int diffuseTextureId, int normalTextureId, int bumpTextureId, int specularTextureId,
                     int reflectionTextureId, int transparentTextureId, int ambientOcclusionTextureId, float specValue,
                     float specPower, float specCoef, float innerIllumination, float illuminationDiffusion,
                     float illuminationPropagation, bool fastTransparency);
    void setMaterialColor(unsigned int index, float r, float g, float b);
    Material *getMaterial(const int index);

    /* ---------- Camera (GPUKernel.h:194) ---------- */
    void setCamera(const vec3f &eye, const vec3f &dir, const vec4f &angles);

    /* ---------- Textures (GPUKernel.h:198-205) ---------- */
    void setTexture(const int index, const TextureInfo &textureInfo);
    void getTexture(const int index, TextureInfo &textureInfo);
    void setTexturesTransfered(const bool transfered) { m_texturesTransfered = transfered; }
    void realignTexturesAndMaterials();
    void processTextureOffsets();
    TextureInfo &getTextureInformation(const int index);
    /* reference: GPUKernel.h:204, GPUKernel.cpp:2110-2161.  A .bmp, .jpg or .tga file (chosen by that substring of the
     * name) into slot `index`; the texture's type from the b. / n. / a. / r. / s. / t. substrings of the name, the
     * last match winning.  An empty name or a file that does not load gives false, one line on stderr, and leaves
     * the slot and the counters as they were (host/ImageLoader.h has the readers) */
    bool loadTextureFromFile(const int index, const std::string &filename);
    std::string getTextureFilename(const int index);

    /* ---------- Screenshots (GPUKernel.h:262 of the reference, GPUKernel.cpp:2792-2852) ---------- */
    /* `quality` passes of path tracing (pathTracingIteration 0 ... quality - 1 of maxPathTracingIterations = quality)
     * at width x height, clamped to MAX_BITMAP_WIDTH x MAX_BITMAP_HEIGHT, then the last image as a JPEG file with the
     * reference encoder's default parameters (quality 85, 2x2 chroma).  The reference writes the file after every pass;
     * here it is written once, after the last.  The picture is read as the reference reads it: pixel p from pixel
     * N - p of the frame (N = width * height; for p = 0 the reference reads one pixel past the frame, here that index is
     * N - 1), red and blue swapped unless the frame buffer is ftRGB.  Frames in flight are flushed first, the buffers
     * re-shaped for the screenshot and back, the scene info restored.  Nothing is written when a pass fails.  Until the
     * next frame is rendered getBitmap() is the frame that was encoded (width * height * 3 bytes of the screenshot's size). */
    void generateScreenshot(const std::string &filename, const unsigned int width, const unsigned int height,
                            const unsigned int quality);
    /* extension: the encoder alone, on the caller's width * height * 3 bytes; false when an argument is out of range
     * (nothing is written), the engine failed or the file could not be written */
    /* the engine's pixel stage alone (the jpegCoefficients hook), for the tests */
    bool jpegCoefficientsOf(const SolrJpegSource &source, const unsigned char *rgb, std::vector<short> &coefficients)
    {
        return jpegCoefficients(source, rgb, coefficients);
    }
    /* optimise (here and below): the file of the reference encoder's two-pass mode - four Huffman tables built for the
     * picture's own symbols, written in its DHT segments - in place of the standard tables; the same pixels decode from it */
    bool encodeJpeg(const std::string &filename, const unsigned char *pixels, int width, int height, int jpegQuality,
                    int lumaH, int lumaV, bool turned, bool swapRedBlue, bool optimise = false);
    /* the same file in memory: the header, the engine's entropy-coded segment (the jpegScanOf hook), EOI */
    bool encodeJpeg(std::vector<unsigned char> &file, const unsigned char *pixels, int width, int height, int jpegQuality,
                    int lumaH, int lumaV, bool turned, bool swapRedBlue, bool optimise = false);
    /* the file of coefficient blocks somebody else made, through the engine's entropy stage alone (the jpegScan hook);
     * for the tests, next to JpegWriter::encode */
    bool jpegFileFromCoefficients(std::vector<unsigned char> &file, const short *coefficients, long nbBlocks, int width,
                                  int height, int jpegQuality, int lumaH, int lumaV, bool optimise = false);
    /* extension for whoever streams frames: one frame as SolR_RunKernel renders it (render_begin with `timer`), returned
     * as a JPEG file in memory - the file a one-pass screenshot of the same size and settings would be: JPEG quality
     * 1 ... 100, luma sampling 1x1, 2x1 or 2x2, the frame turned, red and blue swapped unless the frame buffer is ftRGB.
     * Frames in flight are flushed first.  An engine with a device codes the frame there (jpegScanOfFrame) and copies only
     * the file's bytes; getBitmap() is then NOT refreshed - it stays what it was before the call.  Where the engine
     * declines (no device, frames in flight, strips, several devices) the frame comes back through render_end and is
     * encoded from the host's bitmap: the same bytes.  false: an argument out of range or a failed frame */
    bool renderJpeg(const float timer, int jpegQuality, int lumaH, int lumaV, std::vector<unsigned char> &file,
                    bool optimise = false);
    /* JPEG frames in flight.  renderJpegBegin: renderJpeg up to the launch - the frame is rendered (render_begin with
     * `timer`) on the next flight, as render_begin takes it with setFramesInFlight(n), and submitted to the engine for
     * delivery as a JPEG (jpegBeginOfFrame); frames in flight are NOT flushed, the image stays whole on the device, no band
     * leaves and no image-ring copy is made; ids on the device, getBitmap() not refreshed, as renderJpeg leaves them.
     * Returns a ticket >= 0, or -1 (an argument out of range, a failed frame).  renderJpegEnd: that frame's file - the
     * header (with the collected tables in optimised mode) around the collected segment, EOI; waits for that frame alone.
     * A ticket may be collected any number of times until three more have been handed out; a stale or never-issued one
     * gives false with jpegTicketError() set, never another frame's file.  Where the engine declines (no device, strips,
     * several devices) renderJpegBegin renders and encodes at once by renderJpeg's road and parks the file under a ticket
     * of the same rule: interface and protocol are those of both engines.  flushFrames, render_begin / render_end and
     * renderJpeg may be mixed with outstanding tickets: a ticket's bytes are those of its own frame */
    int renderJpegBegin(const float timer, int jpegQuality, int lumaH, int lumaV, bool optimise = false);
    bool renderJpegEnd(int ticket, std::vector<unsigned char> *&file);
    const std::string &jpegTicketError() const { return m_jpegTicketError; }
    /* for the tests of the ticket rule where no frame can be rendered: the caller's pixels, read as a frame is read
     * (turned; red and blue swapped when asked), encoded at once and parked under a ticket as a declined renderJpegBegin
     * parks its file.  -1: an argument out of range */
    int jpegParkPixels(const unsigned char *pixels, int width, int height, int jpegQuality, int lumaH, int lumaV,
                       bool swapRedBlue, bool optimise);

    /* ---------- Scene (GPUKernel.h:208-221) ---------- */
    void setSceneInfo(int width, int height, float transparentColor, int graphicsLevel, float viewDistance,
                      float shadowIntensity, int nbRayIterations, vec4f backgroundColor, int cameraType,
                      float eyeSeparation, bool renderBoxes, int pathTracingIteration, int maxPathTracingIterations,
                      FrameBufferType frameBufferType, int timestamp, int atmosphericEffect, int skyboxSize,
                      int skyboxMaterialId);
    void setSceneInfo(const SceneInfo &sceneInfo);
    SceneInfo &getSceneInfo();
    void setPostProcessingInfo(PostProcessingType type, float param1, float param2, int param3);
    void setPostProcessingInfo(const PostProcessingInfo &postProcessingInfo);
    PostProcessingInfo &getPostProcessingInfo() { return m_postProcessingInfo; }

    /* ---------- Counters / frames (GPUKernel.h:267-298) ---------- */
    unsigned int getNbActiveBoxes();
    unsigned int getNbActivePrimitives();
    unsigned int getNbActiveLamps();
    unsigned int getNbActiveMaterials();
    unsigned int getNbActiveTextures();
    void resetFrame();
    void resetAll();
    void setNbFrames(const int nbFrames);
    void setFrame(const int frame)
    {
        if ((unsigned int)frame != m_frame)
            switchFrame((unsigned int)frame);
    }
    /* extension: the frame bank.  The reference's AnimationScene holds one mesh per frame and shows them with setFrame +
     * compactBoxes(false) once per displayed frame (AnimationScene.cpp:55-109): a flatten and a full upload each.  With a
     * bank of `bytes` > 0 a frame switch sets the frame that is left aside instead - its resident scene on the engine
     * (deviceParkScene), its flattened arrays and its ResidentScene here, provided the engine holds that frame untouched -
     * and puts the frame that is entered back (deviceResumeScene): compactBoxes(false) then returns at once and render_begin
     * uploads nothing.  0, the default: off - setFrame, nextFrame and previousFrame do what they always did.  Engines
     * without a device keep nothing */
    void setFrameBank(unsigned long long bytes);
    unsigned long long getFrameBank() const { return m_frameBankBytes; }
    size_t nbParkedFrames() const { return m_parked.size(); }
    /* frame switches served from the bank / scene uploads (ResidentScene::uploaded) since this kernel was made */
    unsigned long nbFrameSwitches() const { return m_nbFrameSwitches; }
    unsigned long nbSceneUploads() const { return m_nbSceneUploads; }
    /* extension: material edits on the resident scene.  A host that sets a material (setMaterial, setMaterialColor,
     * setMaterialTextureId) has the table uploaded with the next frame, which has the engine retag every primitive and lay
     * out and upload the whole scene again.  With the switch on, the engine is first asked to follow the edit in place
     * (deviceEditMaterials: the changed records, the tags and colour keys of the primitives that have them), and the table is
     * uploaded as ever when it declines.  Off, the default: the upload as ever.  materialEdits: edits the engine followed
     * since this kernel was made */
    void setMaterialEdits(bool on) { m_materialEdits = on; }
    unsigned long materialEdits() const { return m_nbMaterialEdits; }
    int getNbFrames() { return m_nbFrames; }
    int getFrame() { return m_frame; }
    /* key-frame animation (GPUKernel.h:275-298 of the reference) */
    void nextFrame();
    void previousFrame();
    void morphPrimitives();
    /* The current frame - one strictly between the first and the last key frame, with as many primitives as each of
     * them, pairwise of the same type by rank in id order - blended anew at any finite weight: every primitive set in
     * place by morphPrimitives' statements with r = weight (first + r * (last - first), setPrimitive,
     * setPrimitiveNormals, the first key's texture coordinates, material and movable flag), the boxes refitted in the
     * shape they have, compactBoxes(false).  An engine that keeps the scene resident may blend it there
     * (deviceMorphKeyFrames); the host copy then lags behind by that morph (pendingMorph) and the rotations after it, and
     * syncHost() catches it up.  Returns 0 when done, -1 when the request cannot be served (fewer than three frames, the
     * current frame is a key frame, counts or types differ, a weight that is not finite): nothing changed. */
    int morphFrame(float weight);
    /* The same with any two frames as the keys: the current frame - the stage - set anew, primitive by primitive in id
     * order, to A + weight * (B - A), the primitives of frames A and B paired by rank; material, texture coordinates and
     * movable flag are A's.  Any finite weight is served (outside 0 ... 1 it extrapolates), frameA == frameB is allowed.
     * Returns 0 when done - the stage's tree refitted in the shape it has, the frame flattened -, -1 when the request cannot
     * be served: a key that is no frame (not below getNbFrames()) or is the stage itself (the blend would destroy its own
     * key), counts or types that differ among the three frames, a weight that is not finite: nothing changed.  An engine
     * that keeps the stage resident blends it there from key frames it is handed once per upload (deviceMorphKeyFrames);
     * what morphFrame says about the host copy holds. */
    int morphBetween(unsigned int frameA, unsigned int frameB, float weight);
    bool pendingMorph() const { return m_resident.pendingMorph(); }
    void resetAddingIndex() { m_addingIndex = 0; }
    void doneWithAdding(const bool &done) { m_doneWithAdding = done; }
    void getPrimitiveOtherCenter(unsigned int index, vec3f &center);
    int getCurrentMaterial() { return m_currentMaterial; }
    void setCurrentMaterial(const int currentMaterial) { m_currentMaterial = currentMaterial; }
    void setMaterialTextureId(unsigned int textureId);

    /* ---------- Box tree (GPUKernel.h:304-309) ---------- */
    int compactBoxes(bool reconstructBoxes);
    void streamDataToGPU();
    void resetBoxes(bool resetPrimitives);
    void setPrimitivesTransfered(const bool value) { m_resident.setTransfered(value); }

    vec3f &getViewPos() { return m_viewPos; }
    vec3f &getViewDir() { return m_viewDir; }
    vec4f &getViewAngles() { return m_angles; }

    /* ---------- Extensions (no reference equivalent) ---------- */
    /* The reference draws sceneInfo.timestamp and the random buffer from
     * rand()/time(0) in render_begin (GPUKernel.cpp:2719-2726).  With a
     * non-negative seed the timestamp given in SceneInfo is kept and the
     * random buffer is filled once from a 32-bit LCG with the reference's
     * distribution 5e-6 * (k % 2000 - 1000); -1 restores rand(). */
    void setDeterministic(long seed);
    /* flattened arrays of the current frame, as handed to the device layer */
    const std::vector<BoundingBox> &hostBoxes() { syncHost(); return m_hBoundingBoxes; }
    const std::vector<Primitive> &hostPrimitives() { syncHost(); return m_hPrimitives; }
    const std::vector<Lamp> &hostLamps() { syncHost(); return m_hLamps; }
    const std::vector<LightInformation> &hostLights() { syncHost(); return m_lightInformation; }
    /* per flattened primitive: would rotatePrimitives move it (level-0 box, movable, not the camera) */
    const std::vector<unsigned char> &hostMovable() { syncHost(); return m_hMovable; }
    /* Animated scenes: rotatePrimitives + compactBoxes(false) per frame (MoleculeScene.cpp:75-81), translatePrimitives
     * behind it (Scene.cpp:1546-1548), a lamp dragged with setPrimitiveCenter (solrViewer.cpp:1058-1069).  An
     * engine that keeps the scene resident may apply such a move there (deviceRotatePrimitives,
     * deviceTranslatePrimitives, deviceMoveLamp); the host copy then lags behind by the moves in the journal of m_resident
     * and is caught up - the same arithmetic, replayed in order - by syncHost() before anything reads or changes it. */
    void syncHost();
    size_t nbPendingRotations() const { return m_resident.nbPendingRotations(); }
    /* ... and the whole journal: rotations, translations and lamp moves */
    size_t nbPendingMoves() const { return m_resident.nbPendingMoves(); }
    int lightInformationSize() const { return m_lightInformationSize; }
    const Material *hostMaterials() const { return m_hMaterials.data(); }
    const std::vector<RandomBuffer> &hostRandoms();
    size_t randomsNeeded() const;
    void setHostBuildOnly(bool on) { m_hostBuildOnly = on; }
    const std::vector<BitmapBuffer> &hostTextureAtlas();
    PrimitiveXYIdBuffer *hostPrimitiveIds() { fetchPrimitiveIds(); return m_hPrimitivesXYIds.data(); }
    unsigned int treeDepth() const { return m_treeDepth; }

protected:
    struct Frame
    {
        BoxContainer boundingBoxes[BOUNDING_BOXES_TREE_DEPTH];
        PrimitiveContainer primitives;
        int nbActiveBoxes = 0;
        int nbActivePrimitives = 0;
        int nbActiveLamps = 0;
        vec3f minPos = {0.f, 0.f, 0.f};
        vec3f maxPos = {0.f, 0.f, 0.f};
        bool levelsBuilt = true; /* false: the flattened arrays came from the device build, the level maps are empty */
    };
    /* every access to the scene store: catches the host copy up and ends the device-side fast path until
     * the next upload (the caller may be about to change what the device holds) */
    Frame &frame()
    {
        m_resident.touch();
        /* a tree that came from the device build left the per-level maps empty: they are made now, from the
         * primitives as they still are, before whoever asks can change one (the cells a primitive sits in are
         * those of the last full build, GPUKernel.cpp:1378-1460 refits them, it does not re-hash) */
        if (!m_frames[m_frame].levelsBuilt)
            buildLevelsOnHost();
        if (m_resident.lags() && !m_resident.buildingLevels)
            syncHost();
        return m_frames[m_frame];
    }
    /* a look that changes nothing (getPrimitiveCenter, getLight ...): up to date, fast path kept */
    const CPUPrimitive *peekPrimitive(unsigned int index)
    {
        syncHost();
        return m_frames[m_frame].primitives.lookup(index);
    }
    /* counters and the frame protocol: reads that stay valid while rotations are pending */
    Frame &frameAsIs() { return m_frames[m_frame]; }
    /* engine hook: the per-pixel primitive ids of the last frame are wanted on the host (getPrimitiveAt).
     * The reference copies all of them back after every frame (CudaKernel.cpp:304-312 via d2h_bitmap) -
     * 16 bytes per pixel, five times the image - although only picking ever looks at them; an engine may
     * leave them on the device until then */
    virtual void fetchPrimitiveIds() {}
    /* m_bitmap brought up to date with the frame rendered last, where render_end(image) left it behind */
    virtual void fetchBitmap() {}
    /* engine hook: the primitives as the resident scene holds them now, written into the store (the same
     * bits a replay of the pending rotations produces - tests/test_animation_gpu.py - at a cost that does not
     * grow with their number); false = not available, replay */
    virtual bool primitivesFromDevice(Frame &) { return false; }
    /* engine hook: GPUKernel::compactBoxes(true) on the device (include/solr_hip.h, solr_hip_build_tree): the
     * flattened node list, the order in which the primitives are streamed and the number of lamps, from the
     * frame's primitives in index order.  Returns the tree depth, or a negative value when the engine has no
     * such thing or leaves this scene to the host builder */
    virtual int deviceBuildTree(const std::vector<Primitive> &, const std::vector<unsigned char> &, const vec3f &,
                                const vec3f &, float, int /* depthBefore */, std::vector<BoundingBox> &, std::vector<int> &,
                                int &)
    {
        return -2;
    }
    /* the per-level maps of the host builder, built when something needs them after a device-side build
     * (host-side rotations and translations, compactBoxes(false)) */
    void ensureLevels();
    bool buildTreeOnDevice();
    void buildLevelsOnHost();
    /* engine hooks of the frame bank: set the resident scene aside under that frame's number; make the scene set aside
     * under it the resident one; drop the one of that frame (-1: all of them).  false = not done, nothing changed */
    virtual bool deviceParkScene(unsigned int) { return false; }
    virtual bool deviceResumeScene(unsigned int) { return false; }
    virtual void deviceDropParked(long) {}
    /* ... and the most the engine may hold of them (setFrameBank hands it on, the 0 too) */
    virtual void deviceSetBankBytes(unsigned long long) {}
    /* setFrame, nextFrame, previousFrame: the store caught up, then the switch - through the bank when it is on */
    void switchFrame(unsigned int frame);
    /* every parked frame forgotten on both sides (resetAll, cleanup, an engine that goes down or is set up anew, a resume
     * that failed) */
    void dropFrameBank();
    /* the engine has uploaded the scene of the current frame (render_begin, when an upload was due) */
    void sceneUploaded() { m_resident.uploaded(m_frame, ++m_nbSceneUploads); }
    /* a material was set: the table is uploaded again with the next frame, and a parked frame flattened under the table
     * before is flattened again when it is entered (its light records carry the materials' colours) */
    void materialsChanged()
    {
        m_materialsTransfered = false;
        ++m_materialsSerial;
    }
    /* engine hook: follow the table of materials as it is now (m_hMaterials, realigned) in the engine's table and on its
     * resident scene; false = not done, nothing changed: the table is uploaded */
    virtual bool deviceEditMaterials() { return false; }
    bool m_materialEdits = false;
    unsigned long m_nbMaterialEdits = 0;
    /* engine hook: apply the rotation to the resident scene; false = not done, nothing changed */
    virtual bool deviceRotatePrimitives(const vec3f &, const vec3f &, const vec3f &) { return false; }
    /* engine hooks: apply the translation to the resident scene; set the centre of lamp `slot` of the resident scene (the
     * primitive m_hLamps[slot]) and of its light record; false = not done, nothing changed */
    virtual bool deviceTranslatePrimitives(const vec3f &) { return false; }
    virtual bool deviceMoveLamp(int, const vec3f &) { return false; }
    /* engine hook: set these primitives of the resident scene anew (every index is in the store); false = not done, nothing
     * changed */
    virtual bool deviceSetPrimitives(const SolrPrimitiveEdit *, int) { return false; }
    /* for that hook: the batch as the engine takes it - of several records for one index the last one only (setPrimitive
     * resets everything a record can set), each with the slot of its primitive in the flattened order, from a map made
     * once per upload.  False when the store's side of the engine's conditions fails: an index without exactly one slot,
     * a slot among the lamps', another material than the primitive has now - with what is pending - (tags and colour keys
     * are a join with the materials), an emissive material (the light record would have to follow), a float that is not finite */
    bool editSlots(const SolrPrimitiveEdit *edits, int n, std::vector<SolrPrimitiveEdit> &last, std::vector<int> &slots);
    /* setPrimitives' loop over the records (no box is updated) */
    void setPrimitivesOnly(const SolrPrimitiveEdit *edits, int n);
    /* engine hook: give these primitives of the resident scene these materials (every index is in the store); false = not
     * done, nothing changed */
    virtual bool deviceSetPrimitiveMaterials(const int *, const int *, int) { return false; }
    /* for that hook: the batch as the engine takes it - each slot of the flattened order once, with the material the last
     * record for its primitive names.  False when the store's side of the engine's conditions fails: an index without
     * exactly one slot, a slot among the lamps' (the light record carries the material), a material id that is negative or
     * beyond the active ones */
    bool materialSlots(const int *indices, const int *materialIds, int n, std::vector<int> &slots, std::vector<int> &lastIds);
    /* store index -> slot of the flattened order of the resident scene (m_slotOf), made once per upload */
    void ensureSlotMap();
    /* engine hook: the pixel stage of a JPEG texture (csrc/jpeg_pixels.h) - coefficient blocks as
     * ImageLoader::parseJPEG leaves them to frame.width * frame.height * 3 bytes in `rgb`.  Here: a loop on the CPU;
     * false = the engine failed (its error is pending) */
    virtual bool jpegPixels(const SolrJpegFrame &frame, const std::vector<short> &coefficients, unsigned char *rgb);
    /* engine hook: the pixel stage of a JPEG screenshot (csrc/jpeg_encode.h) - width * height * 3 bytes in `rgb`, read
     * as `source` says, to quantised coefficient blocks in MCU and zigzag order (`coefficients` is resized).  Here: a
     * loop on the CPU; false = the arguments are out of range or the engine failed (its error is pending) */
    virtual bool jpegCoefficients(const SolrJpegSource &source, const unsigned char *rgb,
                                  std::vector<short> &coefficients);
    /* engine hooks: the entropy stage of the JPEG writer (csrc/jpeg_entropy.h) - the entropy-coded segment, stuffed and
     * completed, no EOI (`scan` is resized).  jpegScan: of nbBlocks coefficient blocks as jpegCoefficients leaves them (of
     * `source` the size and sampling matter); jpegScanOf: of a picture, both stages.  Here: JpegWriter::scan, the header's
     * loops in the decomposed order; false = the arguments are out of range, a block is outside what the standard tables
     * code, or the engine failed (its error is pending).  optimised (here and in jpegScanOfFrame) not null: the segment is
     * coded with tables built for its own symbols, which come back there for the header */
    virtual bool jpegScan(const SolrJpegSource &source, const short *coefficients, long nbBlocks,
                          std::vector<unsigned char> &scan, SolrJpegHuffman *optimised = nullptr);
    virtual bool jpegScanOf(const SolrJpegSource &source, const unsigned char *rgb, std::vector<unsigned char> &scan,
                            SolrJpegHuffman *optimised = nullptr);
    /* engine hook of renderJpeg: the frame render_begin has just launched as the entropy-coded segment of its JPEG, taken
     * from the device's image - the frame never reaches the host as pixels, m_bitmap is left alone.  false (here, always):
     * not this way; the caller goes through render_end and encodeJpeg */
    virtual bool jpegScanOfFrame(int jpegQuality, int lumaH, int lumaV, std::vector<unsigned char> &scan,
                                 SolrJpegHuffman *optimised = nullptr);
    /* engine hooks of renderJpegBegin / renderJpegEnd.  jpegStreamOffered: the engine would take the next frame for
     * delivery as a JPEG in flight (here: never) - asked before the frame is rendered, because such a frame is rendered
     * with m_jpegStreamFrame set.  jpegBeginOfFrame: the frame render_begin has just launched, submitted; the engine's
     * ticket, or -1.  jpegEndOfFrame: that ticket's entropy-coded segment, and with `optimised` its tables; waits for
     * that frame alone.  false: the ticket is stale or the engine failed (its error is pending) */
    virtual bool jpegStreamOffered() { return false; }
    virtual int jpegBeginOfFrame(int jpegQuality, int lumaH, int lumaV, bool optimise);
    virtual bool jpegEndOfFrame(int engineTicket, std::vector<unsigned char> &scan, SolrJpegHuffman *optimised);
    /* engine hooks: the iso-surface of a field of metaballs (csrc/iso_surface.h).  isoSurface: balls to triangles, cubes in
     * index order (`triangles` is resized); isoField: balls to (N+1)^3 records of {nx, ny, nz, value}; isoTriangles: such
     * a field to triangles - the number the surface has, the first min(count, capacity) written, -1 on failure.  Here:
     * loops on the CPU; false / -1 = the arguments are out of range or the engine failed (its error is pending) */
    virtual bool isoSurface(const SolrIsoGrid &grid, const float *balls, int nbBalls,
                            std::vector<SolrIsoTriangle> &triangles);
    virtual bool isoField(const SolrIsoGrid &grid, const float *balls, int nbBalls, float *field);
    virtual int isoTriangles(const SolrIsoGrid &grid, const float *field, SolrIsoTriangle *triangles, int capacity);
    /* engine hook of stickPairsOf.  Here: the loops of csrc/stick_pairs.h on the CPU; false = the arguments are out of
     * range.  An engine with a device searches there and comes back here where it has none, where the device declines
     * (more pairs than it indexes) or where it fails (its error is pending) */
    virtual bool stickPairs(const float *atoms, const unsigned char *backbone, int n, float reachPlain, float reachBackbone,
                            std::vector<long long> &start, std::vector<int> &partners);
    /* a search has been served: by a device, or by the loops */
    static void countStickSearch(bool onDevice);
    void rotatePrimitivesOnly(Frame &f, const vec3f &rotationCenter, const vec3f &cosA, const vec3f &sinA);
    /* translatePrimitives' loop over the level-0 boxes (no box is updated) */
    void translatePrimitivesOnly(Frame &f, const vec3f &translation);
    void refitBoxes(Frame &f);
    /* morphBetween's body; track: an engine serves it from the slots of a track, else through its two-key interface */
    int morphKeyFrames(unsigned int frameA, unsigned int frameB, float weight, bool track);
    /* blend the resident scene between these key frames at that weight, the keys the engine does not hold yet handed over
     * first (morphKey, morphKeys; which ones it holds: m_resident); false = not done, nothing changed */
    bool deviceMorphKeyFrames(unsigned int frameA, unsigned int frameB, float weight, bool track);
    /* engine hooks of the two-key interface: take these keys - the two key frames in the order of the resident primitives -;
     * blend the resident scene between them at that weight; false = not done, nothing changed */
    virtual bool deviceSetMorphKeys(const std::vector<Primitive> &, const std::vector<Primitive> &) { return false; }
    virtual bool deviceMorphPrimitives(float) { return false; }
    /* engine hooks of a track: take this key frame - its primitives in id order, and per resident primitive its rank in
     * that order - into that slot; blend the resident scene between two slots; false = not done, nothing changed */
    virtual bool deviceSetMorphTrackKey(unsigned int, const std::vector<Primitive> &, const std::vector<int> &) { return false; }
    virtual bool deviceMorphBetween(unsigned int, unsigned int, float) { return false; }
    /* the current frame against the two key frames: counts, types by rank */
    bool morphKeysMatch(unsigned int frameA, unsigned int frameB);
    /* morphBetween's loop over the store of the current frame (no boxes, no flattening) */
    void morphPrimitivesOnly(unsigned int frameA, unsigned int frameB, float weight);
    /* a key frame as records in id order (of a record only the geometry, the type and the index are filled in); compare:
     * false when a primitive of the current frame differs from the key's in what a morph takes from its first key and a
     * resident scene keeps as it is - material, texture coordinates, movable flag */
    bool morphKey(unsigned int frame, bool compare, std::vector<Primitive> &key);
    /* per primitive of the flattened order its rank in id order, of upload number m_rankOfUpload; nullptr when the flattened
     * arrays do not describe the current frame */
    const std::vector<int> *residentRanks();
    /* the two key frames in the order of the flattened primitives, the first one compared (morphKey) */
    bool morphKeys(unsigned int frameA, unsigned int frameB, std::vector<Primitive> &first, std::vector<Primitive> &last);
    /* the engine's resident scene against the store: who serves a move, and what the store owes afterwards */
    ResidentScene m_resident;
    /* editSlots: store index -> slot of the flattened order (-1: none, -2: several), of upload number m_slotOfUpload */
    std::vector<int> m_slotOf;
    unsigned long m_slotOfUpload = 0;
    std::vector<int> m_rankOf;
    unsigned long m_rankOfUpload = 0;
    /* the frame bank: per parked frame - never the current one - what the host knows of the scene the engine has set aside
     * and the flattened arrays of that frame, everything streamDataToGPU writes */
    struct ParkedFrame
    {
        ResidentScene resident;
        std::vector<BoundingBox> boundingBoxes;
        std::vector<Primitive> primitives;
        std::vector<Lamp> lamps;
        std::vector<unsigned char> movable;
        std::vector<LightInformation> lightInformation;
        int lightInformationSize = 0;
        size_t maxPrimitivesPerBox = 0;
        unsigned long materialsSerial = 0; /* m_flattenedSerial of its arrays: their light records carry colours */
    };
    std::map<unsigned int, ParkedFrame> m_parked;
    unsigned long long m_frameBankBytes = 0;
    unsigned long m_nbFrameSwitches = 0, m_nbSceneUploads = 0; /* (the latter is also the serial ResidentScene::uploads draws) */
    unsigned long m_materialsSerial = 0; /* how often the materials were changed */
    /* ... and m_materialsSerial when the flattened arrays were made (streamDataToGPU, the device build): their light
     * records carry the materials' colours.  A frame flattened under another table is neither parked nor taken as resumed */
    unsigned long m_flattenedSerial = 0;
    bool m_flattenDue = false; /* the flattened arrays went into the bank and the frame entered had none there */

    /* box-tree build (GPUKernel.h:318-324) */
    int processBoxes(const int boxSize, bool simulate);
    int processOutterBoxes(const int boxSize, const int boundingBoxesDepth);
    bool updateBoundingBox(CPUBoundingBox &box);
    bool updateOutterBoundingBox(CPUBoundingBox &box, const int depth);
    void resetBox(CPUBoundingBox &box, bool resetPrimitives);
    void recursiveDataStreamToGPU(const int depth, CPUBoundingBox &parent);
    void appendPrimitive(long id, bool inLevel0Box);
    void fillRandoms();

    float vectorLength(const vec3f &v);
    void normalizeVector(vec3f &v);
    vec3f crossProduct(const vec3f &b, const vec3f &c);
    void rotateVector(vec3f &v, const vec3f &rotationCenter, const vec3f &cosAngles, const vec3f &sinAngles);

protected:
    /* flattened, device-bound arrays (reference: GPUKernel.h:328-339) */
    std::vector<BoundingBox> m_hBoundingBoxes;
    std::vector<Primitive> m_hPrimitives;
    std::vector<Lamp> m_hLamps;
    std::vector<unsigned char> m_hMovable;
    std::vector<Material> m_hMaterials;
    TextureInfo m_hTextures[NB_MAX_TEXTURES];
    std::map<int, std::string> m_textureFilenames;
    std::vector<BitmapBuffer> m_textureAtlas;
    std::vector<RandomBuffer> m_hRandoms;
    bool m_randomsFilled = false;
    bool m_hostBuildOnly = false; /* SolRx_HostBuild(1) / SOLR_HOST_BUILD=1: never ask the engine for the tree */
    std::vector<PrimitiveXYIdBuffer> m_hPrimitivesXYIds;
    std::vector<LightInformation> m_lightInformation;
    std::vector<BitmapBuffer> m_bitmap;

    std::map<unsigned int, Frame> m_frames;
    int m_nbActiveMaterials;
    int m_nbActiveTextures;
    int m_lightInformationSize;
    size_t m_maxPrimitivesPerBox;
    bool m_doneWithAdding;
    int m_currentMaterial = 0;
    int m_addingIndex;

    vec3f m_viewPos;
    vec3f m_viewDir;
    vec4f m_angles;

    unsigned int m_frame;
    unsigned int m_nbFrames;
    unsigned int m_treeDepth;
    /* m_treeDepth as the last compactBoxes(true) found it (the constructor's 2, or the depth of the build before): the
     * level whose box 0 the reference resets - and so creates - before it builds (GPUKernel.cpp:1049) */
    unsigned int m_depthBeforeBuild = 2;

    bool m_materialsTransfered;
    bool m_texturesTransfered;
    bool m_randomsTransfered;

    SceneInfo m_sceneInfo;
    PostProcessingInfo m_postProcessingInfo;
    bool m_refresh;
    std::string m_gpuDescription;
    vec2i m_occupancyParameters;
    bool m_buffersInitialized;
    long m_deterministicSeed;
};

/* reference: GPUKernel.h:446-455 */
class SingletonKernel
{
public:
    static GPUKernel *kernel();
    /* extension: "hip" (default) or "host-only" (scene store without a
     * device, render_begin fails loudly; used by the CPU test-suite) */
    static void selectEngine(const char *name);
    static void destroy();

private:
    SingletonKernel();
    static GPUKernel *m_kernel;
};
}
