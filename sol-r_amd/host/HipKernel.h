/*
 * HipKernel.h - the engine class that drives the MI355X device layer.
 *
 * Takes the place of the reference's solr::CudaKernel
 * (reference: solr/engines/cuda/CudaKernel.h:27-72, CudaKernel.cpp:81-389):
 * a GPUKernel subclass whose render_begin performs the dirty-flag driven
 * uploads and launches the frame through the ten extern "C" entry points of
 * include/solr_hip.h, and whose render_end brings the bitmap and primitive
 * ids back.  No OpenGL calls (the reference blits in render_end,
 * CudaKernel.cpp:313-388; see INTEGRATION.md for where that block goes).
 */
#pragma once

#include <deque>
#include <set>

#include "GPUKernel.h"

namespace solr
{
class HipKernel : public GPUKernel
{
public:
    HipKernel();
    ~HipKernel();

    void initBuffers() override;
    void cleanup() override;
    void reshape() override;
    void queryDevice() override;
    std::string getGPUDescription() override { return m_gpuDescription; }

    /* reference: CudaKernel.h:44-47 */
    void initializeDevice();
    void releaseDevice();
    void resetBoxesAndPrimitives() {}

    /* reference: CudaKernel.cpp:174-302 / 304-389 */
    void render_begin(const float timer) override;
    void render_end() override;
    void render_end(BitmapBuffer *image) override;
    int lastError(std::string *message = nullptr) override;
    void setFramesInFlight(int n) override;
    int getFramesInFlight() const override { return m_flights; }
    void flushFrames() override;
    void setGpuCount(int n) override;
    int getGpuCount() const override;

    /* reference: CudaKernel.h:59-65; accepted and forwarded, the wave64 tile
     * shape is the engine's choice */
    void setBlockSize(int x, int y, int z)
    {
        m_blockSize.x = x;
        m_blockSize.y = y;
        m_blockSize.z = z;
    }
    void setSharedMemSize(int sharedMemSize) { m_sharedMemSize = sharedMemSize; }

protected:
    /* rotatePrimitives on the resident scene, solr_hip_rotate_primitives (include/solr_hip.h) */
    bool deviceRotatePrimitives(const vec3f &center, const vec3f &cosA, const vec3f &sinA) override;
    /* morphFrame on the resident scene, solr_hip_set_morph_keys + solr_hip_morph_primitives (include/solr_hip.h) */
    bool deviceSetMorphKeys(const std::vector<Primitive> &first, const std::vector<Primitive> &last) override;
    bool deviceMorphPrimitives(float weight) override;
    /* morphBetween on the resident scene, solr_hip_set_morph_track_key + solr_hip_morph_between (include/solr_hip.h) */
    bool deviceSetMorphTrackKey(unsigned int slot, const std::vector<Primitive> &key, const std::vector<int> &rankOf) override;
    bool deviceMorphBetween(unsigned int slotA, unsigned int slotB, float weight) override;
    /* translatePrimitives and a lamp's setPrimitiveCenter on the resident scene, solr_hip_translate_primitives and
     * solr_hip_move_lamp (include/solr_hip.h) */
    bool deviceTranslatePrimitives(const vec3f &translation) override;
    bool deviceMoveLamp(int slot, const vec3f &center) override;
    /* setPrimitives on the resident scene, solr_hip_set_primitives (include/solr_hip.h): store indices to slots first */
    bool deviceSetPrimitives(const SolrPrimitiveEdit *edits, int n) override;
    /* setPrimitiveMaterials on the resident scene, solr_hip_set_primitive_materials (include/solr_hip.h): store indices to
     * slots first, each slot once */
    bool deviceSetPrimitiveMaterials(const int *indices, const int *materialIds, int n) override;
    /* an edited table of materials on the resident scene, solr_hip_edit_materials (include/solr_hip.h) */
    bool deviceEditMaterials() override;
    /* the frame bank on the engine: solr_hip_park_scene, solr_hip_resume_scene, solr_hip_drop_parked_scenes
     * (include/solr_hip.h), the frame's number as the key */
    bool deviceParkScene(unsigned int frame) override;
    bool deviceResumeScene(unsigned int frame) override;
    void deviceDropParked(long frame) override;
    void deviceSetBankBytes(unsigned long long bytes) override;
    void fetchPrimitiveIds() override;
    void fetchBitmap() override;
    bool primitivesFromDevice(Frame &f) override;
    int deviceBuildTree(const std::vector<Primitive> &primitives, const std::vector<unsigned char> &emissive,
                        const vec3f &minPos, const vec3f &maxPos, float viewDistance, int depthBefore,
                        std::vector<BoundingBox> &boxes, std::vector<int> &order, int &nbLamps) override;
    /* solr_hip_jpeg_to_rgb (include/solr_hip.h) where there is a device, the base class's loop where there is none */
    bool jpegPixels(const SolrJpegFrame &frame, const std::vector<short> &coefficients, unsigned char *rgb) override;
    /* solr_hip_rgb_to_jpeg_blocks (include/solr_hip.h) where there is a device, the base class's loop where there is none */
    bool jpegCoefficients(const SolrJpegSource &source, const unsigned char *rgb,
                          std::vector<short> &coefficients) override;
    /* solr_hip_jpeg_blocks_to_scan, solr_hip_rgb_to_jpeg_scan (include/solr_hip.h) where there is a device, the base
     * class's loops where there is none; solr_hip_frame_to_jpeg_scan for a frame rendered one at a time on one device */
    bool jpegScan(const SolrJpegSource &source, const short *coefficients, long nbBlocks, std::vector<unsigned char> &scan,
                  SolrJpegHuffman *optimised = nullptr) override;
    bool jpegScanOf(const SolrJpegSource &source, const unsigned char *rgb, std::vector<unsigned char> &scan,
                    SolrJpegHuffman *optimised = nullptr) override;
    bool jpegScanOfFrame(int jpegQuality, int lumaH, int lumaV, std::vector<unsigned char> &scan,
                         SolrJpegHuffman *optimised = nullptr) override;
    /* JPEG frames in flight: solr_hip_jpeg_stream_offered, solr_hip_frame_to_jpeg_async, solr_hip_jpeg_wait */
    bool jpegStreamOffered() override;
    int jpegBeginOfFrame(int jpegQuality, int lumaH, int lumaV, bool optimise) override;
    bool jpegEndOfFrame(int engineTicket, std::vector<unsigned char> &scan, SolrJpegHuffman *optimised) override;
    /* solr_hip_metaballs, solr_hip_iso_field, solr_hip_iso_surface (include/solr_hip.h) where there is a device, the base
     * class's loops where there is none */
    bool isoSurface(const SolrIsoGrid &grid, const float *balls, int nbBalls,
                    std::vector<SolrIsoTriangle> &triangles) override;
    bool isoField(const SolrIsoGrid &grid, const float *balls, int nbBalls, float *field) override;
    int isoTriangles(const SolrIsoGrid &grid, const float *field, SolrIsoTriangle *triangles, int capacity) override;
    /* solr_hip_stick_pairs (include/solr_hip.h) where there is a device and the molecule has stickDeviceFrom() atoms or
     * more; the base class's loops below that, where there is no device, where
     * the entry declines (more than 2^31 - 1 pairs) and where it reports an error (which stays pending) */
    bool stickPairs(const float *atoms, const unsigned char *backbone, int n, float reachPlain, float reachBackbone,
                    std::vector<long long> &start, std::vector<int> &partners) override;

private:
    vec4i m_blockSize;
    int m_sharedMemSize;
    bool m_deviceInitialized;
    bool m_idsOnDevice = false;
    size_t m_isoCapacity = 4096; /* triangles the buffer of the next isoSurface call starts with */
    size_t m_jpegCapacity = 65536; /* bytes the buffer of the next entropy-coded segment starts with */
    bool m_streamed = false;      /* the frame render_begin launched counts its tiles: render_end takes its image band by band */
    bool m_bitmapOnDevice = false; /* render_end(image) delivered to the caller's array: m_bitmap follows when asked */
    unsigned m_sharedSeed = 0, m_sharedState = 0; /* solr_hip_comm_shared_seed and the generator it seeds (render_begin) */
    int m_flights = 1;            /* frames in flight through render_begin / render_end (setFramesInFlight) */
    std::deque<int> m_tickets;    /* read-backs under way, oldest first (solr_hip_d2h_image_async) */
    void deliver(int ticket);
};

/* Scene store without a device: everything up to compactBoxes works, any
 * attempt to render fails loudly.  Exists so that the host logic can be
 * tested on machines without a GPU; it is NOT a CPU rendering fallback. */
class HostOnlyKernel : public GPUKernel
{
public:
    void render_begin(const float timer) override;
    void render_end() override;
    int lastError(std::string *message = nullptr) override;

protected:
    bool m_failed = false;
};

/* Test double for the animated-scene protocol (GPUKernel::rotatePrimitives / translatePrimitives / setPrimitiveCenter /
 * morphFrame / morphBetween / syncHost): a host-only store that claims to upload the scene with a frame when an upload is due - the rule of
 * HipKernel::render_begin, through the same ResidentScene::uploaded - and to apply every move it is offered "over there".
 * What is offered (ResidentScene::offers) and the morph keys are the base class's business; the double only counts.  So the
 * lazy replay of what is pending can be checked against the eager host route without a GPU.  Renders nothing. */
class ReplayKernel : public HostOnlyKernel
{
public:
    void render_begin(const float timer) override;
    int nbClaimedRotations() const { return m_claimed; }
    int nbClaimedMorphs() const { return m_claimedMorphs; }
    int nbClaimedTrackMorphs() const { return m_claimedTrackMorphs; }
    int nbClaimedTrackKeys() const { return m_claimedTrackKeys; }
    int nbClaimedTranslations() const { return m_claimedTranslations; }
    int nbClaimedLampMoves() const { return m_claimedLampMoves; }
    int nbClaimedEdits() const { return m_claimedEdits; }
    int nbClaimedMaterialSets() const { return m_claimedMaterialSets; }
    int nbClaimedParks() const { return m_claimedParks; }
    int nbClaimedResumes() const { return m_claimedResumes; }

protected:
    /* the frame bank: every park is claimed, a resume when that frame was parked and not dropped since */
    bool deviceParkScene(unsigned int frame) override;
    bool deviceResumeScene(unsigned int frame) override;
    void deviceDropParked(long frame) override;
    bool deviceRotatePrimitives(const vec3f &, const vec3f &, const vec3f &) override;
    bool deviceSetMorphKeys(const std::vector<Primitive> &, const std::vector<Primitive> &) override { return true; }
    bool deviceMorphPrimitives(float weight) override;
    /* (a slot for every frame number a real engine has one for) */
    bool deviceSetMorphTrackKey(unsigned int slot, const std::vector<Primitive> &key, const std::vector<int> &rankOf) override;
    bool deviceMorphBetween(unsigned int slotA, unsigned int slotB, float weight) override;
    bool deviceTranslatePrimitives(const vec3f &) override;
    bool deviceMoveLamp(int slot, const vec3f &center) override;
    /* (claimed where the store's side of the engine's conditions holds: GPUKernel::editSlots) */
    bool deviceSetPrimitives(const SolrPrimitiveEdit *edits, int n) override;
    /* (claimed where the store's side of the engine's conditions holds: GPUKernel::materialSlots) */
    bool deviceSetPrimitiveMaterials(const int *indices, const int *materialIds, int n) override;

private:
    int m_claimedMaterialSets = 0;
    int m_claimed = 0, m_claimedMorphs = 0, m_claimedTranslations = 0, m_claimedLampMoves = 0, m_claimedEdits = 0;
    int m_claimedTrackMorphs = 0, m_claimedTrackKeys = 0;
    int m_claimedParks = 0, m_claimedResumes = 0;
    std::set<unsigned int> m_parkedOverThere;
};
}
