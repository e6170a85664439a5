/*
 * SolRStub.cpp - see SolRStub.h.  Call sequences follow the reference's
 * solr/SolRStub.cpp:48-164 (scene info staged in a global and applied in
 * SolR_InitializeKernel / SolR_RunKernel), :166-330 (primitives),
 * :368-424 (materials), :533-544 (boxes, lights).
 */
#include "SolRStub.h"

#include <cstring>
#include <string>
#include <vector>

#include "../../include/solr_hip.h"
#include "FileMarshaller.h"
#include "GPUKernel.h"
#include "JpegWriter.h"
#include "../csrc/jpeg_encode.h"
#include "../csrc/jpeg_entropy.h"
#include "../csrc/iso_surface.h"
#include "../csrc/stick_pairs.h"
#include "OBJReader.h"
#include "PDBReader.h"
#include "SWCReader.h"

using solr::SingletonKernel;

static SceneInfo gSceneInfoStub;
static PostProcessingInfo gPostProcessingInfoStub;

static int engineStatus()
{
    return SingletonKernel::kernel()->lastError() == 0 ? 0 : -1;
}

extern "C" {

int SolR_SetSceneInfo(int width, int height, int graphicsLevel, int nbRayIterations, double transparentColor,
                      double viewDistance, double shadowIntensity, double eyeSeparation, double bgColorR,
                      double bgColorG, double bgColorB, double bgColorA, int renderBoxes, int pathTracingIteration,
                      int maxPathTracingIterations, int frameBufferType, int timestamp, int atmosphericEffect,
                      int cameraType, int doubleSidedTriangles, int extendedGeometry, int advancedIllumination,
                      int skyboxSize, int skyboxMaterialId, double geometryEpsilon, double rayEpsilon)
{
    gSceneInfoStub.size.x = width;
    gSceneInfoStub.size.y = height;
    gSceneInfoStub.graphicsLevel = graphicsLevel;
    gSceneInfoStub.nbRayIterations = nbRayIterations;
    gSceneInfoStub.transparentColor = static_cast<float>(transparentColor);
    gSceneInfoStub.viewDistance = static_cast<float>(viewDistance);
    gSceneInfoStub.shadowIntensity = static_cast<float>(shadowIntensity);
    gSceneInfoStub.eyeSeparation = static_cast<float>(eyeSeparation);
    gSceneInfoStub.backgroundColor.x = static_cast<float>(bgColorR);
    gSceneInfoStub.backgroundColor.y = static_cast<float>(bgColorG);
    gSceneInfoStub.backgroundColor.z = static_cast<float>(bgColorB);
    gSceneInfoStub.backgroundColor.w = static_cast<float>(bgColorA);
    gSceneInfoStub.renderBoxes = renderBoxes;
    gSceneInfoStub.pathTracingIteration = pathTracingIteration;
    gSceneInfoStub.maxPathTracingIterations = maxPathTracingIterations;
    gSceneInfoStub.frameBufferType = frameBufferType;
    gSceneInfoStub.timestamp = timestamp;
    gSceneInfoStub.atmosphericEffect = atmosphericEffect;
    gSceneInfoStub.cameraType = cameraType;
    gSceneInfoStub.doubleSidedTriangles = doubleSidedTriangles;
    gSceneInfoStub.extendedGeometry = extendedGeometry;
    gSceneInfoStub.advancedIllumination = advancedIllumination;
    gSceneInfoStub.skyboxRadius = skyboxSize;
    gSceneInfoStub.skyboxMaterialId = skyboxMaterialId;
    gSceneInfoStub.geometryEpsilon = static_cast<float>(geometryEpsilon);
    gSceneInfoStub.rayEpsilon = static_cast<float>(rayEpsilon);
    return 0;
}

int SolR_SetPostProcessingInfo(int type, double param1, double param2, int param3)
{
    gPostProcessingInfoStub.type = type;
    gPostProcessingInfoStub.param1 = static_cast<float>(param1);
    gPostProcessingInfoStub.param2 = static_cast<float>(param2);
    gPostProcessingInfoStub.param3 = param3;
    return 0;
}

int SolR_SetDraftMode(int draft)
{
    gSceneInfoStub.draftMode = draft;
    return 0;
}

int SolRx_SetSceneInfoExtras(int gradientBackground, int draftMode)
{
    gSceneInfoStub.gradientBackground = gradientBackground;
    gSceneInfoStub.draftMode = draftMode;
    return 0;
}

int SolR_InitializeKernel(bool, int, int device)
{
    solr::GPUKernel *kernel = SingletonKernel::kernel();
    if (!kernel)
        return -1;
    gSceneInfoStub.pathTracingIteration = 0;
    kernel->setSceneInfo(gSceneInfoStub);
    kernel->setDeviceId(device);
    kernel->initBuffers();
    kernel->setFrame(0);
    return engineStatus();
}

int SolR_FinalizeKernel()
{
    SingletonKernel::destroy();
    return 0;
}

int SolR_ResetKernel()
{
    SingletonKernel::kernel()->resetAll();
    return 0;
}

void SolR_SetCamera(double eye_x, double eye_y, double eye_z, double dir_x, double dir_y, double dir_z,
                    double angle_x, double angle_y, double angle_z)
{
    SolRx_SetCameraW(eye_x, eye_y, eye_z, dir_x, dir_y, dir_z, angle_x, angle_y, angle_z, 6400.0);
}

void SolRx_SetCameraW(double eye_x, double eye_y, double eye_z, double dir_x, double dir_y, double dir_z,
                      double angle_x, double angle_y, double angle_z, double angle_w)
{
    const vec3f eye = solr::make_vec3f((float)eye_x, (float)eye_y, (float)eye_z);
    const vec3f dir = solr::make_vec3f((float)dir_x, (float)dir_y, (float)dir_z);
    const vec4f angles = solr::make_vec4f((float)angle_x, (float)angle_y, (float)angle_z, (float)angle_w);
    SingletonKernel::kernel()->setCamera(eye, dir, angles);
}

int SolRx_Render(double timer)
{
    solr::GPUKernel *kernel = SingletonKernel::kernel();
    kernel->setSceneInfo(gSceneInfoStub);
    kernel->setPostProcessingInfo(gPostProcessingInfoStub);
    kernel->render_begin(static_cast<float>(timer));
    kernel->render_end();
    return engineStatus();
}

/* Extension: frames in flight through SolR_RunKernel / SolRx_Render (GPUKernel::setFramesInFlight): with n > 1 a
 * call delivers the image of the frame n - 1 calls back while the newer ones render; SolRx_FlushFrames waits for
 * all of them, the next getBitmap / SolRx_GetBitmap is then the newest frame's. */
int SolRx_SetFramesInFlight(int n)
{
    SingletonKernel::kernel()->setFramesInFlight(n);
    return engineStatus();
}

/* ... and what it is set to (1 for an engine without a device) */
int SolRx_GetFramesInFlight()
{
    return SingletonKernel::kernel()->getFramesInFlight();
}

/* Extension: the frame shared out over n devices of THIS process (the reference's occupancyParameters.x, which its
 * API cannot set: CudaKernel.cpp:90); returns the number in use after the change (fewer when fewer are there) or -1 */
int SolRx_SetGpuCount(int n)
{
    SingletonKernel::kernel()->setGpuCount(n);
    return engineStatus() == 0 ? SingletonKernel::kernel()->getGpuCount() : -1;
}

int SolRx_FlushFrames(void)
{
    SingletonKernel::kernel()->flushFrames();
    return engineStatus();
}

/* the image render_end delivered last, without a copy (valid until four more frames were rendered) */
const BitmapBuffer *SolRx_GetBitmap(void)
{
    return SingletonKernel::kernel()->getBitmap();
}

int SolR_RunKernel(double timer, BitmapBuffer *image)
{
    /* reference: SolRStub.cpp:154-164 - render_begin, render_end, then m_bitmap copied to the caller.  render_end(image)
     * is those last two steps (an engine with a device delivers straight into `image`, GPUKernel.h) */
    if (!image)
        return -1;
    solr::GPUKernel *kernel = SingletonKernel::kernel();
    kernel->setSceneInfo(gSceneInfoStub);
    kernel->setPostProcessingInfo(gPostProcessingInfoStub);
    kernel->render_begin(static_cast<float>(timer));
    kernel->render_end(image);
    return engineStatus();
}

/* reference: SolRStub.cpp:546-550 - always 0.  `quality` is the number of path-tracing passes, not the JPEG quality
 * (GPUKernel::generateScreenshot).  The scene and post-processing settings are the ones SolR_RunKernel would render with. */
int SolR_GenerateScreenshot(char *filename, int width, int height, int quality)
{
    solr::GPUKernel *kernel = SingletonKernel::kernel();
    kernel->setSceneInfo(gSceneInfoStub);
    kernel->setPostProcessingInfo(gPostProcessingInfoStub);
    kernel->generateScreenshot(filename ? filename : "", width < 0 ? 0 : width, height < 0 ? 0 : height,
                               quality < 0 ? 0 : quality);
    return 0;
}

/* Extension: the screenshot's encoder alone on the caller's pixels (GPUKernel::encodeJpeg): 0, or -1 when an argument is
 * out of range - nothing is written then - or the file could not be written */
static int encodeJpegFile(const char *filename, const unsigned char *pixels, int width, int height, int jpegQuality,
                          int lumaH, int lumaV, int turned, int swapRedBlue, bool optimise)
{
    if (!filename || !pixels)
        return -1;
    return SingletonKernel::kernel()->encodeJpeg(filename, pixels, width, height, jpegQuality, lumaH, lumaV,
                                                 turned != 0, swapRedBlue != 0, optimise)
               ? 0
               : -1;
}

int SolRx_EncodeJpeg(const char *filename, const unsigned char *pixels, int width, int height, int jpegQuality,
                     int lumaH, int lumaV, int turned, int swapRedBlue)
{
    return encodeJpegFile(filename, pixels, width, height, jpegQuality, lumaH, lumaV, turned, swapRedBlue, false);
}

/* ... with optimised Huffman tables (GPUKernel.h, encodeJpeg) */
int SolRx_EncodeJpegOptimised(const char *filename, const unsigned char *pixels, int width, int height, int jpegQuality,
                              int lumaH, int lumaV, int turned, int swapRedBlue)
{
    return encodeJpegFile(filename, pixels, width, height, jpegQuality, lumaH, lumaV, turned, swapRedBlue, true);
}

/* Extensions for the tests of the encoder's two halves.  SolRx_JpegCoefficients: the engine's pixel stage alone
 * (GPUKernel::jpegCoefficients) - `coefficients` has room for nbBlocks blocks of 64, which must be the number the
 * picture has.  SolRx_JpegFromCoefficients: the writer alone (host/JpegWriter.h).  SolRx_JpegQuantise: count values
 * first, first + 1, ... (negated if negative != 0) through jpe::quantise with quantiser q. */
int SolRx_JpegCoefficients(const unsigned char *pixels, int width, int height, int jpegQuality, int lumaH, int lumaV,
                           int turned, int swapRedBlue, short *coefficients, long nbBlocks)
{
    if (!pixels || !coefficients)
        return -1;
    const SolrJpegSource source = {width, height, lumaH, lumaV, jpegQuality, turned, swapRedBlue};
    std::vector<short> blocks;
    if (!SingletonKernel::kernel()->jpegCoefficientsOf(source, pixels, blocks) || (long)(blocks.size() / 64) != nbBlocks)
        return -1;
    memcpy(coefficients, blocks.data(), blocks.size() * sizeof(short));
    return 0;
}

static int jpegFromCoefficients(const char *filename, const short *coefficients, long nbBlocks, int width, int height,
                                int jpegQuality, int lumaH, int lumaV, bool optimise)
{
    if (!filename || !coefficients || width < 1 || height < 1 || jpegQuality < 1 || jpegQuality > 100 ||
        !jpe::samplingSupported(lumaH, lumaV) ||
        nbBlocks != (long)((width + 8 * lumaH - 1) / (8 * lumaH)) * ((height + 8 * lumaV - 1) / (8 * lumaV)) *
                        jpe::blocksPerMcu(lumaH, lumaV))
        return -1;
    unsigned short quant[2][64];
    jpe::quantTable(jpegQuality, 0, quant[0]);
    jpe::quantTable(jpegQuality, 1, quant[1]);
    return solr::JpegWriter::writeFile(filename, solr::JpegWriter::encode(width, height, lumaH, lumaV, quant,
                                                                          coefficients, nbBlocks, optimise))
               ? 0
               : -1;
}

int SolRx_JpegFromCoefficients(const char *filename, const short *coefficients, long nbBlocks, int width, int height,
                               int jpegQuality, int lumaH, int lumaV)
{
    return jpegFromCoefficients(filename, coefficients, nbBlocks, width, height, jpegQuality, lumaH, lumaV, false);
}

int SolRx_JpegFromCoefficientsOptimised(const char *filename, const short *coefficients, long nbBlocks, int width,
                                        int height, int jpegQuality, int lumaH, int lumaV)
{
    return jpegFromCoefficients(filename, coefficients, nbBlocks, width, height, jpegQuality, lumaH, lumaV, true);
}

/* a file in memory into the caller's buffer: 0; -1 with *nbBytes = the size needed when it does not fit (nothing is
 * written) */
static int jpegFileOut(const std::vector<unsigned char> &bytes, unsigned char *file, long capacity, long *nbBytes)
{
    *nbBytes = (long)bytes.size();
    if (*nbBytes > capacity)
        return -1;
    memcpy(file, bytes.data(), bytes.size());
    return 0;
}

/* Extension: the file of SolRx_JpegFromCoefficients in memory, its entropy-coded segment by the engine's entropy stage
 * (GPUKernel::jpegFileFromCoefficients: the device's kernels, or the same steps in loops).  -1 with *nbBytes = 0: an
 * argument out of range, a block outside what the standard tables code, or the engine failed */
static int jpegFileFromCoefficients(const short *coefficients, long nbBlocks, int width, int height, int jpegQuality,
                                    int lumaH, int lumaV, unsigned char *file, long capacity, long *nbBytes, bool optimise)
{
    if (!nbBytes)
        return -1;
    *nbBytes = 0;
    std::vector<unsigned char> bytes;
    if (!coefficients || !file || capacity < 0 ||
        !SingletonKernel::kernel()->jpegFileFromCoefficients(bytes, coefficients, nbBlocks, width, height, jpegQuality,
                                                             lumaH, lumaV, optimise))
        return -1;
    return jpegFileOut(bytes, file, capacity, nbBytes);
}

int SolRx_JpegFileFromCoefficients(const short *coefficients, long nbBlocks, int width, int height, int jpegQuality,
                                   int lumaH, int lumaV, unsigned char *file, long capacity, long *nbBytes)
{
    return jpegFileFromCoefficients(coefficients, nbBlocks, width, height, jpegQuality, lumaH, lumaV, file, capacity,
                                    nbBytes, false);
}

int SolRx_JpegFileFromCoefficientsOptimised(const short *coefficients, long nbBlocks, int width, int height,
                                            int jpegQuality, int lumaH, int lumaV, unsigned char *file, long capacity,
                                            long *nbBytes)
{
    return jpegFileFromCoefficients(coefficients, nbBlocks, width, height, jpegQuality, lumaH, lumaV, file, capacity,
                                    nbBytes, true);
}

/* Extension: one frame as SolR_RunKernel renders it, delivered as a JPEG file in memory (GPUKernel::renderJpeg): with
 * the HIP engine the frame is coded on the device and only the file crosses to the host; SolRx_GetBitmap() is not
 * refreshed.  A file that does not fit is not kept: the next call renders the next frame */
static int renderJpeg(double timer, int jpegQuality, int lumaH, int lumaV, unsigned char *file, long capacity,
                      long *nbBytes, bool optimise)
{
    if (!nbBytes)
        return -1;
    *nbBytes = 0;
    if (!file || capacity < 0)
        return -1;
    solr::GPUKernel *kernel = SingletonKernel::kernel();
    kernel->setSceneInfo(gSceneInfoStub);
    kernel->setPostProcessingInfo(gPostProcessingInfoStub);
    std::vector<unsigned char> bytes;
    if (!kernel->renderJpeg(static_cast<float>(timer), jpegQuality, lumaH, lumaV, bytes, optimise))
        return -1;
    return jpegFileOut(bytes, file, capacity, nbBytes);
}

int SolRx_RenderJpeg(double timer, int jpegQuality, int lumaH, int lumaV, unsigned char *file, long capacity,
                     long *nbBytes)
{
    return renderJpeg(timer, jpegQuality, lumaH, lumaV, file, capacity, nbBytes, false);
}

int SolRx_RenderJpegOptimised(double timer, int jpegQuality, int lumaH, int lumaV, unsigned char *file, long capacity,
                              long *nbBytes)
{
    return renderJpeg(timer, jpegQuality, lumaH, lumaV, file, capacity, nbBytes, true);
}

/* Extensions: JPEG frames in flight (GPUKernel::renderJpegBegin / renderJpegEnd).  SolRx_RenderJpegBegin: the next frame
 * rendered and submitted for delivery as a JPEG file; a ticket >= 0, or -1.  SolRx_RenderJpegEnd: that ticket's file - 0;
 * -1 with *nbBytes = the size when `capacity` is too small (nothing written; the ticket stays good, no frame is rendered
 * again); -1 with *nbBytes = 0 for a stale or never-issued ticket or a failed frame, SolRx_RenderJpegTicketError then says
 * which.  SolRx_JpegParkPixels (for the tests): the caller's pixels, read as a frame is read, parked under a ticket */
int SolRx_RenderJpegBegin(double timer, int jpegQuality, int lumaH, int lumaV, int optimised)
{
    solr::GPUKernel *kernel = SingletonKernel::kernel();
    kernel->setSceneInfo(gSceneInfoStub);
    kernel->setPostProcessingInfo(gPostProcessingInfoStub);
    return kernel->renderJpegBegin(static_cast<float>(timer), jpegQuality, lumaH, lumaV, optimised != 0);
}

int SolRx_RenderJpegEnd(int ticket, unsigned char *file, long capacity, long *nbBytes)
{
    if (!nbBytes)
        return -1;
    *nbBytes = 0;
    if (!file || capacity < 0)
        return -1;
    std::vector<unsigned char> *bytes = nullptr;
    if (!SingletonKernel::kernel()->renderJpegEnd(ticket, bytes))
        return -1;
    return jpegFileOut(*bytes, file, capacity, nbBytes);
}

int SolRx_RenderJpegTicketError(char *buf, int len)
{
    const std::string &message = SingletonKernel::kernel()->jpegTicketError();
    if (buf && len > 0)
    {
        strncpy(buf, message.c_str(), len - 1);
        buf[len - 1] = 0;
    }
    return message.empty() ? 0 : -1;
}

int SolRx_JpegParkPixels(const unsigned char *pixels, int width, int height, int jpegQuality, int lumaH, int lumaV,
                         int swapRedBlue, int optimised)
{
    if (!pixels)
        return -1;
    return SingletonKernel::kernel()->jpegParkPixels(pixels, width, height, jpegQuality, lumaH, lumaV, swapRedBlue != 0,
                                                     optimised != 0);
}

/* Extension for the tests of the plan of a resident pipeline (csrc/jpeg_entropy.h, planScan): out[0 ... 4] = total bits,
 * unstuffed bytes, stream words, chunks, flag for a scan's total and flag; out[5 ... 8] = the bounds of nbBlocks blocks:
 * bits, bytes, chunks, stuffed bytes */
void SolRx_JpegEntropyPlan(unsigned long long totalBits, int flag, long nbBlocks, unsigned long long out[9])
{
    const jpn::ScanPlan plan = jpn::planScan(totalBits, (jpn::u32)flag);
    out[0] = plan.totalBits;
    out[1] = plan.unstuffedBytes;
    out[2] = plan.streamWords;
    out[3] = plan.nbChunks;
    out[4] = plan.flag;
    out[5] = jpn::maxStreamBits(nbBlocks);
    out[6] = jpn::maxStreamBytes(nbBlocks);
    out[7] = jpn::maxStreamChunks(nbBlocks);
    out[8] = jpn::maxStuffedBytes(nbBlocks);
}

/* ... and of the functions it is held to: out[0 ... 2] = streamBytes, streamWords, tailBits of totalBits */
void SolRx_JpegEntropyStreamSizes(unsigned long long totalBits, unsigned long long out[3])
{
    out[0] = jpn::streamBytes(totalBits);
    out[1] = jpn::streamWords(totalBits);
    out[2] = (unsigned long long)jpn::tailBits(totalBits);
}

/* Extensions for the tests of the optimised tables (csrc/jpeg_entropy.h): the table builder on a histogram of the
 * caller's; the census of the caller's blocks, in the order of jpn::Census */
int SolRx_JpegOptimiseTable(const unsigned int *counts, int len, unsigned char *bits, unsigned char *values)
{
    if (!counts || !bits || !values || len < 1 || len > 256)
        return -1;
    return jpn::optimiseTable(counts, len, bits, values);
}

int SolRx_JpegCensus(const short *coefficients, long nbBlocks, int lumaBlocks, unsigned int *counts)
{
    if (!coefficients || !counts || nbBlocks < 0 || (lumaBlocks != 1 && lumaBlocks != 2 && lumaBlocks != 4))
        return -1;
    jpn::Census census = {};
    bool inside = true;
    for (long i = 0; i < nbBlocks; ++i)
    {
        const long before = jpn::predecessor(i, lumaBlocks);
        inside &= jpn::blockCensus(coefficients + i * 64, before < 0 ? 0 : (int)coefficients[before * 64],
                                   jpn::chromaOf(i, lumaBlocks), census);
    }
    if (!inside)
        return -1;
    memcpy(counts, &census, sizeof(census));
    return 0;
}

/* Extensions for the tests of csrc/jpeg_entropy.h: its granularities {blocks per workgroup, bytes per stuffing chunk};
 * its prefix sum (n lengths to n + 1 offsets of 64 bits); the bits one block takes after a predecessor's DC (-1 when
 * the block is outside the domain) */
void SolRx_JpegEntropyGranularity(int out[2])
{
    out[0] = jpn::BLOCKS_PER_GROUP;
    out[1] = jpn::STUFF_CHUNK_BYTES;
}

void SolRx_JpegEntropyPrefix(const unsigned int *lengths, long n, unsigned long long *offsets)
{
    jpn::exclusiveSum(lengths, n, offsets);
}

int SolRx_JpegBlockBits(const short *block, int previousDc, int chroma)
{
    jpn::u32 bits = 0;
    return jpn::blockBits(block, previousDc, chroma != 0, &bits) ? (int)bits : -1;
}

int SolRx_JpegQuantise(int q, int first, int count, int negative, short *out)
{
    if (q < 1 || q > 255 || first < 0 || count < 0 || (long)first + count - 1 + (q >> 1) > jpe::MAX_MAGNITUDE || !out)
        return -1;
    const jpe::u32 m = jpe::reciprocal(q);
    for (int i = 0; i < count; ++i)
        out[i] = jpe::quantise(negative ? -(first + i) : first + i, q, m);
    return 0;
}

/* Extension: GPUKernel::resetFrame */
int SolRx_ResetFrame()
{
    SingletonKernel::kernel()->resetFrame();
    return 0;
}

/* Extension: GPUKernel::addMetaballs */
int SolRx_AddMetaballs(const SolrIsoGrid *grid, const float *balls, int nbBalls, int materialId)
{
    if (!grid || !balls)
        return -1;
    return SingletonKernel::kernel()->addMetaballs(*grid, balls, nbBalls, materialId);
}

/* Extensions for the tests: the engine's field and surface stages alone (GPUKernel::isoField / isoTriangles), and the
 * table of cases the header's generator makes */
int SolRx_IsoField(const SolrIsoGrid *grid, const float *balls, int nbBalls, float *field)
{
    if (!grid || !balls || !field)
        return -1;
    return SingletonKernel::kernel()->isoFieldOf(*grid, balls, nbBalls, field) ? 0 : -1;
}

int SolRx_IsoSurface(const SolrIsoGrid *grid, const float *field, SolrIsoTriangle *triangles, int capacity)
{
    if (!grid || !field)
        return -1;
    return SingletonKernel::kernel()->isoTrianglesOf(*grid, field, triangles, capacity);
}

int SolRx_IsoCaseTable(unsigned char *count, unsigned char *edges)
{
    iso::CaseTable table;
    if (!count || !edges || !iso::buildCaseTable(table))
        return -1;
    memcpy(count, table.count, sizeof(table.count));
    memcpy(edges, table.edges, sizeof(table.edges));
    return 0;
}

/* Extension: GPUKernel::stickPairsOf */
long long SolRx_StickPairs(const float *atoms, const unsigned char *backbone, int n, float reachPlain, float reachBackbone,
                           long long *start, int *partners, long long capacity)
{
    if (sticks::refusal(atoms, backbone, n, reachPlain, reachBackbone, start, partners, capacity))
        return -1;
    std::vector<long long> starts;
    std::vector<int> all;
    if (!SingletonKernel::kernel()->stickPairsOf(atoms, backbone, n, reachPlain, reachBackbone, starts, all))
        return -1;
    std::copy(starts.begin(), starts.end(), start);
    std::copy(all.begin(), all.begin() + (size_t)std::min<long long>((long long)all.size(), capacity), partners);
    return (long long)all.size();
}

void SolRx_StickSearches(long long out[2])
{
    solr::GPUKernel::stickSearches(out);
}

int SolRx_SetStickDeviceFrom(int n)
{
    return solr::GPUKernel::setStickDeviceFrom(n);
}

float SolRx_StickSquaredReach(float reach)
{
    return sticks::squaredReach(reach);
}

static double gMoleculeLoadSeconds[3];

void SolRx_MoleculeLoadTimes(double out[3])
{
    std::copy(gMoleculeLoadSeconds, gMoleculeLoadSeconds + 3, out);
}

int SolR_AddPrimitive(int type, int movable)
{
    int id = SingletonKernel::kernel()->addPrimitive(static_cast<PrimitiveType>(type));
    SingletonKernel::kernel()->setPrimitiveIsMovable(id, (movable == 1));
    return id;
}

int SolR_SetPrimitive(int index, double p0_x, double p0_y, double p0_z, double p1_x, double p1_y, double p1_z,
                      double p2_x, double p2_y, double p2_z, double size_x, double size_y, double size_z,
                      int materialId)
{
    SingletonKernel::kernel()->setPrimitive(index, (float)p0_x, (float)p0_y, (float)p0_z, (float)p1_x, (float)p1_y,
                                            (float)p1_z, (float)p2_x, (float)p2_y, (float)p2_z, (float)size_x,
                                            (float)size_y, (float)size_z, materialId);
    return 0;
}

int SolR_GetPrimitive(int index, double *p0_x, double *p0_y, double *p0_z, double *p1_x, double *p1_y, double *p1_z,
                      double *p2_x, double *p2_y, double *p2_z, double *size_x, double *size_y, double *size_z,
                      int *materialId)
{
    solr::CPUPrimitive *p = SingletonKernel::kernel()->getPrimitive(index);
    if (!p)
        return -1;
    *p0_x = p->p0.x; *p0_y = p->p0.y; *p0_z = p->p0.z;
    *p1_x = p->p1.x; *p1_y = p->p1.y; *p1_z = p->p1.z;
    *p2_x = p->p2.x; *p2_y = p->p2.y; *p2_z = p->p2.z;
    *size_x = p->size.x; *size_y = p->size.y; *size_z = p->size.z;
    *materialId = p->materialId;
    return 0;
}

int SolR_GetPrimitiveAt(int x, int y)
{
    return SingletonKernel::kernel()->getPrimitiveAt(x, y);
}

int SolR_GetPrimitiveCenter(int index, double *x, double *y, double *z)
{
    vec4f center = SingletonKernel::kernel()->getPrimitiveCenter(index);
    *x = center.x;
    *y = center.y;
    *z = center.z;
    return 0;
}

int SolR_RotatePrimitives(int, int, double rx, double ry, double rz, double ax, double ay, double az)
{
    vec3f rotationCenter = solr::make_vec3f((float)rx, (float)ry, (float)rz);
    vec4f angles = solr::make_vec4f((float)ax, (float)ay, (float)az);
    SingletonKernel::kernel()->rotatePrimitives(rotationCenter, angles);
    SingletonKernel::kernel()->compactBoxes(false);
    return 0;
}

int SolR_LoadMolecule(char *filename, int geometryType, double defaultAtomSize, double defaultStickSize,
                      int atomMaterialType, double scale)
{
    solr::PDBReader reader;
    const float s = static_cast<float>(scale);
    reader.loadAtomsFromFile(filename ? filename : "", *SingletonKernel::kernel(),
                             static_cast<solr::GeometryType>(geometryType), static_cast<float>(defaultAtomSize),
                             static_cast<float>(defaultStickSize), atomMaterialType, solr::make_vec4f(s, s, s));
    std::copy(reader.getStepSeconds(), reader.getStepSeconds() + 3, gMoleculeLoadSeconds);
    return (int)SingletonKernel::kernel()->getNbActivePrimitives();
}

int SolR_LoadOBJModel(char *filename, int materialId, int autoScale, double scale, int autoCenter, double *height)
{
    solr::OBJReader reader;
    const float s = static_cast<float>(scale);
    solr::CPUBoundingBox aabb, inAABB;
    const vec4f size = reader.loadModelFromFile(filename ? filename : "", *SingletonKernel::kernel(),
                                                solr::make_vec4f(0.f, 0.f, 0.f), autoScale == 1,
                                                solr::make_vec4f(s, s, s), true, materialId, false, autoCenter == 1, aabb,
                                                false, inAABB);
    if (height)
        *height = -size.y / 2.f;
    return (int)SingletonKernel::kernel()->getNbActivePrimitives();
}

/* the samples of the morphology SolRx_LoadSWCMorphology read last (SolRx_GetMorphologies) */
static solr::Morphologies gMorphologies;

int SolRx_LoadSWCMorphology(const char *filename, double px, double py, double pz, double sx, double sy, double sz,
                            double sw, int materialId)
{
    solr::SWCReader reader;
    reader.loadMorphologyFromFile(filename ? filename : "", *SingletonKernel::kernel(),
                                  solr::make_vec4f((float)px, (float)py, (float)pz),
                                  solr::make_vec4f((float)sx, (float)sy, (float)sz, (float)sw), materialId);
    gMorphologies = reader.getMorphologies();
    return (int)gMorphologies.size();
}

int SolRx_GetMorphologies(SolrSwcSample *samples, int capacity)
{
    int n = 0;
    for (const auto &entry : gMorphologies)
    {
        if (samples && n < capacity)
        {
            const solr::Morphology &m = entry.second;
            samples[n] = {entry.first, m.branch, m.x, m.y, m.z, m.radius, m.parent, m.primitiveId};
        }
        ++n;
    }
    return n;
}

int SolR_SaveToFile(char *filename)
{
    solr::FileMarshaller fm;
    fm.saveToFile(*SingletonKernel::kernel(), filename ? filename : "");
    return (int)SingletonKernel::kernel()->getNbActivePrimitives();
}

int SolR_LoadFromFile(char *filename, double scale)
{
    solr::FileMarshaller fm;
    fm.loadFromFile(*SingletonKernel::kernel(), filename ? filename : "", solr::make_vec4f(0.f, 0.f, 0.f),
                    static_cast<float>(scale));
    return (int)SingletonKernel::kernel()->getNbActivePrimitives();
}

int SolRx_SetNbFrames(int nbFrames)
{
    SingletonKernel::kernel()->setNbFrames(nbFrames);
    return 0;
}

int SolRx_GetNbFrames()
{
    return SingletonKernel::kernel()->getNbFrames();
}

int SolRx_SetFrame(int frame)
{
    SingletonKernel::kernel()->setFrame(frame);
    return SingletonKernel::kernel()->getFrame();
}

int SolRx_MorphPrimitives()
{
    SingletonKernel::kernel()->morphPrimitives();
    return SingletonKernel::kernel()->getFrame();
}

/* Extension: the current frame blended anew from the first and the last key frame at any weight
 * (GPUKernel::morphFrame); with the HIP engine and an unchanged resident scene the blend runs on the device */
int SolRx_MorphFrame(double weight)
{
    return SingletonKernel::kernel()->morphFrame((float)weight);
}

/* Extension: the current frame blended anew from any two other frames at any weight (GPUKernel::morphBetween); with the
 * HIP engine and an unchanged resident scene the blend runs on the device, each key frame handed over once */
int SolRx_MorphBetween(int frameA, int frameB, double weight)
{
    if (frameA < 0 || frameB < 0)
        return -1;
    return SingletonKernel::kernel()->morphBetween((unsigned int)frameA, (unsigned int)frameB, (float)weight);
}

/* Extension: GPUKernel::setPrimitiveIsMovable (SolR_SetPrimitive makes a primitive movable again, as setPrimitive does) */
int SolRx_SetPrimitiveIsMovable(int index, int movable)
{
    SingletonKernel::kernel()->setPrimitiveIsMovable(index, movable != 0);
    return 0;
}

int SolRx_PendingMorph()
{
    return SingletonKernel::kernel()->pendingMorph() ? 1 : 0;
}

int SolRx_PendingRotations()
{
    return (int)SingletonKernel::kernel()->nbPendingRotations();
}

/* Extension: GPUKernel::translatePrimitives + compactBoxes(false), as the reference's scenes run it behind a rotation
 * (apps/scenes/Scene.cpp:1546-1548) */
int SolRx_TranslatePrimitives(double x, double y, double z)
{
    SingletonKernel::kernel()->translatePrimitives(solr::make_vec3f((float)x, (float)y, (float)z));
    SingletonKernel::kernel()->compactBoxes(false);
    return 0;
}

/* Extension: GPUKernel::setPrimitiveCenter + compactBoxes(false), the viewer's lamp drag (apps/solrViewer.cpp:1058-1069) */
int SolRx_SetPrimitiveCenter(int index, double x, double y, double z)
{
    SingletonKernel::kernel()->setPrimitiveCenter(index, solr::make_vec3f((float)x, (float)y, (float)z));
    SingletonKernel::kernel()->compactBoxes(false);
    return 0;
}

/* Extension: GPUKernel::setPrimitives + compactBoxes(false): a batch of primitives set anew, what a scene that animates its
 * own vertices does per frame (apps/scenes/animation/WaterScene.cpp doAnimate).  -1: an index is not in the store, nothing
 * changed */
int SolRx_SetPrimitives(const SolrPrimitiveEdit *edits, int n)
{
    const int status = SingletonKernel::kernel()->setPrimitives(edits, n);
    if (status == 0 && n > 0)
        SingletonKernel::kernel()->compactBoxes(false);
    return status;
}

/* Extension: GPUKernel::setPrimitiveMaterials + compactBoxes(false): a batch of primitives given another material, what a
 * scene that marks some of its primitives does per frame (apps/scenes/science/SwcScene.cpp doAnimate).  -1: an index is not
 * in the store, nothing changed */
int SolRx_SetPrimitiveMaterials(const int *indices, const int *materialIds, int n)
{
    const int status = SingletonKernel::kernel()->setPrimitiveMaterials(indices, materialIds, n);
    if (status == 0 && n > 0)
        SingletonKernel::kernel()->compactBoxes(false);
    return status;
}

int SolRx_SizeofPrimitiveEdit()
{
    return (int)sizeof(SolrPrimitiveEdit);
}

int SolRx_PendingMoves()
{
    return (int)SingletonKernel::kernel()->nbPendingMoves();
}

/* Extension: the frame bank (GPUKernel::setFrameBank) - an animation of whole meshes, one per frame, shown with
 * SolRx_SetFrame + SolR_CompactBoxes(false): the frames the engine has been given stay there, and a switch back uploads
 * nothing */
int SolRx_SetFrameBank(unsigned long long bytes)
{
    SingletonKernel::kernel()->setFrameBank(bytes);
    return engineStatus();
}

int SolRx_ParkedFrames()
{
    return (int)SingletonKernel::kernel()->nbParkedFrames();
}

int SolRx_FrameSwitches()
{
    return (int)SingletonKernel::kernel()->nbFrameSwitches();
}

int SolRx_SceneUploads()
{
    return (int)SingletonKernel::kernel()->nbSceneUploads();
}

/* Extension: material edits on the resident scene (GPUKernel::setMaterialEdits) - a host that sets a material per frame has
 * the engine follow it in place where it can, instead of the upload of the table that retags and lays out the whole scene */
int SolRx_SetMaterialEdits(int on)
{
    SingletonKernel::kernel()->setMaterialEdits(on != 0);
    return 0;
}

int SolRx_MaterialEdits()
{
    return (int)SingletonKernel::kernel()->materialEdits();
}

int SolRx_SyncHost()
{
    SingletonKernel::kernel()->syncHost();
    return 0;
}

int SolRx_GetMovable(const unsigned char **flags, int *nbPrimitives)
{
    const std::vector<unsigned char> &v = SingletonKernel::kernel()->hostMovable();
    *flags = v.data();
    *nbPrimitives = (int)v.size();
    return 0;
}

int SolR_SetPrimitiveMaterial(int index, int materialId)
{
    SingletonKernel::kernel()->setPrimitiveMaterial(index, materialId);
    return 0;
}

int SolR_GetPrimitiveMaterial(int index)
{
    return SingletonKernel::kernel()->getPrimitiveMaterial(index);
}

int SolR_SetPrimitiveNormals(int index, double n0_x, double n0_y, double n0_z, double n1_x, double n1_y, double n1_z,
                             double n2_x, double n2_y, double n2_z)
{
    SingletonKernel::kernel()->setPrimitiveNormals(index, solr::make_vec3f((float)n0_x, (float)n0_y, (float)n0_z),
                                                   solr::make_vec3f((float)n1_x, (float)n1_y, (float)n1_z),
                                                   solr::make_vec3f((float)n2_x, (float)n2_y, (float)n2_z));
    return 0;
}

int SolR_SetPrimitiveTextureCoordinates(int index, double t0_x, double t0_y, double t1_x, double t1_y, double t2_x,
                                        double t2_y)
{
    SingletonKernel::kernel()->setPrimitiveTextureCoordinates(index, solr::make_vec2f((float)t0_x, (float)t0_y),
                                                              solr::make_vec2f((float)t1_x, (float)t1_y),
                                                              solr::make_vec2f((float)t2_x, (float)t2_y));
    return 0;
}

int SolR_AddMaterial()
{
    return SingletonKernel::kernel()->addMaterial();
}

int SolR_SetMaterial(int index, double color_r, double color_g, double color_b, double noise, double reflection,
                     double refraction, int procedural, int wireframe, int wireframeDepth, double transparency,
                     double opacity, int diffuseTextureId, int normalTextureId, int bumpTextureId,
                     int specularTextureId, int reflectionTextureId, int transparencyTextureId,
                     int ambientOcclusionTextureId, double specValue, double specPower, double specCoef,
                     double innerIllumination, double illuminationDiffusion, double illuminationPropagation,
                     int fastTransparency)
{
    SingletonKernel::kernel()->setMaterial(
        index, (float)color_r, (float)color_g, (float)color_b, (float)noise, (float)reflection, (float)refraction,
        (procedural == 1), (wireframe == 1), wireframeDepth, (float)transparency, (float)opacity, diffuseTextureId,
        normalTextureId, bumpTextureId, specularTextureId, reflectionTextureId, transparencyTextureId,
        ambientOcclusionTextureId, (float)specValue, (float)specPower, (float)specCoef, (float)innerIllumination,
        (float)illuminationDiffusion, (float)illuminationPropagation, (fastTransparency == 1));
    return 0;
}

int SolR_CompactBoxes(bool update)
{
    return SingletonKernel::kernel()->compactBoxes(update);
}

int SolR_GetLight(int index)
{
    return SingletonKernel::kernel()->getLight(index);
}

int SolR_SetTexture(int index, const unsigned char *pixels, int width, int height, int depth, int textureType)
{
    if (!pixels || index < 0 || index >= NB_MAX_TEXTURES || width <= 0 || height <= 0 || depth <= 0)
        return -1;
    TextureInfo info;
    memset(&info, 0, sizeof(info));
    info.buffer = const_cast<unsigned char *>(pixels);
    info.size.x = width;
    info.size.y = height;
    info.size.z = depth;
    info.type = textureType;
    SingletonKernel::kernel()->setTexture(index, info);
    return 0;
}

int SolR_GetTextureSize(int index, int *width, int *height, int *depth)
{
    if (index < 0 || index >= NB_MAX_TEXTURES)
        return -1;
    TextureInfo &t = SingletonKernel::kernel()->getTextureInformation(index);
    *width = t.size.x;
    *height = t.size.y;
    *depth = t.size.z;
    return 0;
}

int SolR_LoadTextureFromFile(int index, char *filename)
{
    return SingletonKernel::kernel()->loadTextureFromFile(index, filename ? filename : "") ? 1 : 0;
}

int SolRx_GetTextureType(int index)
{
    if (index < 0 || index >= NB_MAX_TEXTURES)
        return -1;
    return SingletonKernel::kernel()->getTextureInformation(index).type;
}

int SolR_GetNbTextures(int *nbTextures)
{
    *nbTextures = SingletonKernel::kernel()->getNbActiveTextures();
    return 0;
}

int SolR_GetMaterial(int index, double *color_r, double *color_g, double *color_b, double *noise, double *reflection,
                     double *refraction, int *procedural, int *wireframe, int *wireframeDepth, double *transparency,
                     double *opacity, int *diffuseTextureId, int *normalTextureId, int *bumpTextureId,
                     int *specularTextureId, int *reflectionTextureId, int *transparencyTextureId,
                     int *ambientOcclusionTextureId, double *specValue, double *specPower, double *specCoef,
                     double *innerIllumination, double *illuminationDiffusion, double *illuminationPropagation,
                     int *fastTransparency)
{
    /* where GPUKernel::setMaterial put each attribute (GPUKernel.cpp:1780-1909 of the reference) */
    const Material *m = SingletonKernel::kernel()->getMaterial(index);
    if (!m)
        return -1;
    auto d = [](double *out, float v) { if (out) *out = static_cast<double>(v); };
    auto n = [](int *out, int v) { if (out) *out = v; };
    d(color_r, m->color.x), d(color_g, m->color.y), d(color_b, m->color.z);
    d(noise, m->innerIllumination.w);
    d(reflection, m->reflection), d(refraction, m->refraction);
    d(transparency, m->transparency), d(opacity, m->opacity);
    n(fastTransparency, m->attributes.x == 1), n(procedural, m->attributes.y == 1);
    n(wireframe, m->attributes.z == 1), n(wireframeDepth, m->attributes.w);
    n(diffuseTextureId, m->textureIds.x), n(normalTextureId, m->textureIds.y);
    n(bumpTextureId, m->textureIds.z), n(specularTextureId, m->textureIds.w);
    n(reflectionTextureId, m->advancedTextureIds.x), n(transparencyTextureId, m->advancedTextureIds.y);
    n(ambientOcclusionTextureId, m->advancedTextureIds.z);
    d(specValue, m->specular.x), d(specPower, m->specular.y), d(specCoef, m->specular.w);
    d(innerIllumination, m->innerIllumination.x), d(illuminationDiffusion, m->innerIllumination.y);
    d(illuminationPropagation, m->innerIllumination.z);
    return 0;
}

int SolR_GetTexture(int index, BitmapBuffer *image)
{
    if (index < 0 || index >= (int)SingletonKernel::kernel()->getNbActiveTextures() || !image)
        return 1;
    TextureInfo info;
    memset(&info, 0, sizeof(info));
    SingletonKernel::kernel()->getTexture(index, info);
    if (info.buffer && info.size.z >= 3)
    {
        const int len = info.size.x * info.size.y * info.size.z;
        for (int i = 0; i + 2 < len; i += info.size.z)
        {
            image[i] = info.buffer[i + 2];
            image[i + 1] = info.buffer[i + 1];
            image[i + 2] = info.buffer[i];
        }
    }
    return 0;
}

int SolR_RotatePrimitive(int, double, double, double, double, double, double)
{
    return 0;
}

int SolR_RecompileKernels(char *)
{
    return 0;
}

/* ---------------------------------------------------------------- extensions */

int SolRx_SelectEngine(const char *name)
{
    SingletonKernel::selectEngine(name);
    return 0;
}

int SolRx_HostBuild(int hostOnly)
{
    SingletonKernel::kernel()->setHostBuildOnly(hostOnly != 0);
    return 0;
}

int SolRx_SetDeterministic(long seed)
{
    SingletonKernel::kernel()->setDeterministic(seed);
    return 0;
}

int SolRx_LastError(char *buf, int len)
{
    std::string message;
    int code = SingletonKernel::kernel()->lastError(&message);
    if (buf && len > 0)
    {
        strncpy(buf, message.c_str(), len - 1);
        buf[len - 1] = 0;
    }
    return code;
}

int SolRx_GetBoxes(const BoundingBox **boxes, int *nbBoxes)
{
    const std::vector<BoundingBox> &v = SingletonKernel::kernel()->hostBoxes();
    *boxes = v.data();
    *nbBoxes = (int)SingletonKernel::kernel()->getNbActiveBoxes();
    return 0;
}

int SolRx_GetPrimitives(const Primitive **primitives, int *nbPrimitives)
{
    const std::vector<Primitive> &v = SingletonKernel::kernel()->hostPrimitives();
    *primitives = v.data();
    *nbPrimitives = (int)SingletonKernel::kernel()->getNbActivePrimitives();
    return 0;
}

int SolRx_GetLights(const LightInformation **lights, int *nbLights, int *nbLamps)
{
    *lights = SingletonKernel::kernel()->hostLights().data();
    *nbLights = SingletonKernel::kernel()->lightInformationSize();
    *nbLamps = (int)SingletonKernel::kernel()->getNbActiveLamps();
    return 0;
}

int SolRx_GetMaterials(const Material **materials, int *nbMaterials)
{
    SingletonKernel::kernel()->realignTexturesAndMaterials();
    *materials = SingletonKernel::kernel()->hostMaterials();
    *nbMaterials = (int)SingletonKernel::kernel()->getNbActiveMaterials() + 1;
    return 0;
}

int SolRx_GetRandoms(const float **randoms, int *nbRandoms)
{
    const std::vector<RandomBuffer> &v = SingletonKernel::kernel()->hostRandoms();
    *randoms = v.data();
    *nbRandoms = (int)v.size();
    return 0;
}

int SolRx_GetTextureAtlas(const unsigned char **atlas, long *nbBytes)
{
    const std::vector<BitmapBuffer> &v = SingletonKernel::kernel()->hostTextureAtlas();
    *atlas = v.empty() ? nullptr : v.data();
    *nbBytes = (long)v.size();
    return 0;
}

int SolRx_GetPrimitiveIds(const PrimitiveXYIdBuffer **ids, int *nbPixels)
{
    *ids = SingletonKernel::kernel()->hostPrimitiveIds();
    SceneInfo &si = SingletonKernel::kernel()->getSceneInfo();
    *nbPixels = si.size.x * si.size.y;
    return 0;
}

int SolRx_GetSceneInfo(SceneInfo *sceneInfo, PostProcessingInfo *postProcessingInfo, float eye[3], float dir[3],
                       float angles[4])
{
    solr::GPUKernel *k = SingletonKernel::kernel();
    if (sceneInfo)
        *sceneInfo = gSceneInfoStub;
    if (postProcessingInfo)
        *postProcessingInfo = gPostProcessingInfoStub;
    if (eye)
    {
        eye[0] = k->getViewPos().x; eye[1] = k->getViewPos().y; eye[2] = k->getViewPos().z;
    }
    if (dir)
    {
        dir[0] = k->getViewDir().x; dir[1] = k->getViewDir().y; dir[2] = k->getViewDir().z;
    }
    if (angles)
    {
        angles[0] = k->getViewAngles().x; angles[1] = k->getViewAngles().y;
        angles[2] = k->getViewAngles().z; angles[3] = k->getViewAngles().w;
    }
    return 0;
}

int SolRx_GetTreeDepth()
{
    return (int)SingletonKernel::kernel()->treeDepth();
}

int SolRx_GetPostProcessingBuffer(PostProcessingBuffer *buffer)
{
    if (!buffer)
        return -1;
    solr_hip_d2h_postprocessing(buffer);
    return engineStatus();
}

int SolRx_AddRectangle(double x, double y, double z, double w, double h, double d, int materialId)
{
    return SingletonKernel::kernel()->addRectangle((float)x, (float)y, (float)z, (float)w, (float)h, (float)d,
                                                   materialId);
}
}
