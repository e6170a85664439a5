/*
 * solr_jpeg_encode.hip - the pixel stage of the JPEG screenshot writer on the device (include/solr_hip.h,
 * solr_hip_rgb_to_jpeg_blocks): the RGB bytes of a frame to quantised coefficient blocks in zigzag order, which the host's
 * Huffman coder (host/JpegWriter.cpp) turns into the file.  The arithmetic is jpeg_encode.h - the reference encoder's
 * (solr/images/jpge.cpp), integer only, bit for bit - and this file is only its lane mapping.  gfx950 only.
 *
 * One wave64 workgroup takes two neighbouring MCUs of an MCU row, as k_jpegPixels does: 2 x 3, 2 x 4 or 2 x 6 forward DCTs
 * of 8 lanes each, eight at a time.
 *   convert   a lane takes pixels of the two MCUs in turn: three bytes read through the screenshot's pixel order
 *             (jpe::sample: turned, red and blue swapped, coordinates clamped to the picture - the edge rule), Y, Cb, Cr
 *             into LDS.  An MCU is 8 or 16 pixels wide and high, so a lane finds its pixel with shifts
 *   rows      a lane owns one row of one of eight blocks: the block load (sample - 128, or the chroma average), the first
 *             pass, and its eight results into LDS ...
 *   columns   ... where the lane that owns the column picks them up, runs the second pass and puts the coefficients back
 *             in the places it read (nobody else touches a column).  A row's 8 ints are 9 apart and a block's rows 72, the
 *             pitches of k_jpegPixels: both the write of element i of every row and the read of row i of every column
 *             touch 32 different banks within a 32-lane half
 *   quantise  a lane takes eight consecutive zigzag positions of its block: eight quantisers and reciprocals as 16-byte
 *             loads, eight coefficients gathered from LDS, eight shorts out as one 16-byte store
 * The grid runs over (pairs of MCUs along a row, MCU rows): no lane divides by a number it was handed.
 */
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>

#include "engine.h"
#include "jpeg_device.h"
#include "jpeg_encode.h"

namespace
{
constexpr int MCUS_PER_GROUP = 2;
constexpr int ROW_PITCH = 9, BLOCK_PITCH = 72; /* ints between two rows / two blocks of first-pass results, see above */
constexpr int MCU_BYTES = 16 * 16 * 3;

struct JpegEncodeGeometry
{
    int width, height, lumaH, lumaV, turned, swapRedBlue, mcusPerRow;
};

using solreng::JpegEncodeTables;

__global__ __launch_bounds__(64) void k_jpegCoefficients(const JpegEncodeGeometry geo,
                                                         const JpegEncodeTables *__restrict__ tables,
                                                         const unsigned char *__restrict__ rgb,
                                                         short *__restrict__ coefficients)
{
    __shared__ unsigned char ycc[MCUS_PER_GROUP][MCU_BYTES];
    __shared__ int rows[8][BLOCK_PITCH];

    const int lane = threadIdx.x;
    const int lumaBlocks = geo.lumaH * geo.lumaV;
    const int perMcu = jpe::blocksPerMcu(geo.lumaH, geo.lumaV);
    const int mcuRow = blockIdx.y, firstMcuX = blockIdx.x * MCUS_PER_GROUP;
    const long firstMcu = (long)mcuRow * geo.mcusPerRow + firstMcuX;

    /* ---- convert ----------------------------------------------------------------------------------------------- */
    /* 8 or 16 pixels in a row of an MCU, 64, 128 or 256 in an MCU: powers of two, taken apart with shifts */
    const int rowShift = geo.lumaH + 2, mcuShift = geo.lumaH + geo.lumaV + 4;
    for (int pixel = lane; pixel < (MCUS_PER_GROUP << mcuShift); pixel += 64)
    {
        const int local = pixel >> mcuShift, within = pixel & ((1 << mcuShift) - 1);
        if (firstMcuX + local >= geo.mcusPerRow)
            continue;
        const int y = within >> rowShift, x = within & ((1 << rowShift) - 1);
        jpe::sample(rgb, geo.width, geo.height, geo.turned, geo.swapRedBlue, ((firstMcuX + local) << rowShift) + x,
                    (mcuRow << (geo.lumaV + 2)) + y, &ycc[local][within * 3]);
    }
    __syncthreads();

    /* ---- the forward DCTs, eight blocks at a time ---------------------------------------------------------------- */
    const int nbJobs = MCUS_PER_GROUP * perMcu;
    for (int first = 0; first < nbJobs; first += 8)
    {
        const int slot = lane >> 3, line = lane & 7, job = first + slot;
        const int local = job >= perMcu ? 1 : 0, block = job - local * perMcu;
        const bool live = job < nbJobs && firstMcuX + local < geo.mcusPerRow;
        if (live)
        {
            int v[8];
            jpe::blockRow(ycc[local], geo.lumaH, geo.lumaV, block, line, v);
            jpe::dctRow(v);
            for (int i = 0; i < 8; ++i)
                rows[slot][line * ROW_PITCH + i] = v[i];
        }
        __syncthreads();
        if (live)
        {
            int v[8];
            for (int i = 0; i < 8; ++i)
                v[i] = rows[slot][i * ROW_PITCH + line];
            jpe::dctColumn(v);
            for (int i = 0; i < 8; ++i)
                rows[slot][i * ROW_PITCH + line] = v[i];
        }
        __syncthreads();
        if (live)
        {
            const int table = block < lumaBlocks ? 0 : 1;
            const uint4 q = *reinterpret_cast<const uint4 *>(&tables->quant[table][line * 8]);
            const uint4 m0 = *reinterpret_cast<const uint4 *>(&tables->recip[table][line * 8]);
            const uint4 m1 = *reinterpret_cast<const uint4 *>(&tables->recip[table][line * 8 + 4]);
            const unsigned qs[4] = {q.x, q.y, q.z, q.w};
            const unsigned ms[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
            unsigned packed[4];
            for (int i = 0; i < 8; ++i)
            {
                const int natural = jpe::zigzag(line * 8 + i);
                const int value = rows[slot][(natural >> 3) * ROW_PITCH + (natural & 7)];
                const int quantiser = (int)((qs[i >> 1] >> ((i & 1) * 16)) & 0xffffu);
                const unsigned out = (unsigned short)jpe::quantise(value, quantiser, ms[i]);
                packed[i >> 1] = (i & 1) ? (packed[i >> 1] | (out << 16)) : out;
            }
            short *to = coefficients + (((firstMcu + local) * perMcu + block) * 64 + line * 8);
            *reinterpret_cast<uint4 *>(to) = make_uint4(packed[0], packed[1], packed[2], packed[3]);
        }
        __syncthreads();
    }
}

/* the tables as an argument to their place on the device: what a launch carries needs no host memory that outlives the
 * call (launchJpegCoefficientsResident; 768 bytes, 192 words) */
static_assert(sizeof(JpegEncodeTables) == 192 * sizeof(unsigned), "three words a lane");
__global__ __launch_bounds__(64) void k_jpegPutTables(const JpegEncodeTables tables, JpegEncodeTables *__restrict__ to)
{
    const unsigned *from = reinterpret_cast<const unsigned *>(&tables);
    for (int i = threadIdx.x; i < 192; i += 64)
        reinterpret_cast<unsigned *>(to)[i] = from[i];
}

std::atomic<unsigned long long> gEncodedBlocks{0};

inline size_t roundUp(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
}

namespace solreng
{
bool jpegSourceAccepted(const char *who, const SolrJpegSource *source, long *nbBlocks)
{
    const std::string name(who);
    if (!jpe::samplingSupported(source->lumaH, source->lumaV))
    {
        setError(-1, (name + ": luma sampling must be 1x1, 2x1 or 2x2").c_str(), __FILE__, __LINE__);
        return false;
    }
    if (source->width < 1 || source->height < 1 || source->width > SOLR_JPEG_MAX_SIDE ||
        source->height > SOLR_JPEG_MAX_SIDE || (long)source->width * source->height > SOLR_JPEG_MAX_PIXELS)
    {
        setError(-1, (name + ": image size out of range").c_str(), __FILE__, __LINE__);
        return false;
    }
    if (source->quality < 1 || source->quality > 100)
    {
        setError(-1, (name + ": the JPEG quality must be 1 ... 100").c_str(), __FILE__, __LINE__);
        return false;
    }
    const int mcusPerRow = (source->width + 8 * source->lumaH - 1) / (8 * source->lumaH);
    const int mcuRows = (source->height + 8 * source->lumaV - 1) / (8 * source->lumaV);
    *nbBlocks = (long)mcusPerRow * mcuRows * jpe::blocksPerMcu(source->lumaH, source->lumaV);
    return true;
}

void launchJpegCoefficients(const SolrJpegSource &source, JpegEncodeTables &tables, JpegEncodeTables *dTables,
                            const unsigned char *dRgb, short *dCoefficients, long nbBlocks, hipStream_t stream)
{
    for (int t = 0; t < 2; ++t)
    {
        jpe::quantTable(source.quality, t, tables.quant[t]);
        for (int k = 0; k < 64; ++k)
            tables.recip[t][k] = jpe::reciprocal(tables.quant[t][k]);
    }
    const int mcusPerRow = (source.width + 8 * source.lumaH - 1) / (8 * source.lumaH);
    const int mcuRows = (source.height + 8 * source.lumaV - 1) / (8 * source.lumaV);
    HIPCHECK(hipMemcpyAsync(dTables, &tables, sizeof(tables), hipMemcpyHostToDevice, stream));
    if (!ok())
        return;
    const JpegEncodeGeometry geo = {source.width,       source.height,           source.lumaH, source.lumaV,
                                    source.turned != 0, source.swapRedBlue != 0, mcusPerRow};
    const dim3 grid((unsigned)((mcusPerRow + MCUS_PER_GROUP - 1) / MCUS_PER_GROUP), (unsigned)mcuRows);
    k_jpegCoefficients<<<grid, dim3(64), 0, stream>>>(geo, dTables, dRgb, dCoefficients);
    HIPCHECK(hipGetLastError());
}

void launchJpegCoefficientsResident(const SolrJpegSource &source, JpegEncodeTables *dTables, const unsigned char *dRgb,
                                    short *dCoefficients, long nbBlocks, hipStream_t stream)
{
    JpegEncodeTables tables;
    for (int t = 0; t < 2; ++t)
    {
        jpe::quantTable(source.quality, t, tables.quant[t]);
        for (int k = 0; k < 64; ++k)
            tables.recip[t][k] = jpe::reciprocal(tables.quant[t][k]);
    }
    const int mcusPerRow = (source.width + 8 * source.lumaH - 1) / (8 * source.lumaH);
    const int mcuRows = (source.height + 8 * source.lumaV - 1) / (8 * source.lumaV);
    k_jpegPutTables<<<dim3(1), dim3(64), 0, stream>>>(tables, dTables);
    HIPCHECK(hipGetLastError());
    if (!ok())
        return;
    const JpegEncodeGeometry geo = {source.width,       source.height,           source.lumaH, source.lumaV,
                                    source.turned != 0, source.swapRedBlue != 0, mcusPerRow};
    const dim3 grid((unsigned)((mcusPerRow + MCUS_PER_GROUP - 1) / MCUS_PER_GROUP), (unsigned)mcuRows);
    k_jpegCoefficients<<<grid, dim3(64), 0, stream>>>(geo, dTables, dRgb, dCoefficients);
    HIPCHECK(hipGetLastError());
}

void countJpegEncodedBlocks(long nbBlocks)
{
    gEncodedBlocks += (unsigned long long)nbBlocks;
}
}

extern "C" {

int solr_hip_rgb_to_jpeg_blocks(const SolrJpegSource *source, const unsigned char *rgb, short *coefficients,
                                long nbBlocks)
{
    using namespace solreng;
    if (!ok())
        return -1;
    /* ---- arguments: nothing is launched for a call that fails here ---- */
    if (!source || !rgb || !coefficients)
    {
        setError(-1, "solr_hip_rgb_to_jpeg_blocks: null source, rgb or coefficients", __FILE__, __LINE__);
        return -1;
    }
    long expected = 0;
    if (!jpegSourceAccepted("solr_hip_rgb_to_jpeg_blocks", source, &expected))
        return -1;
    if (nbBlocks != expected)
    {
        setError(-1, "solr_hip_rgb_to_jpeg_blocks: nbBlocks does not match the image size and sampling", __FILE__,
                 __LINE__);
        return -1;
    }
    JpegEncodeTables tables;

    /* on the engine's device whichever thread calls; the caller's current device is restored on the way out */
    int before = -1;
    if (hipGetDevice(&before) != hipSuccess)
        before = -1;
    HIPCHECK(hipSetDevice(solr_hip_get_device()));

    const size_t tableBytes = roundUp(sizeof(tables));
    const size_t rgbBytes = (size_t)source->width * source->height * 3;
    const size_t coefficientBytes = (size_t)nbBlocks * 64 * sizeof(short);
    unsigned char *device = nullptr;
    hipStream_t stream = nullptr;
    if (ok())
        HIPCHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    if (ok())
        HIPCHECK(hipMalloc((void **)&device, tableBytes + roundUp(coefficientBytes) + roundUp(rgbBytes)));
    if (ok())
    {
        JpegEncodeTables *dTables = reinterpret_cast<JpegEncodeTables *>(device);
        short *dCoefficients = reinterpret_cast<short *>(device + tableBytes);
        unsigned char *dRgb = device + tableBytes + roundUp(coefficientBytes);
        HIPCHECK(hipMemcpyAsync(dRgb, rgb, rgbBytes, hipMemcpyHostToDevice, stream));
        if (ok())
            launchJpegCoefficients(*source, tables, dTables, dRgb, dCoefficients, nbBlocks, stream);
        if (ok())
            HIPCHECK(hipMemcpyAsync(coefficients, dCoefficients, coefficientBytes, hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        if (ok())
            countJpegEncodedBlocks(nbBlocks);
    }
    if (device)
        (void)hipFree(device);
    if (stream)
        (void)hipStreamDestroy(stream);
    if (before >= 0)
        (void)hipSetDevice(before);
    return ok() ? 0 : -1;
}

unsigned long long solr_hip_jpeg_encoded_blocks(void)
{
    return gEncodedBlocks.load();
}

} /* extern "C" */
