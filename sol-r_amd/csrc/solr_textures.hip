/*
 * solr_textures.hip - the pixel stage of the JPEG texture loader on the device (include/solr_hip.h,
 * solr_hip_jpeg_to_rgb): coefficient blocks, as the host's Huffman decoder leaves them, to the RGB bytes of the texture.
 * The arithmetic is jpeg_pixels.h - the reference decoder's (solr/images/jpgd.cpp), integer only, bit for bit - and this
 * file is only its lane mapping.  gfx950 only.
 *
 * One wave64 workgroup takes two neighbouring MCUs of an MCU row, so that every sampling keeps most lanes busy: 2 x 3, 2 x 4 or 2 x 12 inverse
 * DCTs of 8 lanes each, eight at a time.
 *   load      a lane takes one row of a block: 8 coefficients and 8 quantisers as one 16-byte load each, dequantised
 *             into LDS
 *   expand    2x2 files only, ahead of the inverse DCTs: the first pass of the frequency-domain upsampling with a lane
 *             per row of a chroma block (32 lanes), the second with a lane per coefficient of the 4x4 corner (4 chroma
 *             blocks x 16), which writes the four expanded blocks' coefficients - the rest of those blocks is zero
 *   rows      a lane owns one row of one of eight blocks and leaves its eight sums in LDS ...
 *   columns   ... where the lane that owns the column picks them up.  A row's 8 ints are 9 apart and a block's rows 72:
 *             ds_write_b32 / ds_read_b32 count banks modulo 32 within a 32-lane half (four blocks x eight lanes), and
 *             with these pitches both the write of element i of every row (banks 9 * line + 8 * block + i) and the
 *             read of row i of every column (banks 9 * i + line + 8 * block) touch 32 different banks; at 8 and 64
 *             the writes would meet eight deep and the reads four deep
 *   colour    a lane takes four neighbouring pixels of a row: 12 bytes, which sit together in the turned texture and
 *             leave as three dwords when the width is a multiple of four (the pixel pitch of 3 bytes then keeps every
 *             group dword-aligned), byte by byte otherwise; pixels beyond the width or height are dropped
 */
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>

#include "engine.h"
#include "jpeg_pixels.h"

namespace
{
constexpr int MCUS_PER_GROUP = 2;
constexpr int MAX_JOBS = MCUS_PER_GROUP * 12; /* inverse DCTs of a workgroup: 2x2 sampling */
constexpr int ROW_PITCH = 9, BLOCK_PITCH = 72; /* ints between two rows / two blocks of first-pass results, see above */

struct JpegGeometry
{
    int width, height, lumaH, lumaV, mcusPerRow;
};

__device__ inline void unpack8(const uint4 v, short out[8])
{
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    for (int i = 0; i < 4; ++i)
    {
        out[2 * i] = (short)(w[i] & 0xffffu);
        out[2 * i + 1] = (short)(w[i] >> 16);
    }
}

__global__ __launch_bounds__(64) void k_jpegPixels(const JpegGeometry geo, const unsigned short *__restrict__ quant,
                                                   const short *__restrict__ coefficients,
                                                   unsigned char *__restrict__ rgb)
{
    __shared__ __attribute__((aligned(16))) short blocks[MAX_JOBS][64];      /* what the inverse DCTs read */
    __shared__ __attribute__((aligned(16))) short chroma[MCUS_PER_GROUP * 2][64]; /* 2x2: dequantised Cb, Cr */
    __shared__ int folded[MCUS_PER_GROUP * 2][2][4][8];                       /* 2x2: jpgd's X0.. and X1.. */
    __shared__ int rows[8][BLOCK_PITCH];
    __shared__ unsigned char samples[MAX_JOBS][64];

    const int lane = threadIdx.x;
    const int lumaBlocks = geo.lumaH * geo.lumaV;
    const int perMcu = jpx::blocksPerMcu(geo.lumaH, geo.lumaV);
    const int jobsPerMcu = jpx::outputBlocksPerMcu(geo.lumaH, geo.lumaV);
    const bool expand = geo.lumaV == 2;
    /* the grid is (pairs of MCUs along a row, MCU rows): no lane ever divides by a number it was handed, which the
     * compiler would do in floating point */
    const int mcuRow = blockIdx.y, firstMcuX = blockIdx.x * MCUS_PER_GROUP;
    const long firstMcu = (long)mcuRow * geo.mcusPerRow + firstMcuX;

    /* ---- load and dequantise ------------------------------------------------------------------------------- */
    if (expand)
        for (int chunk = lane; chunk < MCUS_PER_GROUP * 8 * 8; chunk += 64)
        {
            /* the eight expanded blocks of either MCU: jobs 4..11 and 16..23 */
            const int job = (chunk / 64) * 12 + 4 + (chunk / 8) % 8;
            *reinterpret_cast<uint4 *>(&blocks[job][(chunk % 8) * 8]) = make_uint4(0u, 0u, 0u, 0u);
        }
    for (int row = lane; row < MCUS_PER_GROUP * perMcu * 8; row += 64)
    {
        const int local = row >= perMcu * 8 ? 1 : 0;
        const int b = (row - local * perMcu * 8) / 8, r = row % 8;
        const int c = b < lumaBlocks ? 0 : b - lumaBlocks + 1;
        const long mcu = firstMcu + local;
        short values[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (firstMcuX + local < geo.mcusPerRow)
        {
            short source[8], q[8];
            unpack8(*reinterpret_cast<const uint4 *>(coefficients + ((mcu * perMcu + b) * 64 + r * 8)), source);
            unpack8(*reinterpret_cast<const uint4 *>(quant + c * 64 + r * 8), q);
            for (int i = 0; i < 8; ++i)
                values[i] = jpx::dequantise(source[i], (unsigned short)q[i]);
        }
        short *to = (expand && c > 0) ? &chroma[local * 2 + c - 1][r * 8] : &blocks[local * jobsPerMcu + b][r * 8];
        for (int i = 0; i < 8; ++i)
            to[i] = values[i];
    }
    __syncthreads();

    /* ---- 2x2: the chroma blocks become four blocks each while still coefficients ----------------------------- */
    if (expand)
    {
        if (lane < MCUS_PER_GROUP * 2 * 8)
        {
            const int cb = lane / 8, r = lane % 8;
            int v[8];
            for (int c = 0; c < 8; ++c)
                v[c] = chroma[cb][r * 8 + c];
            for (int t = 0; t < 4; ++t)
                jpx::upsampleStep(t, v, &folded[cb][0][t][r], &folded[cb][1][t][r]);
        }
        __syncthreads();
        {
            const int cb = lane / 16, a = (lane / 4) % 4, j = lane % 4;
            int v0[8], v1[8], p, q, r, s;
            for (int i = 0; i < 8; ++i)
            {
                v0[i] = folded[cb][0][a][i];
                v1[i] = folded[cb][1][a][i];
            }
            jpx::upsampleStep(j, v0, &p, &q);
            jpx::upsampleStep(j, v1, &r, &s);
            short four[4];
            jpx::upsampleCombine(p, q, r, s, four);
            const int firstJob = (cb / 2) * 12 + 4 + (cb % 2) * 4;
            for (int k = 0; k < 4; ++k)
                blocks[firstJob + k][8 * j + a] = four[k];
        }
        __syncthreads();
    }

    /* ---- the inverse DCTs, eight blocks at a time -------------------------------------------------------------- */
    const int nbJobs = MCUS_PER_GROUP * jobsPerMcu;
    for (int first = 0; first < nbJobs; first += 8)
    {
        const int slot = lane / 8, line = lane % 8, job = first + slot;
        if (job < nbJobs)
        {
            int out[8];
            jpx::idctRow(&blocks[job][line * 8], out);
            for (int i = 0; i < 8; ++i)
                rows[slot][line * ROW_PITCH + i] = out[i];
        }
        __syncthreads();
        if (job < nbJobs)
        {
            int column[8];
            unsigned char out[8];
            for (int i = 0; i < 8; ++i)
                column[i] = rows[slot][i * ROW_PITCH + line];
            jpx::idctColumn(column, out);
            for (int i = 0; i < 8; ++i)
                samples[job][i * 8 + line] = out[i];
        }
        __syncthreads();
    }

    /* ---- colour, four pixels of a row a lane ---------------------------------------------------------------------- */
    const int mcuWidth = 8 * geo.lumaH, mcuHeight = 8 * geo.lumaV;
    /* 2 or 4 groups in a row of an MCU, 16, 32 or 64 in an MCU: powers of two, taken apart with shifts */
    const int rowShift = geo.lumaH, mcuShift = geo.lumaH + geo.lumaV + 2;
    const bool dwords = (geo.width & 3) == 0;
    for (int group = lane; group < (MCUS_PER_GROUP << mcuShift); group += 64)
    {
        const int local = group >> mcuShift, within = group & ((1 << mcuShift) - 1);
        const int y = within >> rowShift, x0 = (within & ((1 << rowShift) - 1)) * 4;
        if (firstMcuX + local >= geo.mcusPerRow)
            continue;
        const int py = mcuRow * mcuHeight + y;
        const int px0 = (firstMcuX + local) * mcuWidth + x0;
        if (py >= geo.height || px0 >= geo.width)
            continue;
        const unsigned char *from = samples[local * jobsPerMcu];
        /* the turned texture runs backwards: pixel px0 + 3 comes first in memory */
        unsigned char bytes[12];
        for (int i = 0; i < 4; ++i)
        {
            int offY, offCb, offCr;
            jpx::sampleOffsets(geo.lumaH, geo.lumaV, x0 + 3 - i, y, &offY, &offCb, &offCr);
            jpx::colour(from[offY], from[offCb], from[offCr], &bytes[3 * i]);
        }
        if (dwords)
        {
            unsigned *to = reinterpret_cast<unsigned *>(rgb + 3 * jpx::turnedPixel(geo.width, geo.height, px0 + 3, py));
            for (int w = 0; w < 3; ++w)
                to[w] = bytes[4 * w] | (bytes[4 * w + 1] << 8) | (bytes[4 * w + 2] << 16) |
                        ((unsigned)bytes[4 * w + 3] << 24);
        }
        else
            for (int i = 0; i < 4; ++i)
                if (px0 + 3 - i < geo.width)
                {
                    unsigned char *to = rgb + 3 * jpx::turnedPixel(geo.width, geo.height, px0 + 3 - i, py);
                    to[0] = bytes[3 * i];
                    to[1] = bytes[3 * i + 1];
                    to[2] = bytes[3 * i + 2];
                }
    }
}

std::atomic<unsigned long long> gJpegBlocks{0};

inline size_t roundUp(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
}

extern "C" {

int solr_hip_jpeg_to_rgb(const SolrJpegFrame *frame, const short *coefficients, long nbBlocks, unsigned char *rgb)
{
    using namespace solreng;
    if (!ok())
        return -1;
    /* ---- arguments: nothing is launched for a call that fails here ---- */
    if (!frame || !coefficients || !rgb)
    {
        setError(-1, "solr_hip_jpeg_to_rgb: null frame, coefficients or rgb", __FILE__, __LINE__);
        return -1;
    }
    if (!jpx::samplingSupported(frame->lumaH, frame->lumaV))
    {
        setError(-1, "solr_hip_jpeg_to_rgb: luma sampling must be 1x1, 2x1 or 2x2", __FILE__, __LINE__);
        return -1;
    }
    if (frame->width < 1 || frame->height < 1 || frame->width > SOLR_JPEG_MAX_SIDE || frame->height > SOLR_JPEG_MAX_SIDE ||
        (long)frame->width * frame->height > SOLR_JPEG_MAX_PIXELS)
    {
        setError(-1, "solr_hip_jpeg_to_rgb: image size out of range", __FILE__, __LINE__);
        return -1;
    }
    const int perMcu = jpx::blocksPerMcu(frame->lumaH, frame->lumaV);
    const int mcusPerRow = (frame->width + 8 * frame->lumaH - 1) / (8 * frame->lumaH);
    const int mcuRows = (frame->height + 8 * frame->lumaV - 1) / (8 * frame->lumaV);
    const long nbMcus = (long)mcusPerRow * mcuRows;
    if (frame->mcusPerRow != mcusPerRow || frame->mcuRows != mcuRows || nbBlocks != nbMcus * perMcu)
    {
        setError(-1, "solr_hip_jpeg_to_rgb: the MCU grid or nbBlocks does not match the image size and sampling", __FILE__,
                 __LINE__);
        return -1;
    }

    /* on the engine's device whichever thread calls; the caller's current device is restored on the way out */
    int before = -1;
    if (hipGetDevice(&before) != hipSuccess)
        before = -1;
    HIPCHECK(hipSetDevice(solr_hip_get_device()));

    const size_t quantBytes = roundUp(sizeof(frame->quant));
    const size_t coefficientBytes = roundUp((size_t)nbBlocks * 64 * sizeof(short));
    const size_t rgbBytes = (size_t)frame->width * frame->height * 3;
    unsigned char *device = nullptr;
    hipStream_t stream = nullptr;
    if (ok())
        HIPCHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    if (ok())
        HIPCHECK(hipMalloc((void **)&device, quantBytes + coefficientBytes + roundUp(rgbBytes)));
    if (ok())
    {
        unsigned short *dQuant = reinterpret_cast<unsigned short *>(device);
        short *dCoefficients = reinterpret_cast<short *>(device + quantBytes);
        unsigned char *dRgb = device + quantBytes + coefficientBytes;
        HIPCHECK(hipMemcpyAsync(dQuant, frame->quant, sizeof(frame->quant), hipMemcpyHostToDevice, stream));
        HIPCHECK(hipMemcpyAsync(dCoefficients, coefficients, (size_t)nbBlocks * 64 * sizeof(short), hipMemcpyHostToDevice,
                                stream));
        if (ok())
        {
            const JpegGeometry geo = {frame->width, frame->height, frame->lumaH, frame->lumaV, mcusPerRow};
            const dim3 grid((unsigned)((mcusPerRow + MCUS_PER_GROUP - 1) / MCUS_PER_GROUP), (unsigned)mcuRows);
            k_jpegPixels<<<grid, dim3(64), 0, stream>>>(geo, dQuant, dCoefficients, dRgb);
            HIPCHECK(hipGetLastError());
        }
        if (ok())
            HIPCHECK(hipMemcpyAsync(rgb, dRgb, rgbBytes, hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        if (ok())
            gJpegBlocks += (unsigned long long)nbMcus * jpx::outputBlocksPerMcu(frame->lumaH, frame->lumaV);
    }
    if (device)
        (void)hipFree(device);
    if (stream)
        (void)hipStreamDestroy(stream);
    if (before >= 0)
        (void)hipSetDevice(before);
    return ok() ? 0 : -1;
}

unsigned long long solr_hip_jpeg_blocks(void)
{
    return gJpegBlocks.load();
}

} /* extern "C" */
