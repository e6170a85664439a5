/*
 * solr_jpeg_entropy.hip - the entropy stage of the JPEG writer on the device (include/solr_hip.h,
 * solr_hip_jpeg_blocks_to_scan, solr_hip_rgb_to_jpeg_scan, solr_hip_frame_to_jpeg_scan): quantised coefficient blocks to
 * the entropy-coded segment of a baseline file, the bytes of the one-pass coder (host/JpegWriter.cpp, the reference's
 * solr/images/jpge.cpp).  The arithmetic is jpeg_entropy.h, and this file is only its lane mapping.  gfx950 only.
 *
 *   k_jpegBlockBits   a lane per block: the walk of jpn::blockBits, the count as a 64-bit item; a block outside the tables'
 *                     domain raises the flag word
 *   (scan)            hipcub::DeviceScan::ExclusiveSum over n + 1 items - the scan solr_iso.hip uses, with 64-bit items: the
 *                     bit offset of every block and, as item n, the total
 *   k_jpegEmit        a wave64 workgroup per jpn::BLOCKS_PER_GROUP consecutive blocks, a lane per block: the same walk, the
 *                     bits ORed (LDS atomics - neighbouring lanes share words) into the group's piece of the stream in LDS.
 *                     The piece then goes out word by word: the words strictly inside it are all this group's and leave as
 *                     plain stores, the first and the last may be shared with the groups on either side and are ORed into
 *                     the zeroed stream with a vector atomic.  OR commutes: the stream does not depend on who comes first.
 *                     The lane of the last block also puts the tail's one-bits
 *   k_jpegCountFF     a workgroup per jpn::STUFF_CHUNK_BYTES bytes of the unstuffed stream, a lane per word: the 0xFF bytes
 *                     of the chunk, summed across the wave
 *   (scan)            the same scan over the chunks: the 0xFF bytes before each, and their total
 *   k_jpegStuff       the same mapping: a lane's word goes to the chunk's offset plus the 0xFF before the chunk plus the
 *                     0xFF of the lanes below it (a scan across the wave), a zero behind every 0xFF
 * With optimised tables (the solr_hip_*_to_jpeg_scan_optimised entries; jpge's two-pass mode) two kernels go in front, and
 * k_jpegBlockBits and k_jpegEmit run in a second instantiation whose tables are an LDS copy of what the second one made:
 *   k_jpegSymbolCounts    the same mapping as k_jpegBlockBits: the walk of jpn::blockCensus into a histogram of the group in
 *                     LDS (LDS atomics: lanes meet on the frequent symbols), whose non-zero counters are then added to the
 *                     histogram in device memory
 *   k_jpegOptimiseTables  a wave64 workgroup per table: every lane ranks its symbols among the (count, index) pairs
 *                     (jpn::symbolRank, at most 256 comparisons each), one lane runs the three serial passes of the length
 *                     computation and the 16-bit limit over LDS (jpn::bitsOfSorted), and all lanes write bits, values and
 *                     the code | length << 16 entries.  No host round trip sits between census and coding: bits and values
 *                     come to the host with the total and the flag
 * A block's coefficients are read once per walk from LDS, where the group's blocks are staged with coalesced loads, a block
 * 33 words apart: the lanes of a 32-lane half then read 32 different banks.  The predecessor's DC (jpn::predecessor) is one
 * global load.  Nothing is indexed by a run-time value in registers: no scratch.
 */
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <atomic>
#include <cstddef>
#include <cstring>
#include <string>

#include "engine.h"
#include "jpeg_device.h"
#include "jpeg_encode.h"
#include "jpeg_entropy.h"
#include "../../include/solr_hip_probes_jpeg.h"

namespace
{
using jpn::u32;
using jpn::u64;
using jpn::u8;

constexpr int GROUP = 64;
static_assert(jpn::BLOCKS_PER_GROUP == GROUP, "a lane per block");
static_assert(jpn::STUFF_CHUNK_BYTES == GROUP * 4, "a lane per word of a chunk");
constexpr int STAGE_PITCH = 33; /* words between two staged blocks of 32 words, see above */
/* the words a group's piece can touch: its bits, the tail's (at most 7), and a start anywhere in a word.  DATA: the
 * tables came as data and a block is bounded by what any table of 16-bit codes allows, not by the standard ones */
template <bool DATA>
constexpr u32 GROUP_BITS = (u32)jpn::BLOCKS_PER_GROUP * (DATA ? jpn::MAX_BLOCK_BITS_ANY_TABLE : jpn::MAX_BLOCK_BITS) + 7u;
template <bool DATA>
constexpr int GROUP_WORDS = (int)((GROUP_BITS<DATA> + 31u + 31u) / 32u);
static_assert(GROUP_BITS<false> == 64u * 1660u + 7u && GROUP_BITS<true> == 64u * 1665u + 7u, "the two bounds");
static_assert((GROUP * 33 + GROUP_WORDS<true>) * sizeof(u32) + sizeof(jpn::Tables) <= 64u * 1024u, "k_jpegEmit's LDS");

/* the tables of an instantiation: the standard ones, or the group's LDS copy of the device's (2 144 bytes; every lane
 * takes part, and a barrier must follow before the walk - stageBlocks ends in one) */
template <bool DATA>
__device__ inline const jpn::Tables &groupTables(u32 *own, const jpn::Tables *__restrict__ device)
{
    if constexpr (DATA)
    {
        const u32 *from = reinterpret_cast<const u32 *>(device);
        for (int i = threadIdx.x; i < jpn::CENSUS_COUNTERS; i += GROUP)
            own[i] = from[i];
        return *reinterpret_cast<const jpn::Tables *>(own);
    }
    else
        return jpn::tables();
}

/* the group's blocks from `coefficients` (block `first` on, `count` of them) into `staged`, STAGE_PITCH words apart */
__device__ inline void stageBlocks(const short *__restrict__ coefficients, long first, int count, u32 *staged)
{
    const u32 *from = reinterpret_cast<const u32 *>(coefficients + first * 64);
    for (int i = threadIdx.x; i < count * 32; i += GROUP)
        staged[(i >> 5) * STAGE_PITCH + (i & 31)] = from[i];
    __syncthreads();
}

__device__ inline int previousDc(const short *__restrict__ coefficients, long index, int lumaBlocks)
{
    const long before = jpn::predecessor(index, lumaBlocks);
    return before < 0 ? 0 : (int)coefficients[before * 64];
}

template <bool DATA>
__global__ __launch_bounds__(GROUP) void k_jpegBlockBits(const short *__restrict__ coefficients, const int nbBlocks,
                                                         const int lumaBlocks, u64 *__restrict__ bits,
                                                         u32 *__restrict__ flag, const jpn::Tables *__restrict__ dTables)
{
    __shared__ u32 staged[GROUP * STAGE_PITCH];
    __shared__ u32 own[DATA ? jpn::CENSUS_COUNTERS : 1];
    const jpn::Tables &t = groupTables<DATA>(own, dTables);
    const long first = (long)blockIdx.x * GROUP;
    const int count = nbBlocks - first < GROUP ? (int)(nbBlocks - first) : GROUP;
    stageBlocks(coefficients, first, count, staged);
    const int lane = threadIdx.x;
    if (blockIdx.x == 0 && lane == 0)
        bits[nbBlocks] = 0; /* item n of the scan: its result is the total */
    if (lane >= count)
        return;
    const long index = first + lane;
    u32 n = 0;
    const bool inside = jpn::blockBits(t, reinterpret_cast<const short *>(staged + lane * STAGE_PITCH),
                                       previousDc(coefficients, index, lumaBlocks), jpn::chromaOf(index, lumaBlocks), &n);
    bits[index] = n;
    if (!inside)
        atomicOr(flag, 1u);
}

/* jpn::WordWriter on words that other lanes write too */
struct SharedWriter
{
    u32 *words;
    u32 at;
    __device__ void put(u32 bits, int n)
    {
        u64 word;
        u32 first, second;
        jpn::placeBits(at, bits, n, &word, &first, &second);
        atomicOr(&words[word], first);
        if (second)
            atomicOr(&words[word + 1], second);
        at += (u32)n;
    }
};

template <bool DATA>
__global__ __launch_bounds__(GROUP) void k_jpegEmit(const short *__restrict__ coefficients, const int nbBlocks,
                                                    const int lumaBlocks, const u64 *__restrict__ offsets,
                                                    u32 *__restrict__ stream, const jpn::Tables *__restrict__ dTables)
{
    __shared__ u32 staged[GROUP * STAGE_PITCH];
    __shared__ u32 piece[GROUP_WORDS<DATA>];
    __shared__ u32 own[DATA ? jpn::CENSUS_COUNTERS : 1];
    const int lane = threadIdx.x;
    const long first = (long)blockIdx.x * GROUP;
    const int count = nbBlocks - first < GROUP ? (int)(nbBlocks - first) : GROUP;
    const bool last = first + count == nbBlocks;
    const u64 from = offsets[first];
    u64 to = offsets[first + count];
    if (last)
        to += (u64)jpn::tailBits(to);
    /* (what k_jpegBlockBits counted cannot be more: the guard is against offsets that are not its scan) */
    if (to <= from || to - from > GROUP_BITS<DATA>)
        return;
    const jpn::Tables &t = groupTables<DATA>(own, dTables);
    const u64 firstWord = from >> 5;
    const int nbWords = (int)(((to - 1) >> 5) - firstWord) + 1;
    for (int w = lane; w < nbWords; w += GROUP)
        piece[w] = 0;
    stageBlocks(coefficients, first, count, staged); /* (ends in a barrier) */
    if (lane < count)
    {
        const long index = first + lane;
        SharedWriter writer = {piece, (u32)(offsets[index] - (firstWord << 5))};
        jpn::walkBlock(t, reinterpret_cast<const short *>(staged + lane * STAGE_PITCH),
                       previousDc(coefficients, index, lumaBlocks), jpn::chromaOf(index, lumaBlocks), writer);
        if (index == nbBlocks - 1)
            if (const int tail = jpn::tailBits(offsets[nbBlocks]))
                writer.put((1u << tail) - 1u, tail);
    }
    __syncthreads();
    for (int w = lane; w < nbWords; w += GROUP)
    {
        const u32 value = piece[w];
        if (w == 0 || w == nbWords - 1)
            atomicOr(&stream[firstWord + w], value);
        else
            stream[firstWord + w] = value;
    }
}

/* the sum of `value` over the wave, in every lane */
__device__ inline u32 waveSum(u32 value)
{
    for (int step = 1; step < GROUP; step <<= 1)
        value += __shfl_xor(value, step, GROUP);
    return value;
}

/* ---- optimised tables ---- */
/* jpn::Counter on counters that other lanes count in too: the group's histogram in LDS, laid out as jpn::Census */
static_assert(offsetof(jpn::Census, dc) == 0 && offsetof(jpn::Census, ac) == 2 * 12 * sizeof(u32), "dc[2][12], ac[2][256]");
struct SharedCounter
{
    u32 *counts;
    int chroma;
    __device__ void dc(int size, int) { atomicAdd(&counts[chroma * 12 + size], 1u); }
    __device__ void ac(int symbol, int, int) { atomicAdd(&counts[24 + chroma * 256 + symbol], 1u); }
};

__global__ __launch_bounds__(GROUP) void k_jpegSymbolCounts(const short *__restrict__ coefficients, const int nbBlocks,
                                                            const int lumaBlocks, u32 *__restrict__ histogram,
                                                            u32 *__restrict__ flag)
{
    __shared__ u32 staged[GROUP * STAGE_PITCH];
    __shared__ u32 counts[jpn::CENSUS_COUNTERS];
    const int lane = threadIdx.x;
    const long first = (long)blockIdx.x * GROUP;
    const int count = nbBlocks - first < GROUP ? (int)(nbBlocks - first) : GROUP;
    for (int i = lane; i < jpn::CENSUS_COUNTERS; i += GROUP)
        counts[i] = 0;
    stageBlocks(coefficients, first, count, staged); /* (ends in a barrier) */
    if (lane < count)
    {
        const long index = first + lane;
        SharedCounter counter = {counts, jpn::chromaOf(index, lumaBlocks)};
        if (!jpn::walkSymbols(reinterpret_cast<const short *>(staged + lane * STAGE_PITCH),
                              previousDc(coefficients, index, lumaBlocks), counter))
            atomicOr(flag, 1u);
    }
    __syncthreads();
    for (int i = lane; i < jpn::CENSUS_COUNTERS; i += GROUP)
        if (const u32 n = counts[i])
            atomicAdd(&histogram[i], n);
}

/* one workgroup per table slot (jpn::TABLE_SLOTS of them): `histogram` as jpn::Census to the slot's part of `huffman`
 * (values behind the last one are zero) and of `tables` */
__global__ __launch_bounds__(GROUP) void k_jpegOptimiseTables(const u32 *__restrict__ histogram,
                                                              jpn::Tables *__restrict__ tables,
                                                              jpn::Huffman *__restrict__ huffman)
{
    __shared__ u32 counts[256];
    __shared__ u32 sorted[jpn::MAX_TABLE_SYMBOLS];
    __shared__ int numCodes[jpn::MAX_TABLE_SYMBOLS];
    __shared__ u8 values[256];
    __shared__ u8 bits[16];
    const int lane = threadIdx.x;
    const int slot = blockIdx.x;
    const int length = jpn::slotLength(slot);
    const u32 *from = jpn::slotCounts(*reinterpret_cast<const jpn::Census *>(histogram), slot);
    u32 mine = 0;
    for (int i = lane; i < 256; i += GROUP)
    {
        counts[i] = i < length ? from[i] : 0u;
        values[i] = 0;
        mine += counts[i] ? 1u : 0u;
    }
    const int n = 1 + (int)waveSum(mine); /* the dummy and the used symbols */
    __syncthreads();
    /* the sort: every used symbol to its place behind the dummy; the values are that order reversed, without the dummy */
    if (lane == 0)
        sorted[0] = 1;
    for (int i = lane; i < length; i += GROUP)
        if (counts[i])
        {
            const int at = 1 + jpn::symbolRank(counts, length, i);
            sorted[at] = counts[i];
            values[n - 1 - at] = (u8)i;
        }
    __syncthreads();
    if (lane == 0)
        jpn::bitsOfSorted(sorted, n, numCodes, bits);
    __syncthreads();
    if (lane < 16)
        huffman->bits[slot][lane] = bits[lane];
    if (lane == 0)
        huffman->nbValues[slot] = n - 1;
    u32 *entries = jpn::slotEntries(*tables, slot);
    for (int i = lane; i < 256; i += GROUP)
    {
        huffman->values[slot][i] = values[i];
        if (i < length)
            entries[i] = 0;
    }
    __syncthreads(); /* (the zeros above and the entries below are different lanes') */
    /* annex C, as jpn::fillTable: value k's code counts up from the first code of its length */
    for (int k = lane; k < n - 1; k += GROUP)
    {
        u32 code = 0;
        int firstOfLength = 0;
        for (int l = 1; l <= jpn::MAX_CODE_BITS; ++l)
        {
            const int codes = bits[l - 1];
            if (k < firstOfLength + codes)
            {
                entries[values[k]] = (code + (u32)(k - firstOfLength)) | ((u32)l << 16);
                break;
            }
            code = (code + (u32)codes) << 1;
            firstOfLength += codes;
        }
    }
}

__global__ __launch_bounds__(GROUP) void k_jpegCountFF(const u32 *__restrict__ stream, const u64 nbBytes,
                                                       u64 *__restrict__ counts, const long nbChunks)
{
    const int lane = threadIdx.x;
    const u64 index = (u64)blockIdx.x * GROUP + lane;
    const int n = jpn::bytesOfWord(index, nbBytes);
    const u32 total = waveSum(n ? jpn::countFF(stream[index], n) : 0u);
    if (lane == 0)
    {
        counts[blockIdx.x] = total;
        if (blockIdx.x == 0)
            counts[nbChunks] = 0; /* item n of the scan */
    }
}

__global__ __launch_bounds__(GROUP) void k_jpegStuff(const u32 *__restrict__ stream, const u64 nbBytes,
                                                     const u64 *__restrict__ before, u8 *__restrict__ out)
{
    const int lane = threadIdx.x;
    const u64 index = (u64)blockIdx.x * GROUP + lane;
    const int n = jpn::bytesOfWord(index, nbBytes);
    const u32 word = n ? stream[index] : 0u;
    const u32 mine = jpn::countFF(word, n);
    /* the 0xFF of the lanes below: an inclusive scan across the wave, less this lane's */
    u32 below = mine;
    for (int step = 1; step < GROUP; step <<= 1)
    {
        const u32 other = __shfl_up(below, step, GROUP);
        if (lane >= step)
            below += other;
    }
    below -= mine;
    if (n)
        jpn::stuffWord(word, n, out + (index * 4u + before[blockIdx.x] + below));
}

std::atomic<unsigned long long> gCodedBlocks{0};

inline size_t roundUp(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

hipError_t exclusiveSum(void *temporary, size_t &temporaryBytes, const u64 *in, u64 *out, long n, hipStream_t stream)
{
    return hipcub::DeviceScan::ExclusiveSum(temporary, temporaryBytes, in, out, (int)n, stream);
}

static_assert(sizeof(SolrJpegHuffman) == sizeof(jpn::Huffman) && offsetof(SolrJpegHuffman, values) == offsetof(jpn::Huffman, values) &&
                  offsetof(SolrJpegHuffman, nbValues) == offsetof(jpn::Huffman, nbValues),
              "SolrJpegHuffman is jpn::Huffman");

/* census and tables on `stream`: dCoefficients to dHistogram (zeroed here), dTables and dHuffman; a block outside the
 * domain raises dFlag */
void launchOptimisedTables(const short *dCoefficients, long nbBlocks, int lumaBlocks, hipStream_t stream, u32 *dHistogram,
                           jpn::Tables *dTables, jpn::Huffman *dHuffman, u32 *dFlag)
{
    using namespace solreng;
    HIPCHECK(hipMemsetAsync(dHistogram, 0, sizeof(jpn::Census), stream));
    if (!ok())
        return;
    k_jpegSymbolCounts<<<dim3((unsigned)((nbBlocks + GROUP - 1) / GROUP)), dim3(GROUP), 0, stream>>>(
        dCoefficients, (int)nbBlocks, lumaBlocks, dHistogram, dFlag);
    HIPCHECK(hipGetLastError());
    if (!ok())
        return;
    k_jpegOptimiseTables<<<dim3(jpn::TABLE_SLOTS), dim3(GROUP), 0, stream>>>(dHistogram, dTables, dHuffman);
    HIPCHECK(hipGetLastError());
}

/* The stage on `stream`: dCoefficients (nbBlocks blocks on the device) to the caller's `scan`.  0; or -1 - with the error
 * set for a block outside the domain or a failed call, without for a capacity too small (*nbBytes then says what it
 * takes).  `scan` is written only by the last copy, when everything before it went well.  optimised not null: census and
 * tables first, the steps with those tables, and *optimised - written only with result 0 - is what the DHTs must say; it
 * comes with the first read-back, so the call synchronises as often as without */
int codeBlocks(const char *who, const short *dCoefficients, long nbBlocks, int lumaBlocks, hipStream_t stream,
               unsigned char *scan, long capacity, long *nbBytes, jpn::Huffman *optimised)
{
    using namespace solreng;
    const long nbGroups = (nbBlocks + GROUP - 1) / GROUP;
    unsigned char *first = nullptr, *second = nullptr, *third = nullptr;
    int result = -1;
    do
    {
        /* ---- bits, prefix ---- */
        const size_t itemBytes = roundUp((size_t)(nbBlocks + 1) * sizeof(u64));
        size_t scanBytes = 0;
        HIPCHECK(exclusiveSum(nullptr, scanBytes, nullptr, nullptr, nbBlocks + 1, stream));
        if (!ok())
            break;
        const size_t tableBytes = optimised ? 2 * roundUp(sizeof(jpn::Tables)) + roundUp(sizeof(jpn::Huffman)) : 0;
        HIPCHECK(hipMalloc((void **)&first, 2 * itemBytes + roundUp(scanBytes) + 256 + tableBytes));
        if (!ok())
            break;
        u64 *dBits = reinterpret_cast<u64 *>(first), *dOffsets = reinterpret_cast<u64 *>(first + itemBytes);
        unsigned char *dScan = first + 2 * itemBytes;
        u32 *dFlag = reinterpret_cast<u32 *>(first + 2 * itemBytes + roundUp(scanBytes));
        u32 *dHistogram = reinterpret_cast<u32 *>(first + 2 * itemBytes + roundUp(scanBytes) + 256);
        jpn::Tables *dTables = reinterpret_cast<jpn::Tables *>(reinterpret_cast<unsigned char *>(dHistogram) +
                                                               roundUp(sizeof(jpn::Tables)));
        jpn::Huffman *dHuffman = reinterpret_cast<jpn::Huffman *>(reinterpret_cast<unsigned char *>(dTables) +
                                                                  roundUp(sizeof(jpn::Tables)));
        HIPCHECK(hipMemsetAsync(dFlag, 0, sizeof(u32), stream));
        if (!ok())
            break;
        if (optimised)
        {
            launchOptimisedTables(dCoefficients, nbBlocks, lumaBlocks, stream, dHistogram, dTables, dHuffman, dFlag);
            if (!ok())
                break;
            k_jpegBlockBits<true><<<dim3((unsigned)nbGroups), dim3(GROUP), 0, stream>>>(dCoefficients, (int)nbBlocks,
                                                                                        lumaBlocks, dBits, dFlag, dTables);
        }
        else
            k_jpegBlockBits<false><<<dim3((unsigned)nbGroups), dim3(GROUP), 0, stream>>>(dCoefficients, (int)nbBlocks,
                                                                                         lumaBlocks, dBits, dFlag, nullptr);
        HIPCHECK(hipGetLastError());
        if (ok())
            HIPCHECK(exclusiveSum(dScan, scanBytes, dBits, dOffsets, nbBlocks + 1, stream));
        u64 totalBits = 0;
        u32 flag = 0;
        jpn::Huffman fetched;
        if (ok() && optimised)
            HIPCHECK(hipMemcpyAsync(&fetched, dHuffman, sizeof(fetched), hipMemcpyDeviceToHost, stream));
        if (ok())
            HIPCHECK(hipMemcpyAsync(&totalBits, dOffsets + nbBlocks, sizeof(u64), hipMemcpyDeviceToHost, stream));
        if (ok())
            HIPCHECK(hipMemcpyAsync(&flag, dFlag, sizeof(u32), hipMemcpyDeviceToHost, stream));
        if (ok())
            HIPCHECK(hipStreamSynchronize(stream));
        if (!ok())
            break;
        if (flag)
        {
            setError(-1, (std::string(who) + ": a block is outside what the standard tables code (|DC difference| <= 2047, "
                                             "|AC| <= 1023)").c_str(), __FILE__, __LINE__);
            break;
        }
        /* ---- emit, count, prefix ---- */
        const u64 unstuffedBytes = jpn::streamBytes(totalBits);
        const long nbChunks = (long)((unstuffedBytes + jpn::STUFF_CHUNK_BYTES - 1) / jpn::STUFF_CHUNK_BYTES);
        const size_t streamBytes = roundUp((size_t)jpn::streamWords(totalBits + (u64)jpn::tailBits(totalBits)) * sizeof(u32));
        const size_t chunkBytes = roundUp((size_t)(nbChunks + 1) * sizeof(u64));
        size_t chunkScanBytes = 0;
        HIPCHECK(exclusiveSum(nullptr, chunkScanBytes, nullptr, nullptr, nbChunks + 1, stream));
        if (!ok())
            break;
        HIPCHECK(hipMalloc((void **)&second, streamBytes + 2 * chunkBytes + roundUp(chunkScanBytes)));
        if (!ok())
            break;
        u32 *dStream = reinterpret_cast<u32 *>(second);
        u64 *dCounts = reinterpret_cast<u64 *>(second + streamBytes);
        u64 *dBefore = reinterpret_cast<u64 *>(second + streamBytes + chunkBytes);
        unsigned char *dChunkScan = second + streamBytes + 2 * chunkBytes;
        HIPCHECK(hipMemsetAsync(dStream, 0, streamBytes, stream));
        if (!ok())
            break;
        if (optimised)
            k_jpegEmit<true><<<dim3((unsigned)nbGroups), dim3(GROUP), 0, stream>>>(dCoefficients, (int)nbBlocks, lumaBlocks,
                                                                                   dOffsets, dStream, dTables);
        else
            k_jpegEmit<false><<<dim3((unsigned)nbGroups), dim3(GROUP), 0, stream>>>(dCoefficients, (int)nbBlocks,
                                                                                    lumaBlocks, dOffsets, dStream, nullptr);
        HIPCHECK(hipGetLastError());
        if (!ok())
            break;
        k_jpegCountFF<<<dim3((unsigned)nbChunks), dim3(GROUP), 0, stream>>>(dStream, unstuffedBytes, dCounts, nbChunks);
        HIPCHECK(hipGetLastError());
        if (ok())
            HIPCHECK(exclusiveSum(dChunkScan, chunkScanBytes, dCounts, dBefore, nbChunks + 1, stream));
        u64 nbStuffed = 0;
        if (ok())
            HIPCHECK(hipMemcpyAsync(&nbStuffed, dBefore + nbChunks, sizeof(u64), hipMemcpyDeviceToHost, stream));
        if (ok())
            HIPCHECK(hipStreamSynchronize(stream));
        if (!ok())
            break;
        *nbBytes = (long)(unstuffedBytes + nbStuffed);
        if (*nbBytes > capacity)
            break; /* (no error: the caller comes back with a buffer of that size) */
        /* ---- stuff ---- */
        HIPCHECK(hipMalloc((void **)&third, roundUp((size_t)*nbBytes)));
        if (!ok())
            break;
        k_jpegStuff<<<dim3((unsigned)nbChunks), dim3(GROUP), 0, stream>>>(dStream, unstuffedBytes, dBefore, third);
        HIPCHECK(hipGetLastError());
        if (ok())
            HIPCHECK(hipMemcpyAsync(scan, third, (size_t)*nbBytes, hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        if (!ok())
            break;
        gCodedBlocks += (unsigned long long)nbBlocks;
        if (optimised)
            *optimised = fetched;
        result = 0;
    } while (false);
    if (!ok())
        (void)hipStreamSynchronize(stream); /* nothing of ours may still run when the buffers go */
    for (unsigned char *buffer : {first, second, third})
        if (buffer)
            (void)hipFree(buffer);
    return result;
}

/* what the three entries ask of the caller's buffer */
bool outputAccepted(const char *who, const unsigned char *scan, long capacity, long *nbBytes)
{
    if (scan && capacity >= 0 && nbBytes)
        return true;
    solreng::setError(-1, (std::string(who) + ": null scan or nbBytes, or a negative capacity").c_str(), __FILE__, __LINE__);
    return false;
}

/* ... and the optimised entries of theirs */
bool tablesAccepted(const char *who, const SolrJpegHuffman *tables)
{
    if (tables)
        return true;
    solreng::setError(-1, (std::string(who) + ": null tables").c_str(), __FILE__, __LINE__);
    return false;
}

/* solr_hip_jpeg_blocks_to_scan and solr_hip_rgb_to_jpeg_scan: exactly one of hostBlocks and hostRgb */
int fromHost(const char *who, const SolrJpegSource *source, const short *hostBlocks, const unsigned char *hostRgb,
             long nbBlocks, unsigned char *scan, long capacity, long *nbBytes, SolrJpegHuffman *optimised = nullptr)
{
    using namespace solreng;
    int before = -1;
    if (hipGetDevice(&before) != hipSuccess)
        before = -1;
    HIPCHECK(hipSetDevice(solr_hip_get_device()));
    JpegEncodeTables tables;
    const size_t tableBytes = roundUp(sizeof(tables));
    const size_t coefficientBytes = (size_t)nbBlocks * 64 * sizeof(short);
    const size_t rgbBytes = hostRgb ? (size_t)source->width * source->height * 3 : 0;
    unsigned char *device = nullptr;
    hipStream_t stream = nullptr;
    int result = -1;
    if (ok())
        HIPCHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    if (ok())
        HIPCHECK(hipMalloc((void **)&device, tableBytes + roundUp(coefficientBytes) + roundUp(rgbBytes)));
    if (ok())
    {
        short *dCoefficients = reinterpret_cast<short *>(device + tableBytes);
        unsigned char *dRgb = device + tableBytes + roundUp(coefficientBytes);
        if (hostRgb)
        {
            HIPCHECK(hipMemcpyAsync(dRgb, hostRgb, rgbBytes, hipMemcpyHostToDevice, stream));
            if (ok())
                launchJpegCoefficients(*source, tables, reinterpret_cast<JpegEncodeTables *>(device), dRgb, dCoefficients,
                                       nbBlocks, stream);
        }
        else
            HIPCHECK(hipMemcpyAsync(dCoefficients, hostBlocks, coefficientBytes, hipMemcpyHostToDevice, stream));
        if (ok())
            result = codeBlocks(who, dCoefficients, nbBlocks, source->lumaH * source->lumaV, stream, scan, capacity, nbBytes,
                                reinterpret_cast<jpn::Huffman *>(optimised));
        (void)hipStreamSynchronize(stream);
        if (hostRgb && ok() && result == 0)
            countJpegEncodedBlocks(nbBlocks);
    }
    if (device)
        (void)hipFree(device);
    if (stream)
        (void)hipStreamDestroy(stream);
    if (before >= 0)
        (void)hipSetDevice(before);
    return ok() ? result : -1;
}
/* the three entries and their optimised variants: `optimised` null for the standard tables */
int blocksToScan(const char *who, const SolrJpegSource *source, const short *coefficients, long nbBlocks,
                 unsigned char *scan, long capacity, long *nbBytes, SolrJpegHuffman *optimised, bool wantsTables)
{
    using namespace solreng;
    if (!ok())
        return -1;
    /* ---- arguments: nothing is launched for a call that fails here ---- */
    if (!source || !coefficients)
    {
        setError(-1, (std::string(who) + ": null source or coefficients").c_str(), __FILE__, __LINE__);
        return -1;
    }
    long expected = 0;
    if (!outputAccepted(who, scan, capacity, nbBytes) || (wantsTables && !tablesAccepted(who, optimised)) ||
        !jpegSourceAccepted(who, source, &expected))
        return -1;
    if (nbBlocks != expected)
    {
        setError(-1, (std::string(who) + ": nbBlocks does not match the image size and sampling").c_str(), __FILE__,
                 __LINE__);
        return -1;
    }
    return fromHost(who, source, coefficients, nullptr, nbBlocks, scan, capacity, nbBytes, optimised);
}

int rgbToScan(const char *who, const SolrJpegSource *source, const unsigned char *rgb, unsigned char *scan, long capacity,
              long *nbBytes, SolrJpegHuffman *optimised, bool wantsTables)
{
    using namespace solreng;
    if (!ok())
        return -1;
    if (!source || !rgb)
    {
        setError(-1, (std::string(who) + ": null source or rgb").c_str(), __FILE__, __LINE__);
        return -1;
    }
    long nbBlocks = 0;
    if (!outputAccepted(who, scan, capacity, nbBytes) || (wantsTables && !tablesAccepted(who, optimised)) ||
        !jpegSourceAccepted(who, source, &nbBlocks))
        return -1;
    return fromHost(who, source, nullptr, rgb, nbBlocks, scan, capacity, nbBytes, optimised);
}

int frameToScan(const char *who, int quality, int lumaH, int lumaV, unsigned char *scan, long capacity, long *nbBytes,
                SolrJpegHuffman *optimised, bool wantsTables)
{
    using namespace solreng;
    if (!ready(who))
        return -1;
    /* declined, and no error: a frame in strips or on several devices is not in one image, and before the first frame
     * there is none */
    Flight &set = g.flight[g.current];
    const unsigned char *image = reinterpret_cast<const unsigned char *>(g.boundBitmap ? g.boundBitmap : set.shown().ptr);
    if (gDevices > 1 || g.nbRows >= 0 || g.frameBufferType < 0 || !image)
        return -1;
    const SolrJpegSource source = {g.width, g.height, lumaH, lumaV, quality, 1, g.frameBufferType != (int)ftRGB ? 1 : 0};
    long nbBlocks = 0;
    if (!outputAccepted(who, scan, capacity, nbBytes) || (wantsTables && !tablesAccepted(who, optimised)) ||
        !jpegSourceAccepted(who, &source, &nbBlocks))
        return -1;
    HIPCHECK(hipSetDevice(g.device));
    /* behind the frame, on its stream */
    const hipStream_t stream = set.stream;
    JpegEncodeTables tables;
    const size_t tableBytes = roundUp(sizeof(tables));
    unsigned char *device = nullptr;
    int result = -1;
    if (ok())
        HIPCHECK(hipMalloc((void **)&device, tableBytes + roundUp((size_t)nbBlocks * 64 * sizeof(short))));
    if (ok())
    {
        short *dCoefficients = reinterpret_cast<short *>(device + tableBytes);
        launchJpegCoefficients(source, tables, reinterpret_cast<JpegEncodeTables *>(device), image, dCoefficients, nbBlocks,
                               stream);
        if (ok())
            result = codeBlocks(who, dCoefficients, nbBlocks, lumaH * lumaV, stream, scan, capacity, nbBytes,
                                reinterpret_cast<jpn::Huffman *>(optimised));
        (void)hipStreamSynchronize(stream);
        if (ok() && result == 0)
            countJpegEncodedBlocks(nbBlocks);
    }
    if (device)
        (void)hipFree(device);
    return ok() ? result : -1;
}
}

/* ---- JPEG frames in flight: the resident, wait-free pipeline (engine.h JpegSlot; solr_hip_frame_to_jpeg_async) ----------
 * The steps above with nothing read back between them.  Buffers and launches are sized by the number of blocks alone
 * (jpn::maxStreamBytes, maxStreamChunks, maxStuffedBytes); k_jpegPlan turns the scan's total into the extents
 * (jpn::ScanPlan) that k_jpegCountFFResident and k_jpegStuffResident read where their namesakes took arguments: a chunk
 * beyond the extent counts zero and writes nothing.  The stream's buffer stays: k_jpegEmit ORs into zeros, so the words a
 * use dirtied are zeroed behind it by the step that reads them last (k_jpegStuffResident) - or, SOLR_HIP_JPEG_ZERO_BOUND=1,
 * the whole bound is zeroed in front of every emit (the alternative, kept for the measurement).  A block outside the
 * domain: the plan's extents are zero and k_jpegPlan zeroes the offsets, at which k_jpegEmit's guard returns - nothing is
 * written beyond the record. */
namespace
{
/* what the steps hand each other and, copied to the slot's page-locked record, the host */
struct JpegRecord
{
    jpn::ScanPlan plan;
    u64 stuffedBytes; /* the segment: plan.unstuffedBytes + the 0xFF of all chunks */
    u32 flag;         /* raised by k_jpegBlockBits / k_jpegSymbolCounts */
    u32 pad;
    jpn::Huffman huffman; /* optimised mode: what the DHTs must say */
};

/* one wave: the total behind the offsets and the flag to the plan; a flagged frame's offsets all to zero */
__global__ __launch_bounds__(GROUP) void k_jpegPlan(u64 *__restrict__ offsets, const int nbBlocks, JpegRecord *__restrict__ record)
{
    const u32 flag = record->flag;
    if (threadIdx.x == 0)
        record->plan = jpn::planScan(offsets[nbBlocks], flag);
    if (flag)
    {
        __syncthreads(); /* (lane 0 has read the total) */
        for (int i = threadIdx.x; i <= nbBlocks; i += GROUP)
            offsets[i] = 0;
    }
}

/* k_jpegCountFF over the bound: nbChunks is the bound's, the extent the record's */
__global__ __launch_bounds__(GROUP) void k_jpegCountFFResident(const u32 *__restrict__ stream,
                                                               const JpegRecord *__restrict__ record,
                                                               u64 *__restrict__ counts, const long nbChunks)
{
    const int lane = threadIdx.x;
    const u64 index = (u64)blockIdx.x * GROUP + lane;
    const int n = jpn::planBytesOfWord(record->plan, index);
    const u32 total = waveSum(n ? jpn::countFF(stream[index], n) : 0u);
    if (lane == 0)
    {
        counts[blockIdx.x] = total;
        if (blockIdx.x == 0)
            counts[nbChunks] = 0; /* item n of the scan */
    }
}

/* k_jpegStuff over the bound; chunk 0 also leaves the segment's size.  clearBehind: the words read are left zero */
__global__ __launch_bounds__(GROUP) void k_jpegStuffResident(u32 *stream, JpegRecord *record, const u64 *__restrict__ before,
                                                             u8 *__restrict__ out, const long nbChunks, const int clearBehind)
{
    const int lane = threadIdx.x;
    const jpn::ScanPlan plan = record->plan;
    if (blockIdx.x == 0 && lane == 0)
        record->stuffedBytes = plan.unstuffedBytes + before[nbChunks];
    if ((u64)blockIdx.x >= plan.nbChunks)
        return;
    const u64 index = (u64)blockIdx.x * GROUP + lane;
    const int n = jpn::planBytesOfWord(plan, index);
    const u32 word = n ? stream[index] : 0u;
    const u32 mine = jpn::countFF(word, n);
    u32 below = mine;
    for (int step = 1; step < GROUP; step <<= 1)
    {
        const u32 other = __shfl_up(below, step, GROUP);
        if (lane >= step)
            below += other;
    }
    below -= mine;
    if (n)
    {
        jpn::stuffWord(word, n, out + (index * 4u + before[blockIdx.x] + below));
        if (clearBehind)
            stream[index] = 0;
    }
}

bool zeroTheBound()
{
    const char *env = getenv("SOLR_HIP_JPEG_ZERO_BOUND");
    return env && env[0] == '1';
}

void freeSlot(solreng::JpegSlot &slot)
{
    if (slot.used && slot.done)
        (void)hipEventSynchronize(slot.done); /* nothing of the slot's may still run when its memory goes */
    solreng::release(slot.block);
    if (slot.hostRecord)
        (void)hipHostFree(slot.hostRecord);
    if (slot.done)
        (void)hipEventDestroy(slot.done);
    slot = solreng::JpegSlot();
}

void freeRetired(solreng::JpegRetired &old)
{
    solreng::release(old.block);
    if (old.hostRecord)
        (void)hipHostFree(old.hostRecord);
    if (old.done)
        (void)hipEventDestroy(old.done);
}

/* the slots set aside whose last use is through are given back; none is waited for unless there are too many */
void sweepRetired(solreng::JpegStream &js)
{
    for (size_t i = 0; i < js.retired.size();)
        if (hipEventQuery(js.retired[i].done) == hipSuccess)
        {
            freeRetired(js.retired[i]);
            js.retired.erase(js.retired.begin() + (long)i);
        }
        else
            ++i;
    while (js.retired.size() > solreng::JpegStream::RETIRED_MOST)
    {
        ++js.hostWaits;
        (void)hipEventSynchronize(js.retired.front().done);
        freeRetired(js.retired.front());
        js.retired.erase(js.retired.begin());
    }
}

/* the slot cut for nbBlocks blocks or more: as it is, or - the first use, a frame of more blocks - made anew */
bool ensureSlot(solreng::JpegSlot &slot, long nbBlocks)
{
    using namespace solreng;
    size_t scanBytes = 0, chunkScanBytes = 0;
    const long nbChunks = (long)jpn::maxStreamChunks(nbBlocks);
    HIPCHECK(exclusiveSum(nullptr, scanBytes, nullptr, nullptr, nbBlocks + 1, nullptr));
    if (ok())
        HIPCHECK(exclusiveSum(nullptr, chunkScanBytes, nullptr, nullptr, nbChunks + 1, nullptr));
    if (!ok())
        return false;
    if (slot.block.ptr && slot.capacityBlocks >= nbBlocks && slot.scanBytes >= scanBytes && slot.chunkScanBytes >= chunkScanBytes)
        return true;
    /* a frame of more blocks than the slot was cut for: what its last use may still read is set aside, not waited for */
    if (slot.used)
    {
        g.jpeg.retired.push_back({slot.block, slot.hostRecord, slot.done});
        slot = JpegSlot();
    }
    freeSlot(slot);
    const size_t itemBytes = roundUp((size_t)(nbBlocks + 1) * sizeof(u64));
    const size_t chunkBytes = roundUp((size_t)(nbChunks + 1) * sizeof(u64));
    /* whole chunks: k_jpegCountFFResident's grid is the bound's */
    const size_t streamBytes = roundUp((size_t)nbChunks * jpn::STUFF_CHUNK_BYTES);
    const size_t part = roundUp(sizeof(jpn::Tables));
    const size_t cuts[] = {roundUp(sizeof(JpegEncodeTables)), roundUp((size_t)nbBlocks * 64 * sizeof(short)), itemBytes, itemBytes,
                           roundUp(scanBytes), streamBytes, chunkBytes, chunkBytes, roundUp(chunkScanBytes),
                           roundUp((size_t)jpn::maxStuffedBytes(nbBlocks) + 8), part, part, roundUp(sizeof(JpegRecord))};
    size_t total = 0;
    for (const size_t cut : cuts)
        total += cut;
    reserve(slot.block, total);
    if (ok())
    {
        ++g.jpeg.allocations;
        HIPCHECK(hipHostMalloc(&slot.hostRecord, sizeof(JpegRecord), hipHostMallocDefault));
    }
    if (ok())
    {
        ++g.jpeg.allocations;
        HIPCHECK(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));
    }
    if (!ok())
    {
        freeSlot(slot);
        return false;
    }
    unsigned char *at = static_cast<unsigned char *>(slot.block.ptr);
    unsigned char **const fields[] = {&slot.encodeTables, &slot.coefficients, &slot.bits, &slot.offsets, &slot.scanTemp,
                                      &slot.stream, &slot.counts, &slot.before, &slot.chunkScanTemp, &slot.out,
                                      &slot.histogram, &slot.tables, &slot.record};
    for (size_t i = 0; i < sizeof(cuts) / sizeof(cuts[0]); ++i)
    {
        *fields[i] = at;
        at += cuts[i];
    }
    slot.capacityBlocks = nbBlocks;
    slot.scanBytes = roundUp(scanBytes);
    slot.chunkScanBytes = roundUp(chunkScanBytes);
    slot.streamBytes = streamBytes;
    return true;
}

/* One implementation for frames and the probe: the next slot, behind its last use; the blocks from `image` (the pixel
 * stage) or from the caller's `hostBlocks`; every entropy step; the record's read-back; the event.  The ticket, or -1 with
 * the error set.  Nothing here waits for the device but the upload of pageable `hostBlocks` (the probe's) */
int submitJpeg(const SolrJpegSource &source, const unsigned char *image, const short *hostBlocks, long nbBlocks, bool optimised,
               hipStream_t stream)
{
    using namespace solreng;
    JpegStream &js = g.jpeg;
    JpegSlot &slot = js.slot[js.issued % JPEG_SLOTS];
    slot.serial = -1; /* the ticket that held the slot is stale from here on */
    if (!js.retired.empty())
        sweepRetired(js);
    if (!ensureSlot(slot, nbBlocks))
        return -1;
    const int lumaBlocks = source.lumaH * source.lumaV;
    const long nbGroups = (nbBlocks + GROUP - 1) / GROUP;
    const long nbChunks = (long)jpn::maxStreamChunks(nbBlocks);
    const bool zeroBound = zeroTheBound();
    short *dCoefficients = reinterpret_cast<short *>(slot.coefficients);
    u64 *dBits = reinterpret_cast<u64 *>(slot.bits), *dOffsets = reinterpret_cast<u64 *>(slot.offsets);
    u32 *dStream = reinterpret_cast<u32 *>(slot.stream);
    u64 *dCounts = reinterpret_cast<u64 *>(slot.counts), *dBefore = reinterpret_cast<u64 *>(slot.before);
    JpegRecord *dRecord = reinterpret_cast<JpegRecord *>(slot.record);
    jpn::Tables *dTables = reinterpret_cast<jpn::Tables *>(slot.tables);
    size_t scanBytes = slot.scanBytes, chunkScanBytes = slot.chunkScanBytes;
    /* the slot's last use may have run on another stream */
    if (slot.used)
        HIPCHECK(hipStreamWaitEvent(stream, slot.done, 0));
    if (ok() && (zeroBound || !slot.clean))
        HIPCHECK(hipMemsetAsync(dStream, 0, slot.streamBytes, stream));
    slot.clean = false;
    if (ok())
        HIPCHECK(hipMemsetAsync(dRecord, 0, sizeof(JpegRecord), stream));
    if (ok() && image)
        launchJpegCoefficientsResident(source, reinterpret_cast<JpegEncodeTables *>(slot.encodeTables), image, dCoefficients,
                                       nbBlocks, stream);
    else if (ok())
    {
        HIPCHECK(hipMemcpyAsync(dCoefficients, hostBlocks, (size_t)nbBlocks * 64 * sizeof(short), hipMemcpyHostToDevice, stream));
        HIPCHECK(hipStreamSynchronize(stream)); /* (pageable memory of the caller's: his again when this returns) */
    }
    if (ok() && optimised)
        launchOptimisedTables(dCoefficients, nbBlocks, lumaBlocks, stream, reinterpret_cast<u32 *>(slot.histogram), dTables,
                              &dRecord->huffman, &dRecord->flag);
    if (ok())
    {
        if (optimised)
            k_jpegBlockBits<true><<<dim3((unsigned)nbGroups), dim3(GROUP), 0, stream>>>(dCoefficients, (int)nbBlocks,
                                                                                        lumaBlocks, dBits, &dRecord->flag, dTables);
        else
            k_jpegBlockBits<false><<<dim3((unsigned)nbGroups), dim3(GROUP), 0, stream>>>(dCoefficients, (int)nbBlocks,
                                                                                         lumaBlocks, dBits, &dRecord->flag, nullptr);
        HIPCHECK(hipGetLastError());
    }
    if (ok())
        HIPCHECK(exclusiveSum(slot.scanTemp, scanBytes, dBits, dOffsets, nbBlocks + 1, stream));
    if (ok())
    {
        k_jpegPlan<<<dim3(1), dim3(GROUP), 0, stream>>>(dOffsets, (int)nbBlocks, dRecord);
        HIPCHECK(hipGetLastError());
    }
    if (ok())
    {
        if (optimised)
            k_jpegEmit<true><<<dim3((unsigned)nbGroups), dim3(GROUP), 0, stream>>>(dCoefficients, (int)nbBlocks, lumaBlocks,
                                                                                   dOffsets, dStream, dTables);
        else
            k_jpegEmit<false><<<dim3((unsigned)nbGroups), dim3(GROUP), 0, stream>>>(dCoefficients, (int)nbBlocks,
                                                                                    lumaBlocks, dOffsets, dStream, nullptr);
        HIPCHECK(hipGetLastError());
    }
    if (ok())
    {
        k_jpegCountFFResident<<<dim3((unsigned)nbChunks), dim3(GROUP), 0, stream>>>(dStream, dRecord, dCounts, nbChunks);
        HIPCHECK(hipGetLastError());
    }
    if (ok())
        HIPCHECK(exclusiveSum(slot.chunkScanTemp, chunkScanBytes, dCounts, dBefore, nbChunks + 1, stream));
    if (ok())
    {
        k_jpegStuffResident<<<dim3((unsigned)nbChunks), dim3(GROUP), 0, stream>>>(dStream, dRecord, dBefore, slot.out, nbChunks,
                                                                                  zeroBound ? 0 : 1);
        HIPCHECK(hipGetLastError());
    }
    if (ok())
        HIPCHECK(hipMemcpyAsync(slot.hostRecord, dRecord, optimised ? sizeof(JpegRecord) : offsetof(JpegRecord, huffman),
                                hipMemcpyDeviceToHost, stream));
    if (ok())
        HIPCHECK(hipEventRecord(slot.done, stream));
    if (!ok())
        return -1; /* (the slot stays dirty: its next use zeroes the whole stream) */
    slot.used = true;
    slot.clean = !zeroBound;
    slot.serial = js.issued++;
    slot.nbBlocks = nbBlocks;
    slot.optimised = optimised;
    slot.fromFrame = image != nullptr;
    slot.collected = false;
    return JpegStream::ticketOf(slot.serial);
}
}

namespace solreng
{
void JpegStream::release()
{
    for (JpegSlot &s : slot)
        freeSlot(s);
    for (JpegRetired &old : retired)
    {
        (void)hipEventSynchronize(old.done);
        freeRetired(old);
    }
    retired.clear();
    for (hipStream_t *stream : {&probeStream, &copyStream})
    {
        if (*stream)
            (void)hipStreamDestroy(*stream);
        *stream = nullptr;
    }
}
}

extern "C" {

int solr_hip_jpeg_blocks_to_scan(const SolrJpegSource *source, const short *coefficients, long nbBlocks,
                                 unsigned char *scan, long capacity, long *nbBytes)
{
    return blocksToScan("solr_hip_jpeg_blocks_to_scan", source, coefficients, nbBlocks, scan, capacity, nbBytes, nullptr,
                        false);
}

int solr_hip_rgb_to_jpeg_scan(const SolrJpegSource *source, const unsigned char *rgb, unsigned char *scan, long capacity,
                              long *nbBytes)
{
    return rgbToScan("solr_hip_rgb_to_jpeg_scan", source, rgb, scan, capacity, nbBytes, nullptr, false);
}

int solr_hip_frame_to_jpeg_scan(int quality, int lumaH, int lumaV, unsigned char *scan, long capacity, long *nbBytes)
{
    return frameToScan("solr_hip_frame_to_jpeg_scan", quality, lumaH, lumaV, scan, capacity, nbBytes, nullptr, false);
}

int solr_hip_jpeg_blocks_to_scan_optimised(const SolrJpegSource *source, const short *coefficients, long nbBlocks,
                                           unsigned char *scan, long capacity, long *nbBytes, SolrJpegHuffman *tables)
{
    return blocksToScan("solr_hip_jpeg_blocks_to_scan_optimised", source, coefficients, nbBlocks, scan, capacity, nbBytes,
                        tables, true);
}

int solr_hip_rgb_to_jpeg_scan_optimised(const SolrJpegSource *source, const unsigned char *rgb, unsigned char *scan,
                                        long capacity, long *nbBytes, SolrJpegHuffman *tables)
{
    return rgbToScan("solr_hip_rgb_to_jpeg_scan_optimised", source, rgb, scan, capacity, nbBytes, tables, true);
}

int solr_hip_frame_to_jpeg_scan_optimised(int quality, int lumaH, int lumaV, unsigned char *scan, long capacity,
                                          long *nbBytes, SolrJpegHuffman *tables)
{
    return frameToScan("solr_hip_frame_to_jpeg_scan_optimised", quality, lumaH, lumaV, scan, capacity, nbBytes, tables,
                       true);
}

/* ---- the probes of include/solr_hip_probes_jpeg.h ---- */
namespace
{
/* the two kernels of the optimised tables on a stream of their own; exactly one of hostBlocks and hostCounts */
int probeTables(const char *who, const short *hostBlocks, long nbBlocks, int lumaBlocks, const unsigned int *hostCounts,
                unsigned int *counts, SolrJpegHuffman *tables)
{
    using namespace solreng;
    int before = -1;
    if (hipGetDevice(&before) != hipSuccess)
        before = -1;
    HIPCHECK(hipSetDevice(solr_hip_get_device()));
    const size_t blockBytes = hostBlocks ? roundUp((size_t)nbBlocks * 64 * sizeof(short)) : 0;
    const size_t part = roundUp(sizeof(jpn::Tables));
    unsigned char *device = nullptr;
    hipStream_t stream = nullptr;
    jpn::Census census;
    jpn::Huffman huffman;
    u32 flag = 0;
    if (ok())
        HIPCHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    if (ok())
        HIPCHECK(hipMalloc((void **)&device, blockBytes + 3 * part + 256));
    if (ok())
    {
        short *dBlocks = reinterpret_cast<short *>(device);
        u32 *dHistogram = reinterpret_cast<u32 *>(device + blockBytes);
        jpn::Tables *dTables = reinterpret_cast<jpn::Tables *>(device + blockBytes + part);
        jpn::Huffman *dHuffman = reinterpret_cast<jpn::Huffman *>(device + blockBytes + 2 * part);
        u32 *dFlag = reinterpret_cast<u32 *>(device + blockBytes + 3 * part);
        HIPCHECK(hipMemsetAsync(dFlag, 0, sizeof(u32), stream));
        if (ok() && hostBlocks)
        {
            HIPCHECK(hipMemcpyAsync(dBlocks, hostBlocks, (size_t)nbBlocks * 64 * sizeof(short), hipMemcpyHostToDevice, stream));
            if (ok())
                launchOptimisedTables(dBlocks, nbBlocks, lumaBlocks, stream, dHistogram, dTables, dHuffman, dFlag);
        }
        else if (ok())
        {
            HIPCHECK(hipMemcpyAsync(dHistogram, hostCounts, sizeof(jpn::Census), hipMemcpyHostToDevice, stream));
            if (ok())
            {
                k_jpegOptimiseTables<<<dim3(jpn::TABLE_SLOTS), dim3(GROUP), 0, stream>>>(dHistogram, dTables, dHuffman);
                HIPCHECK(hipGetLastError());
            }
        }
        if (ok())
            HIPCHECK(hipMemcpyAsync(&census, dHistogram, sizeof(census), hipMemcpyDeviceToHost, stream));
        if (ok())
            HIPCHECK(hipMemcpyAsync(&huffman, dHuffman, sizeof(huffman), hipMemcpyDeviceToHost, stream));
        if (ok())
            HIPCHECK(hipMemcpyAsync(&flag, dFlag, sizeof(u32), hipMemcpyDeviceToHost, stream));
        (void)hipStreamSynchronize(stream);
    }
    if (device)
        (void)hipFree(device);
    if (stream)
        (void)hipStreamDestroy(stream);
    if (before >= 0)
        (void)hipSetDevice(before);
    if (!ok())
        return -1;
    if (flag)
    {
        setError(-1, (std::string(who) + ": a block is outside the domain (|DC difference| <= 2047, |AC| <= 1023)").c_str(),
                 __FILE__, __LINE__);
        return -1;
    }
    if (counts)
        memcpy(counts, &census, sizeof(census));
    if (tables)
        memcpy(tables, &huffman, sizeof(huffman));
    return 0;
}
}

int solr_hip_probe_jpeg_census(const short *coefficients, long nbBlocks, int lumaBlocks, unsigned int *counts)
{
    using namespace solreng;
    if (!ok())
        return -1;
    if (!coefficients || !counts || nbBlocks < 1 || nbBlocks > (1L << 24) ||
        (lumaBlocks != 1 && lumaBlocks != 2 && lumaBlocks != 4))
    {
        setError(-1, "solr_hip_probe_jpeg_census: null blocks or counts, a block count outside 1 ... 2^24, or luma blocks "
                     "per MCU other than 1, 2 or 4", __FILE__, __LINE__);
        return -1;
    }
    return probeTables("solr_hip_probe_jpeg_census", coefficients, nbBlocks, lumaBlocks, nullptr, counts, nullptr);
}

int solr_hip_probe_jpeg_tables(const unsigned int *counts, SolrJpegHuffman *tables)
{
    using namespace solreng;
    if (!ok())
        return -1;
    if (!counts || !tables)
    {
        setError(-1, "solr_hip_probe_jpeg_tables: null counts or tables", __FILE__, __LINE__);
        return -1;
    }
    return probeTables("solr_hip_probe_jpeg_tables", nullptr, 0, 0, counts, nullptr, tables);
}

unsigned long long solr_hip_jpeg_coded_blocks(void)
{
    return gCodedBlocks.load();
}

/* ---- JPEG frames in flight ---- */
int solr_hip_jpeg_stream_offered(void)
{
    using namespace solreng;
    return g.initialized && gDevices == 1 && g.nbRows < 0 ? 1 : 0;
}

int solr_hip_frame_to_jpeg_async(int quality, int lumaH, int lumaV, int optimised)
{
    using namespace solreng;
    const char *who = "solr_hip_frame_to_jpeg_async";
    if (!ready(who))
        return -1;
    /* declined, and no error: solr_hip_frame_to_jpeg_scan's reasons */
    Flight &set = g.flight[g.current];
    const unsigned char *image = reinterpret_cast<const unsigned char *>(g.boundBitmap ? g.boundBitmap : set.shown().ptr);
    if (gDevices > 1 || g.nbRows >= 0 || g.frameBufferType < 0 || !image)
        return -1;
    const SolrJpegSource source = {g.width, g.height, lumaH, lumaV, quality, 1, g.frameBufferType != (int)ftRGB ? 1 : 0};
    long nbBlocks = 0;
    if (!jpegSourceAccepted(who, &source, &nbBlocks))
        return -1;
    HIPCHECK(hipSetDevice(g.device));
    if (!ok())
        return -1;
    /* behind the frame, on its stream */
    return submitJpeg(source, image, nullptr, nbBlocks, optimised != 0, set.stream);
}

int solr_hip_probe_jpeg_stream_blocks(const SolrJpegSource *source, const short *coefficients, long nbBlocks, int optimised)
{
    using namespace solreng;
    const char *who = "solr_hip_probe_jpeg_stream_blocks";
    if (!ok())
        return -1;
    if (!source || !coefficients)
    {
        setError(-1, "solr_hip_probe_jpeg_stream_blocks: null source or coefficients", __FILE__, __LINE__);
        return -1;
    }
    long expected = 0;
    if (!jpegSourceAccepted(who, source, &expected))
        return -1;
    if (nbBlocks != expected)
    {
        setError(-1, "solr_hip_probe_jpeg_stream_blocks: nbBlocks does not match the image size and sampling", __FILE__,
                 __LINE__);
        return -1;
    }
    int before = -1;
    if (hipGetDevice(&before) != hipSuccess)
        before = -1;
    HIPCHECK(hipSetDevice(solr_hip_get_device()));
    if (ok() && !g.jpeg.probeStream)
        HIPCHECK(hipStreamCreateWithFlags(&g.jpeg.probeStream, hipStreamNonBlocking));
    const int ticket = ok() ? submitJpeg(*source, nullptr, coefficients, nbBlocks, optimised != 0, g.jpeg.probeStream) : -1;
    if (before >= 0)
        (void)hipSetDevice(before);
    return ok() ? ticket : -1;
}

int solr_hip_jpeg_wait(int ticket, unsigned char *scan, long capacity, long *nbBytes, SolrJpegHuffman *tables)
{
    using namespace solreng;
    const char *who = "solr_hip_jpeg_wait";
    if (!ok() || !outputAccepted(who, scan, capacity, nbBytes))
        return -1;
    JpegStream &js = g.jpeg;
    JpegSlot *slot = ticket >= 0 ? &js.slot[ticket % JPEG_SLOTS] : nullptr;
    if (!slot || slot->serial < 0 || slot->serial % JpegStream::TICKET_PERIOD != (long)(ticket / JPEG_SLOTS))
    {
        setError(-1, "solr_hip_jpeg_wait: no such ticket: it was never handed out, four tickets have followed it, or the frame "
                     "was re-shaped or the scene finalized since", __FILE__, __LINE__);
        return -1;
    }
    if (slot->optimised && !tablesAccepted(who, tables))
        return -1;
    int before = -1;
    if (hipGetDevice(&before) != hipSuccess)
        before = -1;
    HIPCHECK(hipSetDevice(g.initialized ? g.device : solr_hip_get_device()));
    if (ok())
        HIPCHECK(hipEventSynchronize(slot->done));
    int result = -1;
    const JpegRecord *record = static_cast<const JpegRecord *>(slot->hostRecord);
    if (ok() && (record->flag || record->plan.flag))
        setError(-1, "solr_hip_jpeg_wait: a block is outside what the tables code (|DC difference| <= 2047, |AC| <= 1023)",
                 __FILE__, __LINE__);
    else if (ok())
    {
        *nbBytes = (long)record->stuffedBytes;
        if (*nbBytes <= capacity) /* (else no error: the caller comes back with a buffer of that size) */
        {
            if (!js.copyStream)
                HIPCHECK(hipStreamCreateWithFlags(&js.copyStream, hipStreamNonBlocking));
            if (ok())
                HIPCHECK(hipMemcpyAsync(scan, slot->out, (size_t)*nbBytes, hipMemcpyDeviceToHost, js.copyStream));
            if (ok())
                HIPCHECK(hipStreamSynchronize(js.copyStream));
            if (ok())
            {
                if (slot->optimised)
                    memcpy(tables, &record->huffman, sizeof(jpn::Huffman));
                if (!slot->collected)
                {
                    slot->collected = true;
                    gCodedBlocks += (unsigned long long)slot->nbBlocks;
                    if (slot->fromFrame)
                        countJpegEncodedBlocks(slot->nbBlocks);
                    js.bytesDelivered += (unsigned long long)*nbBytes;
                }
                result = 0;
            }
        }
    }
    if (before >= 0)
        (void)hipSetDevice(before);
    return ok() ? result : -1;
}

void solr_hip_jpeg_stream_stats(unsigned long long out[4])
{
    using namespace solreng;
    if (!out)
        return;
    out[0] = (unsigned long long)g.jpeg.issued;
    out[1] = g.jpeg.allocations;
    out[2] = g.jpeg.hostWaits;
    out[3] = g.jpeg.bytesDelivered;
}

} /* extern "C" */
