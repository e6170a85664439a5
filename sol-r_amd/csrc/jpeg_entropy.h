/*
 * jpeg_entropy.h - the entropy stage of the JPEG writer: quantised coefficient blocks in zigzag order, as the pixel stage
 * (jpeg_encode.h) leaves them, to the entropy-coded segment of a baseline file.  Integer arithmetic only, written once for
 * both sides: the host-only engine runs it in loops (host/JpegWriter.cpp, JpegWriter::scan), the HIP engine in kernels
 * (csrc/solr_jpeg_entropy.hip).
 *
 * The bytes are those of the reference encoder's one-pass coder, solr/images/jpge.cpp: put_bits (:817-835),
 * code_coefficients_pass_two (:883-952) and terminate_pass_two (:1032-1039).  That coder walks the blocks once with a bit
 * buffer; here the same stream is made in steps none of which depends on the block before it:
 *   bits      blockBits: how many bits each block takes
 *   prefix    exclusiveSum of them: the bit offset of every block, 64 bits wide
 *   emit      blockEmit: every block at its offset of an UNSTUFFED stream of 32-bit words (bit 31 of word 0 is the first
 *             bit).  Neighbours share words; bits only ever go in by OR, which commutes
 *   tail      tailBits: the one-bits that complete a started last byte
 *   count     countFF: the 0xFF bytes of every chunk of the unstuffed stream; exclusiveSum of those
 *   stuff     stuffWord: every chunk to its offset plus the number of 0xFF before it, a zero byte behind each 0xFF
 * tests/golden/jpeg_encoder.npz holds jpge's own files; tests/test_jpeg_entropy.py holds the steps to them and to the
 * one-pass writer (JpegWriter::encode).
 *
 * The tables are the four standard ones, or - the reference encoder's two-pass mode, see "optimised tables" below - four
 * built for the symbols of the blocks themselves: a census by the same walk (blockCensus), optimiseTable per table, and the
 * steps above with the result as their tables.  tests/golden/jpeg_two_pass.npz holds jpge's own tables and two-pass files;
 * tests/test_jpeg_two_pass.py holds census, builder and writer to them.
 *
 * The domain is what the four standard tables can code: a DC difference of category 0 ... 11 (|d| <= 2047) and AC
 * coefficients of category 1 ... 10 (|a| <= 1023).  blockBits reports a block outside it.  The pixel stage cannot make
 * one: its forward DCT is the orthonormal one (DC = sum / 8) of samples - 128 in -128 ... 127, so a DC lies in
 * -1024 ... 1016 and two of them differ by at most 2040; an AC output is at most 128 * (sum over x of |cos((2x + 1) u pi / 16)|
 * / 2)^2 <= 128 * (5.126 / 2)^2 = 841 for u, v > 0 and 128 * 8 * 5.126 / (4 * sqrt(2)) = 928 in row or column 0, and the
 * rounding of the fixed-point passes adds a few units; quantisation divides by at least 1.  Blocks from elsewhere
 * (SolRx_JpegFileFromCoefficients, solr_hip_jpeg_blocks_to_scan) are checked.
 */
#pragma once

#include "jpeg_encode.h"

namespace jpn
{
typedef unsigned int u32;
typedef unsigned long long u64;
typedef unsigned char u8;

/* The granularities of the device's kernels, for the tests to put block counts and stream lengths around.  (The two
 * prefix sums are hipcub's DeviceScan, as in solr_iso.hip: its tile is the library's, not a constant of this stage.) */
constexpr int BLOCKS_PER_GROUP = 64;   /* blocks one workgroup assembles in LDS, one per lane */
constexpr int STUFF_CHUNK_BYTES = 256; /* unstuffed bytes one workgroup counts and scatters, one word per lane */

/* ITU T.81 tables K.3 - K.6: the number of codes of each length 1..16, then the symbols in code order */
constexpr u8 DC_LUMA_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr u8 DC_CHROMA_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr u8 DC_VALUES[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr u8 AC_LUMA_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr u8 AC_LUMA_VALUES[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr u8 AC_CHROMA_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr u8 AC_CHROMA_VALUES[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

constexpr int MAX_DC_CATEGORY = 11, MAX_AC_CATEGORY = 10;
constexpr int EOB = 0x00, ZRL = 0xF0;

/* code and length per symbol of the four tables, luma then chroma: code | length << 16 (a length of 0: no such symbol) */
struct Tables
{
    u32 dc[2][12];
    u32 ac[2][256];
};

/* annex C: codes of one length count upwards, the next length continues from twice the last code + 2 (the rule of
 * JpegWriter.cpp's tables before this header took them over) */
constexpr void fillTable(const u8 bits[16], const u8 *values, u32 *entries)
{
    u32 next = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l)
    {
        for (int i = 0; i < bits[l - 1]; ++i, ++k)
            entries[values[k]] = next++ | ((u32)l << 16);
        next <<= 1;
    }
}

constexpr Tables makeTables()
{
    Tables t = {};
    fillTable(DC_LUMA_BITS, DC_VALUES, t.dc[0]);
    fillTable(DC_CHROMA_BITS, DC_VALUES, t.dc[1]);
    fillTable(AC_LUMA_BITS, AC_LUMA_VALUES, t.ac[0]);
    fillTable(AC_CHROMA_BITS, AC_CHROMA_VALUES, t.ac[1]);
    return t;
}

/* The most bits a block can take.  DC: the longest code plus its amplitude.  AC: every one of the 63 positions holds a
 * coefficient with the longest code plus amplitude - a zero costs less: sixteen of them are one ZRL, and the end of block
 * is not coded when position 63 is taken.  A bound, 1660: its DC term is the chroma tables' (11 + 11) and its AC term the
 * luma tables' (16 + 10), so the longest block there is is a luma block of 20 + 63 * 26 = 1658 bits. */
constexpr int maxBlockBits(const Tables &t)
{
    int dc = 0, ac = 0;
    for (int table = 0; table < 2; ++table)
    {
        for (int size = 0; size <= MAX_DC_CATEGORY; ++size)
            if ((int)(t.dc[table][size] >> 16) + size > dc)
                dc = (int)(t.dc[table][size] >> 16) + size;
        for (int run = 0; run < 16; ++run)
            for (int size = 1; size <= MAX_AC_CATEGORY; ++size)
                if ((int)(t.ac[table][(run << 4) + size] >> 16) + size > ac)
                    ac = (int)(t.ac[table][(run << 4) + size] >> 16) + size;
    }
    return dc + 63 * ac;
}
constexpr int MAX_BLOCK_BITS = 22 + 63 * 26;
static_assert(maxBlockBits(makeTables()) == MAX_BLOCK_BITS && MAX_BLOCK_BITS == 1660, "the standard tables' longest block");
/* ... and a ZRL or an EOB must not cost more than the coefficients they stand for could */
static_assert((makeTables().ac[0][ZRL] >> 16) <= 26 && (makeTables().ac[1][ZRL] >> 16) <= 26 &&
                  (makeTables().ac[0][EOB] >> 16) <= 26 && (makeTables().ac[1][EOB] >> 16) <= 26,
              "run symbols are shorter than a coefficient");

/* ... and with ANY table whose codes have at most 16 bits (an optimised one): the DC of category 11 may have a 16-bit
 * code too.  The same two static conditions hold of any such table: a run symbol's 16 bits are fewer than 26 */
constexpr int MAX_CODE_BITS = 16;
constexpr int MAX_BLOCK_BITS_ANY_TABLE = (MAX_CODE_BITS + MAX_DC_CATEGORY) + 63 * (MAX_CODE_BITS + MAX_AC_CATEGORY);
static_assert(MAX_BLOCK_BITS_ANY_TABLE == 1665 && MAX_BLOCK_BITS_ANY_TABLE >= MAX_BLOCK_BITS, "any table's longest block");

JPE_HD inline const Tables &tables()
{
    static constexpr Tables t = makeTables();
    return t;
}

/* ---- which block precedes which ------------------------------------------------------------------------------------- */
/* The blocks come MCU by MCU, inside an MCU the lumaBlocks (1, 2 or 4) luma blocks, then Cb, then Cr
 * (solr_hip_rgb_to_jpeg_blocks).  0 for luma, 1 for chroma: the tables of block `index` */
JPE_HD inline int chromaOf(long index, int lumaBlocks)
{
    return (int)(index % (lumaBlocks + 2)) >= lumaBlocks ? 1 : 0;
}
/* the block whose DC the DC of block `index` is coded against - the last block of the same component (jpge.cpp:883-900,
 * m_last_dc_val per component) - or -1 for the first of each */
JPE_HD inline long predecessor(long index, int lumaBlocks)
{
    const int perMcu = lumaBlocks + 2;
    const long mcu = index / perMcu;
    const int within = (int)(index - mcu * perMcu);
    if (within > 0 && within < lumaBlocks)
        return index - 1;
    if (mcu == 0)
        return -1;
    return within == 0 ? index - 3 : index - perMcu; /* the last luma block of the MCU before; the same chroma block of it */
}

/* ---- one block ------------------------------------------------------------------------------------------------------ */
JPE_HD inline int bitLength(int magnitude)
{
    return magnitude ? 32 - __builtin_clz((unsigned)magnitude) : 0;
}

/* F.1.2.1 / F.1.2.2: the low `size` bits of the value, of the value - 1 when it is negative */
JPE_HD inline u32 amplitude(int value, int size)
{
    return (u32)(value < 0 ? value - 1 : value) & ((1u << size) - 1u);
}

/* The walk over a block (jpge.cpp:883-952; the same decisions as its census, code_coefficients_pass_one, :837-881),
 * handing every symbol to the visitor: dc(category, difference), then ac(symbol, category, value) per (run, size) symbol
 * - and per ZRL and EOB, with category 0 and value 0.  Returns whether the block is inside the domain; outside it the
 * category is held at the tables' last, so that every walk takes the same symbols whoever visits. */
template <class Visitor>
JPE_HD inline bool walkSymbols(const short *block, int previousDc, Visitor &visitor)
{
    bool inside = true;
    const int difference = block[0] - previousDc;
    int size = bitLength(difference < 0 ? -difference : difference);
    if (size > MAX_DC_CATEGORY)
    {
        inside = false;
        size = MAX_DC_CATEGORY;
    }
    visitor.dc(size, difference);
    int run = 0;
    for (int k = 1; k < 64; ++k)
    {
        const int value = block[k];
        if (value == 0)
        {
            ++run;
            continue;
        }
        for (; run >= 16; run -= 16)
            visitor.ac(ZRL, 0, 0);
        size = bitLength(value < 0 ? -value : value);
        if (size > MAX_AC_CATEGORY)
        {
            inside = false;
            size = MAX_AC_CATEGORY;
        }
        visitor.ac((run << 4) + size, size, value);
        run = 0;
    }
    if (run)
        visitor.ac(EOB, 0, 0);
    return inside;
}

/* a visitor that codes: the symbol's code from the tables `t`, the amplitude behind it - at most 16 + 11 bits - to
 * sink.put(bits, n) */
template <class Sink>
struct Coder
{
    const Tables &t;
    int chroma;
    Sink &sink;
    JPE_HD void dc(int size, int difference)
    {
        const u32 entry = t.dc[chroma][size];
        sink.put(((entry & 0xffffu) << size) | amplitude(difference, size), (int)(entry >> 16) + size);
    }
    JPE_HD void ac(int symbol, int size, int value)
    {
        const u32 entry = t.ac[chroma][symbol];
        sink.put(((entry & 0xffffu) << size) | amplitude(value, size), (int)(entry >> 16) + size);
    }
};

/* The walk with the tables of a provider: tables() for the four standard ones, or tables that came as data (an optimised
 * set, on the device its copy in LDS) */
template <class Sink>
JPE_HD inline bool walkBlock(const Tables &t, const short *block, int previousDc, int chroma, Sink &sink)
{
    Coder<Sink> coder = {t, chroma, sink};
    return walkSymbols(block, previousDc, coder);
}
template <class Sink>
JPE_HD inline bool walkBlock(const short *block, int previousDc, int chroma, Sink &sink)
{
    return walkBlock(tables(), block, previousDc, chroma, sink);
}

struct BitCounter
{
    u32 bits = 0;
    JPE_HD void put(u32, int n) { bits += (u32)n; }
};

/* bits: DC category and amplitude, a ZRL per sixteen zeros in front of a coefficient, a symbol and an amplitude per
 * coefficient, EOB unless position 63 is taken; at most MAX_BLOCK_BITS with the standard tables, MAX_BLOCK_BITS_ANY_TABLE
 * with any.  false: the block is outside the domain */
JPE_HD inline bool blockBits(const Tables &t, const short *block, int previousDc, int chroma, u32 *bits)
{
    BitCounter counter;
    const bool inside = walkBlock(t, block, previousDc, chroma, counter);
    *bits = counter.bits;
    return inside;
}
JPE_HD inline bool blockBits(const short *block, int previousDc, int chroma, u32 *bits)
{
    return blockBits(tables(), block, previousDc, chroma, bits);
}

/* the two words that n (1 ... 32) bits at bit offset `at` of the stream touch, and what goes into each */
JPE_HD inline void placeBits(u64 at, u32 bits, int n, u64 *word, u32 *first, u32 *second)
{
    const u64 window = (u64)bits << (64 - n - (int)(at & 31u));
    *word = at >> 5;
    *first = (u32)(window >> 32);
    *second = (u32)window;
}

struct WordWriter
{
    u32 *words;
    u64 at;
    JPE_HD void put(u32 bits, int n)
    {
        u64 word;
        u32 first, second;
        placeBits(at, bits, n, &word, &first, &second);
        words[word] |= first;
        if (second)
            words[word + 1] |= second;
        at += (u64)n;
    }
};

/* the same walk, the bits ORed into `words` from bit offset `at` on */
JPE_HD inline void blockEmit(const Tables &t, const short *block, int previousDc, int chroma, u64 at, u32 *words)
{
    WordWriter writer = {words, at};
    walkBlock(t, block, previousDc, chroma, writer);
}
JPE_HD inline void blockEmit(const short *block, int previousDc, int chroma, u64 at, u32 *words)
{
    blockEmit(tables(), block, previousDc, chroma, at, words);
}

/* ---- optimised tables ------------------------------------------------------------------------------------------------ */
/* The reference encoder's two-pass mode (jpge.cpp, params::m_two_pass_flag): the symbols of the picture are counted
 * (code_coefficients_pass_one, :837-881), four tables are built for exactly those counts (optimize_huffman_table, :353-397)
 * and written in the file's DHT segments, and the blocks are coded with them.  Restated here in steps that the host runs
 * in loops and the device in lanes; tests/golden/jpeg_two_pass.npz holds jpge's own tables and files. */

/* how often every symbol of the four tables occurs: the shape of Tables, a counter where that has a code */
struct Census
{
    u32 dc[2][12];
    u32 ac[2][256];
};
constexpr int CENSUS_COUNTERS = 2 * 12 + 2 * 256;
static_assert(sizeof(Census) == CENSUS_COUNTERS * sizeof(u32) && sizeof(Tables) == sizeof(Census), "counters as entries");

struct Counter
{
    Census &census;
    int chroma;
    JPE_HD void dc(int size, int) { ++census.dc[chroma][size]; }
    JPE_HD void ac(int symbol, int, int) { ++census.ac[chroma][symbol]; }
};

/* the symbols of one block added to `census`: the walk of blockBits, so what is counted is what will be coded.  false:
 * the block is outside the domain (its symbols are counted as the walk holds them) */
JPE_HD inline bool blockCensus(const short *block, int previousDc, int chroma, Census &census)
{
    Counter counter = {census, chroma};
    return walkSymbols(block, previousDc, counter);
}

/* The four tables of a file in the order of its DHT segments (jpge.cpp:486-495): DC luma, AC luma, DC chroma, AC chroma.
 * bits: the number of codes of each length 1 ... 16; values: the symbols in code order, nbValues of them */
constexpr int TABLE_SLOTS = 4;
struct Huffman
{
    u8 bits[TABLE_SLOTS][16];
    u8 values[TABLE_SLOTS][256];
    int nbValues[TABLE_SLOTS];
};
JPE_HD inline int slotIsAc(int slot) { return slot & 1; }
JPE_HD inline int slotChroma(int slot) { return slot >> 1; }
JPE_HD inline int slotLength(int slot) { return slotIsAc(slot) ? 256 : 12; } /* DC_LUM_CODES, AC_LUM_CODES */
JPE_HD inline const u32 *slotCounts(const Census &census, int slot)
{
    return slotIsAc(slot) ? census.ac[slotChroma(slot)] : census.dc[slotChroma(slot)];
}
JPE_HD inline u32 *slotEntries(Tables &t, int slot)
{
    return slotIsAc(slot) ? t.ac[slotChroma(slot)] : t.dc[slotChroma(slot)];
}

/* jpge sorts the used symbols by count with an LSD radix sort (radix_sort_syms, :226-264), which is stable, over the
 * symbols in index order behind a dummy of count 1 (:356-365): the order of (count, index) pairs, the dummy - whose count
 * no used symbol's is below - first.  The place of used symbol i behind the dummy: the used symbols whose pair is below
 * its own.  (Ties and the dummy's place decide bytes.) */
constexpr int MAX_TABLE_SYMBOLS = 1 + 256; /* the dummy and a whole AC table */
JPE_HD inline int symbolRank(const u32 *counts, int tableLen, int i)
{
    const u32 mine = counts[i];
    int below = 0;
    for (int j = 0; j < tableLen; ++j)
    {
        const u32 other = counts[j];
        below += (other != 0u && (other < mine || (other == mine && j < i))) ? 1 : 0;
    }
    return below;
}

/* calculate_minimum_redundancy (:266-321; Moffat and Katajainen, "In-place calculation of minimum-redundancy codes",
 * 1995): a[0 ... n - 1] holds counts in ascending order and receives the code length of each.  Three passes in place:
 * the tree's internal nodes with parent links, the internal nodes' depths, the leaves' depths. */
JPE_HD inline void codeLengths(u32 *a, int n)
{
    if (n == 0)
        return;
    if (n == 1)
    {
        a[0] = 1;
        return;
    }
    a[0] += a[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next)
    {
        /* the two smallest of the unused leaves and the unlinked internal nodes, a leaf on a tie */
        if (leaf >= n || a[root] < a[leaf])
        {
            a[next] = a[root];
            a[root++] = (u32)next;
        }
        else
            a[next] = a[leaf++];
        if (leaf >= n || (root < next && a[root] < a[leaf]))
        {
            a[next] += a[root];
            a[root++] = (u32)next;
        }
        else
            a[next] += a[leaf++];
    }
    a[n - 2] = 0;
    for (int next = n - 3; next >= 0; --next)
        a[next] = a[a[next]] + 1;
    int available = 1, used = 0, depth = 0, next = n - 1;
    root = n - 2;
    while (available > 0)
    {
        while (root >= 0 && (int)a[root] == depth)
        {
            ++used;
            --root;
        }
        while (available > used)
        {
            a[next--] = (u32)depth;
            --available;
        }
        available = 2 * used;
        ++depth;
        used = 0;
    }
}

/* huffman_enforce_max_code_size (:323-350) with the limit of 16: numCodes[l] codes of length l, l up to n - 1 for n
 * symbols.  The longer ones are counted as 16 bits; while the Kraft sum is above one, a code of 16 bits goes and the
 * longest code below 16 bits becomes two one bit longer */
JPE_HD inline void limitCodeLengths(int *numCodes, int n)
{
    if (n <= 1)
        return;
    for (int l = MAX_CODE_BITS + 1; l < MAX_TABLE_SYMBOLS; ++l)
    {
        numCodes[MAX_CODE_BITS] += numCodes[l];
        numCodes[l] = 0;
    }
    u32 total = 0;
    for (int l = MAX_CODE_BITS; l > 0; --l)
        total += (u32)numCodes[l] << (MAX_CODE_BITS - l);
    for (; total != (1u << MAX_CODE_BITS); --total)
    {
        --numCodes[MAX_CODE_BITS];
        for (int l = MAX_CODE_BITS - 1; l > 0; --l)
            if (numCodes[l])
            {
                --numCodes[l];
                numCodes[l + 1] += 2;
                break;
            }
    }
}

/* :367-392 - sorted[0 ... n - 1]: the counts in sorted order, the dummy's 1 first; numCodes: MAX_TABLE_SYMBOLS ints of
 * room.  bits[l - 1] = the codes of length l, the dummy - which is in the longest occupied length, so that no symbol's
 * code is all ones - taken out */
JPE_HD inline void bitsOfSorted(u32 *sorted, int n, int *numCodes, u8 bits[16])
{
    codeLengths(sorted, n);
    for (int l = 0; l < MAX_TABLE_SYMBOLS; ++l)
        numCodes[l] = 0;
    for (int i = 0; i < n; ++i)
        ++numCodes[sorted[i]];
    limitCodeLengths(numCodes, n);
    for (int l = 1; l <= MAX_CODE_BITS; ++l)
        bits[l - 1] = (u8)numCodes[l];
    for (int l = MAX_CODE_BITS; l >= 1; --l)
        if (bits[l - 1])
        {
            --bits[l - 1];
            break;
        }
}

/* optimize_huffman_table (:353-397) for counts[0 ... tableLen - 1], tableLen at most 256: bits[16] and the values - the
 * sorted symbols without the dummy, the most frequent first (:394-396).  Returns how many values there are: the symbols
 * with a count */
inline int optimiseTable(const u32 *counts, int tableLen, u8 bits[16], u8 *values)
{
    u32 sorted[MAX_TABLE_SYMBOLS];
    int numCodes[MAX_TABLE_SYMBOLS];
    int n = 1;
    for (int i = 0; i < tableLen; ++i)
        n += counts[i] ? 1 : 0;
    sorted[0] = 1;
    for (int i = 0; i < tableLen; ++i)
        if (counts[i])
        {
            const int at = 1 + symbolRank(counts, tableLen, i);
            sorted[at] = counts[i];
            values[n - 1 - at] = (u8)i;
        }
    bitsOfSorted(sorted, n, numCodes, bits);
    return n - 1;
}

/* the four tables of a census (:1022-1027) */
inline void optimiseTables(const Census &census, Huffman &huffman)
{
    for (int slot = 0; slot < TABLE_SLOTS; ++slot)
        huffman.nbValues[slot] = optimiseTable(slotCounts(census, slot), slotLength(slot), huffman.bits[slot],
                                               huffman.values[slot]);
}

/* code and length per symbol of tables that came as data (compute_huffman_table, :528-562) */
inline void tablesOf(const Huffman &huffman, Tables &t)
{
    t = Tables();
    for (int slot = 0; slot < TABLE_SLOTS; ++slot)
        fillTable(huffman.bits[slot], huffman.values[slot], slotEntries(t, slot));
}

/* ---- the end of the stream -------------------------------------------------------------------------------------------- */
/* jpge.cpp:1032-1039, put_bits(0x7F, 7): a started last byte is completed with one-bits, a complete one gets nothing.  How
 * many one-bits follow a stream of totalBits; the completed byte is stuffed like any other when it comes out as 0xFF */
JPE_HD inline int tailBits(u64 totalBits)
{
    return (int)((8u - (u32)(totalBits & 7u)) & 7u);
}
JPE_HD inline u64 streamBytes(u64 totalBits)
{
    return (totalBits + 7u) >> 3;
}
JPE_HD inline u64 streamWords(u64 totalBits)
{
    return (totalBits + 31u) >> 5;
}

/* ---- stuffing --------------------------------------------------------------------------------------------------------- */
/* byte j of the stream is bits 31 - 8 (j & 3) ... 24 - 8 (j & 3) of word j >> 2.  The 0xFF among the first nbBytes (0 ... 4)
 * bytes of a word */
JPE_HD inline u32 countFF(u32 word, int nbBytes)
{
    u32 n = 0;
    for (int i = 0; i < nbBytes; ++i)
        n += ((word >> (24 - 8 * i)) & 0xffu) == 0xffu ? 1u : 0u;
    return n;
}
/* those bytes to `to`, a zero behind every 0xFF (B.1.1.5); returns how many were written: nbBytes + countFF */
JPE_HD inline u32 stuffWord(u32 word, int nbBytes, u8 *to)
{
    u32 n = 0;
    for (int i = 0; i < nbBytes; ++i)
    {
        const u8 b = (u8)(word >> (24 - 8 * i));
        to[n++] = b;
        if (b == 0xffu)
            to[n++] = 0;
    }
    return n;
}
/* how many of the stream's nbBytes bytes word `index` holds */
JPE_HD inline int bytesOfWord(u64 index, u64 nbBytes)
{
    const u64 from = index * 4u;
    return from >= nbBytes ? 0 : (nbBytes - from < 4u ? (int)(nbBytes - from) : 4);
}

/* ---- the plan of a resident pipeline ---------------------------------------------------------------------------------- */
/* A pipeline that keeps its buffers and never asks the device how far it got (csrc/solr_jpeg_entropy.hip, the slots of
 * solr_hip_frame_to_jpeg_async) sizes buffers and launches by what the host knows - the number of blocks - and lets one
 * step on the device turn the prefix sum's total into the extents the later steps read.  What a frame of nbBlocks blocks
 * can take with ANY table of 16-bit codes: so many bits unstuffed (the tail's seven included), so many bytes, so many
 * chunks, and twice the bytes stuffed (every byte a 0xFF).  No frame inside the domain is larger: there is no overflow */
JPE_HD inline u64 maxStreamBits(long nbBlocks)
{
    return (u64)nbBlocks * (u64)MAX_BLOCK_BITS_ANY_TABLE + 7u;
}
JPE_HD inline u64 chunksOf(u64 nbBytes)
{
    return (nbBytes + (u64)STUFF_CHUNK_BYTES - 1u) / (u64)STUFF_CHUNK_BYTES;
}
JPE_HD inline u64 maxStreamBytes(long nbBlocks) { return streamBytes(maxStreamBits(nbBlocks)); }
JPE_HD inline u64 maxStreamChunks(long nbBlocks) { return chunksOf(maxStreamBytes(nbBlocks)); }
JPE_HD inline u64 maxStuffedBytes(long nbBlocks) { return 2u * maxStreamBytes(nbBlocks); }

/* what the steps behind the prefix sum read in place of arguments the host would have had to wait for */
struct ScanPlan
{
    u64 totalBits;      /* of the blocks, without the tail */
    u64 unstuffedBytes; /* streamBytes(totalBits): the tail completes the last one */
    u64 streamWords;    /* the words of the unstuffed stream the emit step touches: those the stuff step reads */
    u64 nbChunks;       /* chunks of STUFF_CHUNK_BYTES that hold a byte */
    u32 flag;           /* a block is outside the domain: every extent above is 0, the later steps write nothing */
    u32 pad;
};
JPE_HD inline ScanPlan planScan(u64 totalBits, u32 flag)
{
    ScanPlan plan = {0, 0, 0, 0, flag ? 1u : 0u, 0};
    if (flag)
        return plan;
    plan.totalBits = totalBits;
    plan.unstuffedBytes = streamBytes(totalBits);
    plan.streamWords = streamWords(totalBits + (u64)tailBits(totalBits));
    plan.nbChunks = chunksOf(plan.unstuffedBytes);
    return plan;
}
/* bytesOfWord with the extent from the plan: a word of a chunk beyond it holds none */
JPE_HD inline int planBytesOfWord(const ScanPlan &plan, u64 index)
{
    return index / (u64)(STUFF_CHUNK_BYTES / 4) >= plan.nbChunks ? 0 : bytesOfWord(index, plan.unstuffedBytes);
}
/* the count and the stuff step of one chunk with the extent from the plan, as loops (the device: a lane per word).
 * chunkCountFF: the 0xFF bytes of the chunk, 0 beyond the extent.  chunkStuff: the chunk's bytes to `out` at the chunk's
 * offset plus `before` (the 0xFF of the chunks in front), nothing beyond the extent; clearBehind: every word read is left
 * zero, so that the stream a resident buffer holds is zero again for the next emit step - the work follows the file */
inline u64 chunkCountFF(const u32 *stream, const ScanPlan &plan, u64 chunk)
{
    u64 n = 0;
    for (u64 index = chunk * (STUFF_CHUNK_BYTES / 4); index < (chunk + 1) * (STUFF_CHUNK_BYTES / 4); ++index)
        if (const int bytes = planBytesOfWord(plan, index))
            n += countFF(stream[index], bytes);
    return n;
}
inline void chunkStuff(u32 *stream, const ScanPlan &plan, u64 chunk, u64 before, u8 *out, bool clearBehind)
{
    u64 at = chunk * (u64)STUFF_CHUNK_BYTES + before;
    for (u64 index = chunk * (STUFF_CHUNK_BYTES / 4); index < (chunk + 1) * (STUFF_CHUNK_BYTES / 4); ++index)
        if (const int bytes = planBytesOfWord(plan, index))
        {
            at += stuffWord(stream[index], bytes, out + at);
            if (clearBehind)
                stream[index] = 0;
        }
}

/* ---- prefix sums ------------------------------------------------------------------------------------------------------ */
/* offsets[i] = lengths[0] + ... + lengths[i - 1] for i = 0 ... n (n + 1 results, the last the total), 64 bits wide:
 * SOLR_JPEG_MAX_PIXELS is 2^26 pixels, 1.5 M blocks of up to 1660 bits pass 2^32 */
inline void exclusiveSum(const u32 *lengths, long n, u64 *offsets)
{
    u64 sum = 0;
    for (long i = 0; i < n; ++i)
    {
        offsets[i] = sum;
        sum += lengths[i];
    }
    offsets[n] = sum;
}
} // namespace jpn
