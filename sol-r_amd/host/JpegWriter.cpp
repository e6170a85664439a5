/*
 * JpegWriter.cpp - see JpegWriter.h.  The stream follows ITU T.81 (markers B.2, Huffman tables annex C and K.3, the
 * coding of a block F.1.2); where the standard leaves a choice the reference's jpge.cpp is followed, line numbers below.
 */
#include "JpegWriter.h"

#include <cstdio>
#include <memory>

#include "../csrc/jpeg_entropy.h"

namespace solr
{
namespace
{
typedef unsigned char u8;

/* ITU T.81 tables K.3 - K.6 (csrc/jpeg_entropy.h has them, for the decomposed coder too) */
using jpn::AC_CHROMA_BITS;
using jpn::AC_CHROMA_VALUES;
using jpn::AC_LUMA_BITS;
using jpn::AC_LUMA_VALUES;
using jpn::DC_CHROMA_BITS;
using jpn::DC_LUMA_BITS;
using jpn::DC_VALUES;

struct HuffmanTable
{
    const u8 *bits, *values;
    int nbValues;
    unsigned code[256];
    u8 length[256];

    /* annex C: codes of one length count upwards, the next length continues from twice the last code + 2 */
    HuffmanTable(const u8 *b, const u8 *v, int n) : bits(b), values(v), nbValues(n), code(), length()
    {
        unsigned next = 0;
        int k = 0;
        for (int l = 1; l <= 16; ++l)
        {
            for (int i = 0; i < bits[l - 1]; ++i, ++k)
            {
                code[values[k]] = next++;
                length[values[k]] = (u8)l;
            }
            next <<= 1;
        }
    }
};

struct Stream
{
    std::vector<u8> out;
    unsigned buffer = 0; /* the bits not yet written, from bit 23 downwards (jpge.cpp:817-835) */
    int bitsIn = 0;

    void byte(int b) { out.push_back((u8)b); }
    void word(int w)
    {
        byte(w >> 8);
        byte(w & 0xFF);
    }
    void marker(int m)
    {
        byte(0xFF);
        byte(m);
    }
    /* at most 16 bits at a time; a zero byte follows every 0xFF of the entropy-coded segment (B.1.1.5) */
    void put(unsigned bits, int n)
    {
        bitsIn += n;
        buffer |= bits << (24 - bitsIn);
        while (bitsIn >= 8)
        {
            const u8 b = (u8)((buffer >> 16) & 0xFF);
            out.push_back(b);
            if (b == 0xFF)
                out.push_back(0);
            buffer <<= 8;
            bitsIn -= 8;
        }
    }
    void symbol(const HuffmanTable &t, int s) { put(t.code[s], t.length[s]); }
};

inline int bitLength(int magnitude)
{
    int n = 0;
    while (magnitude)
    {
        ++n;
        magnitude >>= 1;
    }
    return n;
}

/* F.1.2.1 / F.1.2.2: the low `size` bits of the value, of the value - 1 when it is negative */
inline void amplitude(Stream &s, int value, int size)
{
    s.put((unsigned)(value < 0 ? value - 1 : value) & ((1u << size) - 1u), size);
}

void table(Stream &s, const HuffmanTable &t, int index)
{
    s.marker(0xC4);
    s.word(2 + 1 + 16 + t.nbValues);
    s.byte(index);
    for (int i = 0; i < 16; ++i)
        s.byte(t.bits[i]);
    for (int i = 0; i < t.nbValues; ++i)
        s.byte(t.values[i]);
}

const HuffmanTable &dcTable(int chroma)
{
    static const HuffmanTable dc[2] = {HuffmanTable(DC_LUMA_BITS, DC_VALUES, 12), HuffmanTable(DC_CHROMA_BITS, DC_VALUES, 12)};
    return dc[chroma];
}
const HuffmanTable &acTable(int chroma)
{
    static const HuffmanTable ac[2] = {HuffmanTable(AC_LUMA_BITS, AC_LUMA_VALUES, 162),
                                       HuffmanTable(AC_CHROMA_BITS, AC_CHROMA_VALUES, 162)};
    return ac[chroma];
}

/* the tables of an optimised file, in the order of its DHT segments */
struct OptimisedTables
{
    HuffmanTable dc[2], ac[2];
    explicit OptimisedTables(const jpn::Huffman &h)
        : dc{HuffmanTable(h.bits[0], h.values[0], h.nbValues[0]), HuffmanTable(h.bits[2], h.values[2], h.nbValues[2])},
          ac{HuffmanTable(h.bits[1], h.values[1], h.nbValues[1]), HuffmanTable(h.bits[3], h.values[3], h.nbValues[3])}
    {
    }
};

void headerInto(Stream &s, int width, int height, int lumaH, int lumaV, const unsigned short quant[2][64],
                const HuffmanTable *dc, const HuffmanTable *ac)
{
    /* jpge.cpp:517-525 emit_markers */
    s.marker(0xD8);
    s.marker(0xE0); /* JFIF 1.1, no density unit, aspect 1:1, no thumbnail (:418-434) */
    s.word(16);
    for (const char *c = "JFIF"; *c; ++c)
        s.byte(*c);
    s.byte(0);
    s.byte(1);
    s.byte(1);
    s.byte(0);
    s.word(1);
    s.word(1);
    s.byte(0);
    s.byte(0);
    for (int i = 0; i < 2; ++i) /* one segment per table, 8-bit entries in zigzag order (:437-447) */
    {
        s.marker(0xDB);
        s.word(64 + 1 + 2);
        s.byte(i);
        for (int k = 0; k < 64; ++k)
            s.byte(quant[i][k]);
    }
    s.marker(0xC0); /* baseline, 8 bits, three components, chroma 1x1 with table 1 (:450-464) */
    s.word(3 * 3 + 2 + 5 + 1);
    s.byte(8);
    s.word(height);
    s.word(width);
    s.byte(3);
    for (int c = 0; c < 3; ++c)
    {
        s.byte(c + 1);
        s.byte(c == 0 ? (lumaH << 4) + lumaV : 0x11);
        s.byte(c > 0);
    }
    table(s, dc[0], 0x00); /* :486-495 */
    table(s, ac[0], 0x10);
    table(s, dc[1], 0x01);
    table(s, ac[1], 0x11);
    s.marker(0xDA); /* :498-514 */
    s.word(2 * 3 + 2 + 1 + 3);
    s.byte(3);
    for (int c = 0; c < 3; ++c)
    {
        s.byte(c + 1);
        s.byte(c == 0 ? 0x00 : 0x11);
    }
    s.byte(0);
    s.byte(63);
    s.byte(0);
}
}

std::vector<unsigned char> JpegWriter::header(int width, int height, int lumaH, int lumaV,
                                              const unsigned short quant[2][64], const jpn::Huffman *tables)
{
    Stream s;
    if (tables)
    {
        const OptimisedTables optimised(*tables);
        headerInto(s, width, height, lumaH, lumaV, quant, optimised.dc, optimised.ac);
    }
    else
        headerInto(s, width, height, lumaH, lumaV, quant, &dcTable(0), &acTable(0));
    return s.out;
}

std::vector<unsigned char> JpegWriter::encode(int width, int height, int lumaH, int lumaV,
                                              const unsigned short quant[2][64], const short *blocks, long nbBlocks,
                                              bool optimise)
{
    const int lumaBlocks = lumaH * lumaV, perMcu = lumaBlocks + 2;
    const HuffmanTable *dc = &dcTable(0), *ac = &acTable(0);
    std::unique_ptr<OptimisedTables> optimised;
    jpn::Huffman huffman; /* (the tables point into it) */
    if (optimise)
    {
        /* the first pass (:837-881, :1022-1027): the census with one predictor per component, as the second pass codes */
        jpn::Census census = {};
        int lastDc[3] = {0, 0, 0};
        for (long index = 0; index < nbBlocks; ++index)
        {
            const int inMcu = (int)(index % perMcu);
            const int c = inMcu < lumaBlocks ? 0 : inMcu - lumaBlocks + 1;
            jpn::blockCensus(blocks + index * 64, lastDc[c], c > 0, census);
            lastDc[c] = blocks[index * 64];
        }
        jpn::optimiseTables(census, huffman);
        optimised.reset(new OptimisedTables(huffman));
        dc = optimised->dc;
        ac = optimised->ac;
    }
    Stream s;
    s.out.reserve(1024 + (size_t)nbBlocks * 32);
    headerInto(s, width, height, lumaH, lumaV, quant, dc, ac);

    /* the scan: :883-952 */
    int lastDc[3] = {0, 0, 0};
    int inMcu = 0;
    for (long index = 0; index < nbBlocks; ++index)
    {
        const short *block = blocks + index * 64;
        const int c = inMcu < lumaBlocks ? 0 : inMcu - lumaBlocks + 1;
        if (++inMcu == perMcu)
            inMcu = 0;
        const HuffmanTable &d = dc[c > 0], &a = ac[c > 0];
        const int difference = block[0] - lastDc[c];
        lastDc[c] = block[0];
        int size = bitLength(difference < 0 ? -difference : difference);
        s.symbol(d, size);
        if (size)
            amplitude(s, difference, size);
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
                s.symbol(a, 0xF0);
            size = bitLength(value < 0 ? -value : value);
            s.symbol(a, (run << 4) + size);
            amplitude(s, value, size);
            run = 0;
        }
        if (run)
            s.symbol(a, 0x00);
    }
    /* :1032-1039: seven one bits complete the last byte (none is written when it is complete already) */
    s.put(0x7F, 7);
    s.marker(0xD9);
    return s.out;
}

/* The same segment in the order the device takes (csrc/jpeg_entropy.h): every loop below runs over independent items */
bool JpegWriter::scan(int lumaH, int lumaV, const short *blocks, long nbBlocks, std::vector<unsigned char> &out,
                      jpn::Huffman *optimised)
{
    const int lumaBlocks = lumaH * lumaV;
    auto previousDc = [&](long index) {
        const long before = jpn::predecessor(index, lumaBlocks);
        return before < 0 ? 0 : (int)blocks[before * 64];
    };
    /* census, tables: only for an optimised file */
    jpn::Tables own;
    jpn::Huffman huffman;
    if (optimised)
    {
        jpn::Census census = {};
        for (long i = 0; i < nbBlocks; ++i)
            jpn::blockCensus(blocks + i * 64, previousDc(i), jpn::chromaOf(i, lumaBlocks), census);
        jpn::optimiseTables(census, huffman);
        jpn::tablesOf(huffman, own);
    }
    const jpn::Tables &t = optimised ? own : jpn::tables();
    /* bits */
    std::vector<jpn::u32> bits((size_t)nbBlocks);
    bool inside = true;
    for (long i = 0; i < nbBlocks; ++i)
        inside &= jpn::blockBits(t, blocks + i * 64, previousDc(i), jpn::chromaOf(i, lumaBlocks), &bits[(size_t)i]);
    if (!inside)
        return false;
    if (optimised)
        *optimised = huffman;
    /* prefix */
    std::vector<jpn::u64> offsets((size_t)nbBlocks + 1);
    jpn::exclusiveSum(bits.data(), nbBlocks, offsets.data());
    const jpn::u64 totalBits = offsets[(size_t)nbBlocks];
    /* emit, and the tail */
    std::vector<jpn::u32> words((size_t)jpn::streamWords(totalBits), 0u);
    for (long i = 0; i < nbBlocks; ++i)
        jpn::blockEmit(t, blocks + i * 64, previousDc(i), jpn::chromaOf(i, lumaBlocks), offsets[(size_t)i], words.data());
    if (const int tail = jpn::tailBits(totalBits))
    {
        jpn::WordWriter writer = {words.data(), totalBits};
        writer.put((1u << tail) - 1u, tail);
    }
    /* count */
    const jpn::u64 nbBytes = jpn::streamBytes(totalBits);
    const int wordsPerChunk = jpn::STUFF_CHUNK_BYTES / 4;
    const long nbChunks = (long)((nbBytes + jpn::STUFF_CHUNK_BYTES - 1) / jpn::STUFF_CHUNK_BYTES);
    std::vector<jpn::u32> counts((size_t)nbChunks, 0u);
    for (long c = 0; c < nbChunks; ++c)
        for (int w = 0; w < wordsPerChunk; ++w)
        {
            const jpn::u64 index = (jpn::u64)c * wordsPerChunk + w;
            if (const int n = jpn::bytesOfWord(index, nbBytes))
                counts[(size_t)c] += jpn::countFF(words[(size_t)index], n);
        }
    std::vector<jpn::u64> before((size_t)nbChunks + 1);
    jpn::exclusiveSum(counts.data(), nbChunks, before.data());
    /* stuff */
    out.assign((size_t)(nbBytes + before[(size_t)nbChunks]), 0);
    for (long c = 0; c < nbChunks; ++c)
    {
        jpn::u64 to = (jpn::u64)c * jpn::STUFF_CHUNK_BYTES + before[(size_t)c];
        for (int w = 0; w < wordsPerChunk; ++w)
        {
            const jpn::u64 index = (jpn::u64)c * wordsPerChunk + w;
            if (const int n = jpn::bytesOfWord(index, nbBytes))
                to += jpn::stuffWord(words[(size_t)index], n, out.data() + to);
        }
    }
    return true;
}

bool JpegWriter::writeFile(const std::string &filename, const std::vector<unsigned char> &bytes)
{
    FILE *f = fopen(filename.c_str(), "wb");
    if (!f)
        return false;
    const bool written = fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    return (fclose(f) == 0) && written;
}
}
