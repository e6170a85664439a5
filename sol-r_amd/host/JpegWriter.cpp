/*
 * JpegWriter.cpp - see JpegWriter.h.  The stream follows ITU T.81 (markers B.2, Huffman tables annex C and K.3, the
 * coding of a block F.1.2); where the standard leaves a choice the reference's jpge.cpp is followed, line numbers below.
 */
#include "JpegWriter.h"

#include <cstdio>

namespace solr
{
namespace
{
typedef unsigned char u8;

/* ITU T.81 tables K.3 - K.6: the number of codes of each length 1..16, then the symbols in code order */
const u8 DC_LUMA_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const u8 DC_CHROMA_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const u8 DC_VALUES[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const u8 AC_LUMA_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const u8 AC_LUMA_VALUES[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const u8 AC_CHROMA_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const u8 AC_CHROMA_VALUES[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

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
}

std::vector<unsigned char> JpegWriter::encode(int width, int height, int lumaH, int lumaV,
                                              const unsigned short quant[2][64], const short *blocks, long nbBlocks)
{
    static const HuffmanTable dc[2] = {HuffmanTable(DC_LUMA_BITS, DC_VALUES, 12), HuffmanTable(DC_CHROMA_BITS, DC_VALUES, 12)};
    static const HuffmanTable ac[2] = {HuffmanTable(AC_LUMA_BITS, AC_LUMA_VALUES, 162),
                                       HuffmanTable(AC_CHROMA_BITS, AC_CHROMA_VALUES, 162)};
    Stream s;
    s.out.reserve(1024 + (size_t)nbBlocks * 32);
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

    /* the scan: :883-952 */
    const int lumaBlocks = lumaH * lumaV, perMcu = lumaBlocks + 2;
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

bool JpegWriter::writeFile(const std::string &filename, const std::vector<unsigned char> &bytes)
{
    FILE *f = fopen(filename.c_str(), "wb");
    if (!f)
        return false;
    const bool written = fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    return (fclose(f) == 0) && written;
}
}
