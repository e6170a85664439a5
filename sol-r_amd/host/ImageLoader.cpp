/*
 * ImageLoader.cpp - see ImageLoader.h.  The JPEG half follows ITU T.81 for the stream (markers B.2, Huffman tables
 * C / F.2.2) and the reference's decoder for what a block's numbers mean (jpgd.cpp:1923-2028, decode_next_row).
 */
#include "ImageLoader.h"

#include <cstdio>
#include <cstring>

#include "../csrc/jpeg_pixels.h"

namespace solr
{
namespace
{
typedef unsigned char u8;

const size_t MAX_FILE_BYTES = (size_t)1 << 30;

bool readFile(const std::string &filename, std::vector<u8> &bytes, std::string &why)
{
    FILE *file = fopen(filename.c_str(), "rb");
    if (!file)
    {
        why = "cannot be opened";
        return false;
    }
    bool done = false;
    if (fseek(file, 0, SEEK_END) == 0)
    {
        const long size = ftell(file);
        if (size >= 0 && (size_t)size <= MAX_FILE_BYTES && fseek(file, 0, SEEK_SET) == 0)
        {
            bytes.resize((size_t)size);
            done = size == 0 || fread(bytes.data(), 1, (size_t)size, file) == (size_t)size;
        }
    }
    fclose(file);
    if (!done)
        why = "cannot be read";
    return done;
}

unsigned le16(const u8 *p) { return p[0] | (p[1] << 8); }
unsigned le32(const u8 *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((unsigned)p[3] << 24); }
unsigned be16(const u8 *p) { return (p[0] << 8) | p[1]; }

bool saneSize(long width, long height)
{
    return width >= 1 && height >= 1 && width <= SOLR_JPEG_MAX_SIDE && height <= SOLR_JPEG_MAX_SIDE &&
           width * height <= SOLR_JPEG_MAX_PIXELS;
}
}

/* ---------------------------------------------------------------------- */
/* BMP                                                                    */
/* ---------------------------------------------------------------------- */
bool ImageLoader::loadBMP24(const std::string &filename, Image &image, std::string &why)
{
    std::vector<u8> d;
    if (!readFile(filename, d, why))
        return false;
    /* BITMAPFILEHEADER: 14 bytes (bfType, bfSize, two reserved words, bfOffBits at 10); BITMAPINFOHEADER follows:
     * biSize at 14, biWidth 18, biHeight 22, biPlanes 26, biBitCount 28, biCompression 30 */
    if (d.size() < 54 || d[0] != 'B' || d[1] != 'M')
    {
        why = "not a BMP file (wrong bitmap id)";
        return false;
    }
    const size_t offBits = le32(&d[10]);
    const long width = (int)le32(&d[18]);
    long height = (int)le32(&d[22]);
    if (height < 0)
        height = -height; /* a top-down file: the rows are kept in file order either way */
    if (le32(&d[14]) < 40 || le16(&d[28]) != 24 || le32(&d[30]) != 0)
    {
        why = "only uncompressed 24-bit BMP files are read";
        return false;
    }
    if (!saneSize(width, height))
    {
        why = "size out of range";
        return false;
    }
    const size_t rowBytes = ((size_t)width * 3 + 3) & ~(size_t)3;
    if (offBits < 54 || offBits > d.size() || rowBytes * (size_t)(height - 1) + (size_t)width * 3 > d.size() - offBits)
    {
        why = "pixel data beyond the end of the file";
        return false;
    }
    image.width = (int)width;
    image.height = (int)height;
    image.depth = 3;
    image.pixels.resize((size_t)width * height * 3);
    for (long y = 0; y < height; ++y)
    {
        const u8 *row = &d[offBits + rowBytes * (size_t)y];
        u8 *out = &image.pixels[(size_t)y * width * 3];
        for (long x = 0; x < width; ++x)
        {
            out[3 * x] = row[3 * x + 2];
            out[3 * x + 1] = row[3 * x + 1];
            out[3 * x + 2] = row[3 * x];
        }
    }
    return true;
}

/* ---------------------------------------------------------------------- */
/* TGA                                                                    */
/* ---------------------------------------------------------------------- */
bool ImageLoader::loadTGA(const std::string &filename, Image &image, std::string &why)
{
    std::vector<u8> d;
    if (!readFile(filename, d, why))
        return false;
    /* tgad.cpp:18-19,45-58: the first 12 bytes are those of a type-2 or a type-10 file with no id field, no colour
     * map and the origin at 0, 0 - anything else is refused */
    static const u8 raw[12] = {0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0}, rle[12] = {0, 0, 10, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (d.size() < 18 || (memcmp(d.data(), raw, 12) != 0 && memcmp(d.data(), rle, 12) != 0))
    {
        why = "only TGA files of type 2 or 10 without id field and colour map are read";
        return false;
    }
    const bool compressed = d[2] == 10;
    const long width = le16(&d[12]), height = le16(&d[14]);
    const int bpp = d[16];
    if (!saneSize(width, height) || (bpp != 24 && bpp != 32))
    {
        why = "only 24- and 32-bit TGA files of a non-empty size are read";
        return false;
    }
    const size_t depth = bpp / 8, nbPixels = (size_t)width * height;
    std::vector<u8> pixels(nbPixels * depth);
    size_t pos = 18;
    if (!compressed)
    {
        if (d.size() - pos < pixels.size())
        {
            why = "pixel data beyond the end of the file";
            return false;
        }
        for (size_t i = 0; i < nbPixels; ++i, pos += depth)
        {
            u8 *out = &pixels[i * depth];
            out[0] = d[pos + 2];
            out[1] = d[pos + 1];
            out[2] = d[pos];
            if (depth == 4)
                out[3] = d[pos + 3];
        }
    }
    else
    {
        /* tgad.cpp:188-334: a packet header below 128 announces header + 1 pixels, otherwise one pixel repeated
         * header - 127 times */
        size_t pixel = 0;
        while (pixel < nbPixels)
        {
            if (pos >= d.size())
            {
                why = "run-length data ends before the image is complete";
                return false;
            }
            const unsigned header = d[pos++];
            const bool run = header >= 128;
            const size_t count = run ? header - 127 : header + 1;
            const size_t needed = run ? depth : count * depth;
            if (count > nbPixels - pixel || needed > d.size() - pos)
            {
                why = count > nbPixels - pixel ? "a run-length packet runs past the image"
                                               : "run-length data ends before the image is complete";
                return false;
            }
            for (size_t i = 0; i < count; ++i, ++pixel)
            {
                const u8 *in = &d[pos + (run ? 0 : i * depth)];
                u8 *out = &pixels[pixel * depth];
                out[0] = in[2];
                out[1] = in[1];
                out[2] = in[0];
                if (depth == 4)
                    out[3] = in[3];
            }
            pos += needed;
        }
    }
    image.width = (int)width;
    image.height = (int)height;
    image.depth = (int)depth;
    image.pixels.swap(pixels);
    return true;
}

/* ---------------------------------------------------------------------- */
/* JPEG: markers and the Huffman stream                                    */
/* ---------------------------------------------------------------------- */
namespace
{
/* position in the block (row-major) of the k-th coefficient of the zig-zag sequence (T.81 figure A.6) */
const u8 ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffmanTable
{
    bool defined = false;
    int count[17];  /* codes of each length 1..16 */
    int first[17];  /* the first code of that length */
    int index[17];  /* where that length's values begin */
    u8 values[256];
};

struct Component
{
    int id, h, v, quantTable, dcTable, acTable;
};

/* the entropy-coded segment, a bit at a time; 0xFF00 is a data byte 0xFF, any other marker or the end of the file
 * ends the supply of bits, and asking for more is an error */
struct BitReader
{
    const u8 *d;
    size_t n, pos;
    unsigned acc = 0;
    int nbits = 0;

    bool fill()
    {
        if (pos >= n)
            return false;
        unsigned byte = d[pos];
        if (byte == 0xFF)
        {
            if (pos + 1 >= n || d[pos + 1] != 0)
                return false;
            pos += 2;
        }
        else
            ++pos;
        acc = (acc << 8) | byte;
        nbits += 8;
        return true;
    }
    /* k <= 16 */
    bool bits(int k, int &value)
    {
        while (nbits < k)
            if (!fill())
                return false;
        value = (int)((acc >> (nbits - k)) & ((1u << k) - 1u));
        nbits -= k;
        return true;
    }
    bool symbol(const HuffmanTable &t, int &value)
    {
        int code = 0, bit;
        for (int length = 1; length <= 16; ++length)
        {
            if (!bits(1, bit))
                return false;
            code = (code << 1) | bit;
            const int at = code - t.first[length];
            if (at >= 0 && at < t.count[length])
            {
                value = t.values[t.index[length] + at];
                return true;
            }
        }
        return false; /* no such code */
    }
    /* RSTm between two restart intervals (T.81 E.2.4): the rest of the byte is padding */
    bool restart(int expected)
    {
        acc = 0;
        nbits = 0;
        if (pos >= n || d[pos] != 0xFF)
            return false;
        while (pos < n && d[pos] == 0xFF)
            ++pos;
        if (pos >= n || d[pos] != 0xD0 + expected)
            return false;
        ++pos;
        return true;
    }
};

/* T.81 F.2.2.1 (EXTEND); jpgd.cpp:661-681 */
inline int extend(int v, int size)
{
    return v < (1 << (size - 1)) ? v - (1 << size) + 1 : v;
}

struct JpegParser
{
    const std::vector<u8> &d;
    std::string &why;
    unsigned short quant[4][64];
    bool quantDefined[4] = {false, false, false, false};
    HuffmanTable dc[4], ac[4];
    Component comp[3];
    bool haveFrame = false;
    int width = 0, height = 0, restartInterval = 0;

    JpegParser(const std::vector<u8> &data, std::string &reason) : d(data), why(reason) {}

    bool fail(const char *reason)
    {
        why = reason;
        return false;
    }

    bool defineHuffmanTables(const u8 *seg, size_t len)
    {
        while (len > 0)
        {
            if (len < 17)
                return fail("corrupt Huffman table segment");
            const int tableClass = seg[0] >> 4, id = seg[0] & 15;
            if (tableClass > 1 || id > 3)
                return fail("corrupt Huffman table segment (class or number out of range)");
            HuffmanTable &t = tableClass ? ac[id] : dc[id];
            int total = 0, code = 0;
            t.count[0] = t.first[0] = t.index[0] = 0;
            for (int length = 1; length <= 16; ++length)
            {
                t.count[length] = seg[length];
                t.first[length] = code;
                t.index[length] = total;
                total += t.count[length];
                code += t.count[length];
                if (code > (1 << length))
                    return fail("corrupt Huffman table (more codes of a length than there can be)");
                code <<= 1;
            }
            if (total > 256 || (size_t)total > len - 17)
                return fail("corrupt Huffman table segment (values beyond its end)");
            memcpy(t.values, seg + 17, (size_t)total);
            t.defined = true;
            seg += 17 + total;
            len -= 17 + (size_t)total;
        }
        return true;
    }

    bool defineQuantTables(const u8 *seg, size_t len)
    {
        while (len > 0)
        {
            const int precision = seg[0] >> 4, id = seg[0] & 15;
            if (precision == 1)
                return fail("16-bit quantisation tables are not read");
            if (precision != 0 || id > 3 || len < 65)
                return fail("corrupt quantisation table segment");
            for (int k = 0; k < 64; ++k)
                quant[id][ZIGZAG[k]] = seg[1 + k];
            quantDefined[id] = true;
            seg += 65;
            len -= 65;
        }
        return true;
    }

    bool startOfFrame(const u8 *seg, size_t len)
    {
        if (haveFrame)
            return fail("more than one frame header");
        if (len < 6)
            return fail("corrupt frame header");
        if (seg[0] != 8)
            return fail("only 8-bit samples are read");
        height = (int)be16(seg + 1);
        width = (int)be16(seg + 3);
        const int nbComponents = seg[5];
        if (nbComponents == 1)
            return fail("one-component (grayscale) files are not read");
        if (nbComponents != 3 || len < 6 + 3 * 3)
            return fail("only three-component files are read");
        if (!saneSize(width, height))
            return fail("size out of range");
        for (int i = 0; i < 3; ++i)
        {
            comp[i].id = seg[6 + 3 * i];
            comp[i].h = seg[7 + 3 * i] >> 4;
            comp[i].v = seg[7 + 3 * i] & 15;
            comp[i].quantTable = seg[8 + 3 * i];
            if (comp[i].quantTable > 3)
                return fail("corrupt frame header (quantisation table number out of range)");
        }
        if (comp[0].h == 1 && comp[0].v == 2 && comp[1].h == 1 && comp[1].v == 1 && comp[2].h == 1 && comp[2].v == 1)
            return fail("1x2 luma sampling is not read");
        if (!jpx::samplingSupported(comp[0].h, comp[0].v) || comp[1].h != 1 || comp[1].v != 1 || comp[2].h != 1 ||
            comp[2].v != 1)
            return fail("only luma sampling 1x1, 2x1 or 2x2 with chroma 1x1 is read");
        haveFrame = true;
        return true;
    }

    bool startOfScan(const u8 *seg, size_t len)
    {
        if (!haveFrame)
            return fail("scan before the frame header");
        if (len < 1)
            return fail("corrupt scan header");
        const int nbComponents = seg[0];
        if (nbComponents == 1 || nbComponents == 2)
            return fail("non-interleaved scans are not read");
        if (nbComponents != 3 || len < 1 + 2 * 3 + 3)
            return fail("corrupt scan header");
        for (int i = 0; i < 3; ++i)
        {
            if (seg[1 + 2 * i] != comp[i].id)
                return fail("the scan's components are not the frame's, in its order");
            comp[i].dcTable = seg[2 + 2 * i] >> 4;
            comp[i].acTable = seg[2 + 2 * i] & 15;
            if (comp[i].dcTable > 3 || comp[i].acTable > 3 || !dc[comp[i].dcTable].defined ||
                !ac[comp[i].acTable].defined)
                return fail("the scan names a Huffman table that is not defined");
            if (!quantDefined[comp[i].quantTable])
                return fail("the frame names a quantisation table that is not defined");
        }
        if (seg[7] != 0 || seg[8] != 63 || seg[9] != 0)
            return fail("corrupt scan header (spectral selection of a sequential scan)");
        return true;
    }

    bool decodeScan(size_t pos, const SolrJpegFrame &frame, std::vector<short> &coefficients)
    {
        BitReader in{d.data(), d.size(), pos};
        const int lumaBlocks = frame.lumaH * frame.lumaV, perMcu = lumaBlocks + 2;
        const long nbMcus = (long)frame.mcusPerRow * frame.mcuRows;
        int prediction[3] = {0, 0, 0};
        int nextRestart = 0;
        short *block = coefficients.data();
        for (long mcu = 0; mcu < nbMcus; ++mcu)
        {
            if (restartInterval && mcu && mcu % restartInterval == 0)
            {
                if (!in.restart(nextRestart))
                    return fail("truncated or corrupt stream (restart marker missing)");
                nextRestart = (nextRestart + 1) & 7;
                prediction[0] = prediction[1] = prediction[2] = 0;
            }
            for (int b = 0; b < perMcu; ++b, block += 64)
            {
                const int c = b < lumaBlocks ? 0 : b - lumaBlocks + 1;
                const HuffmanTable &dcTable = dc[comp[c].dcTable], &acTable = ac[comp[c].acTable];
                int size, value;
                if (!in.symbol(dcTable, size) || size > 15)
                    return fail("truncated or corrupt stream");
                if (size)
                {
                    if (!in.bits(size, value))
                        return fail("truncated or corrupt stream");
                    prediction[c] += extend(value, size);
                }
                block[0] = (short)prediction[c];
                for (int k = 1; k < 64;)
                {
                    int rs;
                    if (!in.symbol(acTable, rs))
                        return fail("truncated or corrupt stream");
                    const int run = rs >> 4;
                    size = rs & 15;
                    if (size)
                    {
                        k += run;
                        if (k > 63 || !in.bits(size, value))
                            return fail("truncated or corrupt stream");
                        block[ZIGZAG[k]] = (short)extend(value, size);
                        ++k;
                    }
                    else if (run == 15)
                    {
                        if (k + 16 > 64)
                            return fail("truncated or corrupt stream");
                        k += 16;
                    }
                    else
                        break; /* end of block */
                }
            }
        }
        return true;
    }

    bool parse(SolrJpegFrame &frame, std::vector<short> &coefficients)
    {
        const size_t n = d.size();
        if (n < 4 || d[0] != 0xFF || d[1] != 0xD8)
            return fail("not a JPEG file");
        size_t pos = 2;
        for (;;)
        {
            if (pos >= n)
                return fail("truncated before the scan");
            if (d[pos] != 0xFF)
                return fail("corrupt stream (marker expected)");
            while (pos < n && d[pos] == 0xFF)
                ++pos;
            if (pos >= n)
                return fail("truncated before the scan");
            const int marker = d[pos++];
            if (marker == 0x01 || (marker >= 0xD0 && marker <= 0xD7))
                continue;
            if (marker == 0xD9)
                return fail("no scan before the end of the image");
            if (marker == 0x00 || marker == 0xD8)
                return fail("corrupt stream (marker expected)");
            if (n - pos < 2)
                return fail("truncated before the scan");
            const size_t length = be16(&d[pos]);
            if (length < 2 || length > n - pos)
                return fail("truncated before the scan (a segment runs past the end of the file)");
            const u8 *seg = &d[pos + 2];
            const size_t len = length - 2;
            pos += length;
            switch (marker)
            {
            case 0xC0:
            case 0xC1:
                if (!startOfFrame(seg, len))
                    return false;
                break;
            case 0xC2:
                return fail("progressive files are not read");
            case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xC8: case 0xC9: case 0xCA: case 0xCB: case 0xCC:
            case 0xCD: case 0xCE: case 0xCF:
                return fail("only baseline and extended-sequential Huffman files are read");
            case 0xC4:
                if (!defineHuffmanTables(seg, len))
                    return false;
                break;
            case 0xDB:
                if (!defineQuantTables(seg, len))
                    return false;
                break;
            case 0xDD:
                if (len < 2)
                    return fail("corrupt restart interval segment");
                restartInterval = (int)be16(seg);
                break;
            case 0xDA:
            {
                if (!startOfScan(seg, len))
                    return false;
                memset(&frame, 0, sizeof(frame));
                frame.width = width;
                frame.height = height;
                frame.lumaH = comp[0].h;
                frame.lumaV = comp[0].v;
                frame.mcusPerRow = (width + 8 * frame.lumaH - 1) / (8 * frame.lumaH);
                frame.mcuRows = (height + 8 * frame.lumaV - 1) / (8 * frame.lumaV);
                for (int c = 0; c < 3; ++c)
                    memcpy(frame.quant[c], quant[comp[c].quantTable], sizeof(frame.quant[c]));
                const size_t nbBlocks =
                    (size_t)frame.mcusPerRow * frame.mcuRows * jpx::blocksPerMcu(frame.lumaH, frame.lumaV);
                coefficients.assign(nbBlocks * 64, 0);
                return decodeScan(pos, frame, coefficients);
            }
            default:
                break; /* APPn, COM and whatever else carries a length: skipped */
            }
        }
    }
};

/* both passes of the inverse DCT over one dequantised block (jpgd.cpp:304-405) */
void inverseDct(const short block[64], u8 samples[64])
{
    int rows[64];
    for (int r = 0; r < 8; ++r)
        jpx::idctRow(block + 8 * r, rows + 8 * r);
    for (int c = 0; c < 8; ++c)
    {
        int column[8];
        u8 out[8];
        for (int r = 0; r < 8; ++r)
            column[r] = rows[8 * r + c];
        jpx::idctColumn(column, out);
        for (int r = 0; r < 8; ++r)
            samples[8 * r + c] = out[r];
    }
}

/* one dequantised chroma block of a 2x2 file to the four sample blocks of its 16x16 MCU (jpgd.cpp:1684-1787) */
void expandChroma(const short block[64], u8 samples[4 * 64])
{
    int x0[4][8], x1[4][8];
    for (int r = 0; r < 8; ++r)
    {
        int v[8];
        for (int c = 0; c < 8; ++c)
            v[c] = block[8 * r + c];
        for (int t = 0; t < 4; ++t)
            jpx::upsampleStep(t, v, &x0[t][r], &x1[t][r]);
    }
    short expanded[4][64];
    memset(expanded, 0, sizeof(expanded));
    for (int a = 0; a < 4; ++a)
        for (int j = 0; j < 4; ++j)
        {
            int p, q, r, s;
            short four[4];
            jpx::upsampleStep(j, x0[a], &p, &q);
            jpx::upsampleStep(j, x1[a], &r, &s);
            jpx::upsampleCombine(p, q, r, s, four);
            for (int k = 0; k < 4; ++k)
                expanded[k][8 * j + a] = four[k];
        }
    for (int k = 0; k < 4; ++k)
        inverseDct(expanded[k], samples + 64 * k);
}
}

bool ImageLoader::parseJPEG(const std::string &filename, SolrJpegFrame &frame, std::vector<short> &coefficients,
                            std::string &why)
{
    std::vector<u8> d;
    if (!readFile(filename, d, why))
        return false;
    JpegParser parser(d, why);
    return parser.parse(frame, coefficients);
}

void ImageLoader::jpegPixelsOnHost(const SolrJpegFrame &frame, const short *coefficients, unsigned char *rgb)
{
    const int lumaBlocks = frame.lumaH * frame.lumaV, perMcu = lumaBlocks + 2;
    const int mcuWidth = 8 * frame.lumaH, mcuHeight = 8 * frame.lumaV;
    const bool expand = frame.lumaV == 2;
    for (int my = 0; my < frame.mcuRows; ++my)
        for (int mx = 0; mx < frame.mcusPerRow; ++mx)
        {
            const short *source = coefficients + ((size_t)my * frame.mcusPerRow + mx) * perMcu * 64;
            u8 samples[12 * 64];
            for (int b = 0; b < perMcu; ++b)
            {
                const int c = b < lumaBlocks ? 0 : b - lumaBlocks + 1;
                short block[64];
                for (int k = 0; k < 64; ++k)
                    block[k] = jpx::dequantise(source[64 * b + k], frame.quant[c][k]);
                if (expand && c > 0)
                    expandChroma(block, samples + 64 * (lumaBlocks + 4 * (c - 1)));
                else
                    inverseDct(block, samples + 64 * b);
            }
            for (int y = 0; y < mcuHeight && my * mcuHeight + y < frame.height; ++y)
                for (int x = 0; x < mcuWidth && mx * mcuWidth + x < frame.width; ++x)
                {
                    int offY, offCb, offCr;
                    jpx::sampleOffsets(frame.lumaH, frame.lumaV, x, y, &offY, &offCb, &offCr);
                    const long at = jpx::turnedPixel(frame.width, frame.height, mx * mcuWidth + x, my * mcuHeight + y);
                    jpx::colour(samples[offY], samples[offCb], samples[offCr], rgb + 3 * at);
                }
        }
}
}
