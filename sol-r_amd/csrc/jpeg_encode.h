/*
 * jpeg_encode.h - the pixel stage of the JPEG screenshot writer: what turns RGB bytes into quantised coefficient blocks in
 * zigzag order, ready for the Huffman coder (host/JpegWriter.cpp).  Integer arithmetic only, written once for both sides:
 * the host-only engine runs it in a loop (GPUKernel::jpegCoefficients), the HIP engine in a kernel
 * (csrc/solr_jpeg_encode.hip).  The mirror image of jpeg_pixels.h.
 *
 * It restates the arithmetic of the reference's encoder, solr/images/jpge.cpp, bit for bit - a screenshot is then the file
 * the reference writes for the same frame:
 *   colour          fixed-point RGB -> YCbCr with 16 fractional bits, Cb and Cr clamped       jpge.cpp:100-123
 *   edges           the last pixel of a row repeated to the MCU width (after conversion), the last row repeated to
 *                   the MCU height                                                            jpge.cpp:1085-1099, 1043-1049
 *   block loads     sample - 128; 2x1 chroma (a + b) >> 1; 2x2 chroma a four-pixel sum with a bias that alternates
 *                   0, 2 along a row and swaps on every row, >> 2                             jpge.cpp:720-781
 *   forward DCT     rows first (CONST_BITS 13, ROW_BITS 2), then columns                      jpge.cpp:158-223
 *   quantisation    tables from quality 1..100; |x| + (q >> 1), zero below q, else a truncating division, sign
 *                   restored; zigzag order, 16 bits                                           jpge.cpp:565-578, 783-806
 * tests/golden/jpeg_encoder.npz holds jpge's own files and the blocks they carry.
 *
 * No floating point anywhere.  For 8-bit samples every sum fits in 32 bits with room to spare (the largest coefficient
 * is 8 * 8 * 128 * 2 = 16 384 in magnitude), so plain int arithmetic is defined throughout.
 */
#pragma once

#if defined(__HIPCC__)
#define JPE_HD __host__ __device__
#else
#define JPE_HD
#endif

namespace jpe
{
typedef unsigned int u32;

/* the largest magnitude quantise() is exact for: what the DCT can produce (16 384) plus the largest q >> 1 (127) */
constexpr int MAX_MAGNITUDE = 16384 + 127;

JPE_HD inline int blocksPerMcu(int lumaH, int lumaV) { return lumaH * lumaV + 2; }
JPE_HD inline bool samplingSupported(int lumaH, int lumaV)
{
    return (lumaH == 1 && lumaV == 1) || (lumaH == 2 && lumaV == 1) || (lumaH == 2 && lumaV == 2);
}

/* jpge.cpp:102-112 */
JPE_HD inline int clamp255(int i)
{
    return i < 0 ? 0 : (i > 255 ? 255 : i);
}

/* jpge.cpp:100-101 (YR ... CR_B), :114-123 (RGB_to_YCC).  Y needs no clamp (the three weights sum to 65 536); Cb and Cr
 * do: pure blue gives 128 + ((255 * 32768 + 32768) >> 16) = 256, and so does pure red for Cr */
JPE_HD inline void rgbToYcc(int red, int green, int blue, unsigned char ycc[3])
{
    ycc[0] = (unsigned char)((red * 19595 + green * 38470 + blue * 7471 + 32768) >> 16);
    ycc[1] = (unsigned char)clamp255(128 + ((red * -11059 + green * -21709 + blue * 32768 + 32768) >> 16));
    ycc[2] = (unsigned char)clamp255(128 + ((red * 32768 + green * -27439 + blue * -5329 + 32768) >> 16));
}

/* Which pixel of the source picture the encoder sees as its pixel p (row-major, nbPixels = width * height).  A
 * screenshot is turned: the reference's GPUKernel::generateScreenshot (GPUKernel.cpp:2823-2829) fills pixel p from pixel
 * nbPixels - p, which for p = 0 is one pixel past the picture; that one index is clamped to the last pixel here. */
JPE_HD inline long sourcePixel(long nbPixels, long p, int turned)
{
    if (!turned)
        return p;
    const long q = nbPixels - p;
    return q > nbPixels - 1 ? nbPixels - 1 : q;
}

/* Y, Cb, Cr of position (x, y) of the MCU grid, which reaches beyond the picture: the edge rule of load_mcu
 * (jpge.cpp:1085-1099: the last converted pixel of a row repeated) and process_end_of_image (:1043-1049: the last row
 * repeated) is a clamp of the coordinates.  swapRedBlue: the source bytes are B, G, R (GPUKernel.cpp:2836-2842) */
JPE_HD inline void sample(const unsigned char *rgb, int width, int height, int turned, int swapRedBlue, int x, int y,
                          unsigned char ycc[3])
{
    const int cx = x < width ? x : width - 1, cy = y < height ? y : height - 1;
    const unsigned char *from = rgb + 3 * sourcePixel((long)width * height, (long)cy * width + cx, turned);
    rgbToYcc(from[swapRedBlue ? 2 : 0], from[1], from[swapRedBlue ? 0 : 2], ycc);
}

/* Row `row` of block `block` of an MCU whose converted pixels are in `mcu` (8 * lumaV rows of 8 * lumaH pixels of 3
 * bytes): blocks in scan order, the luma blocks row by row, then Cb, then Cr.
 *   luma, 1x1 chroma   load_block_8_8      jpge.cpp:720-738
 *   2x1 chroma         load_block_16_8_8   jpge.cpp:764-781
 *   2x2 chroma         load_block_16_8     jpge.cpp:740-762: a = 0, b = 2 in the first row, swapped on every row */
JPE_HD inline void blockRow(const unsigned char *mcu, int lumaH, int lumaV, int block, int row, int out[8])
{
    const int lumaBlocks = lumaH * lumaV, pitch = 8 * lumaH * 3;
    if (block < lumaBlocks || lumaBlocks == 1)
    {
        const int c = block < lumaBlocks ? 0 : block - lumaBlocks + 1;
        const int bx = block < lumaBlocks ? (lumaH == 2 ? (block & 1) : 0) : 0;
        const int by = block < lumaBlocks ? (lumaH == 2 ? (block >> 1) : 0) : 0;
        const unsigned char *from = mcu + (by * 8 + row) * pitch + bx * 8 * 3 + c;
        for (int i = 0; i < 8; ++i)
            out[i] = from[3 * i] - 128;
        return;
    }
    const int c = block - lumaBlocks + 1;
    if (lumaV == 1)
    {
        const unsigned char *from = mcu + row * pitch + c;
        for (int i = 0; i < 8; ++i)
            out[i] = ((from[6 * i] + from[6 * i + 3]) >> 1) - 128;
        return;
    }
    const unsigned char *upper = mcu + 2 * row * pitch + c, *lower = upper + pitch;
    for (int i = 0; i < 8; ++i)
    {
        const int bias = ((i + row) & 1) ? 2 : 0;
        out[i] = ((upper[6 * i] + upper[6 * i + 3] + lower[6 * i] + lower[6 * i + 3] + bias) >> 2) - 128;
    }
}

/* jpge.cpp:165 DCT_MUL: the first operand goes through 16 bits.  The cast is kept because the reference has it; for
 * 8-bit samples it never truncates.  An operand is a sum of +-1 times the eight inputs of a pass.  First pass: samples of
 * -128 ... 127, at most 1024 in magnitude.  Second pass: the first pass left at most 4 * 1024 = 4096 in column 0 (the row
 * sums, two fractional bits) and less in the others (an AC output is at most sqrt(2) * sum |cos| = 7.25 samples, 3712),
 * so the largest operand is 4 * 4096 + 4 * 4064 = 32 640, in column 0 of a block whose rows alternate between the extremes -
 * below 32 768.  tests/golden/make_jpeg_encoder_fixtures.py asserts it of every operand of every fixture. */
JPE_HD inline int dctMul(int v, int c)
{
    return (int)(short)v * c;
}

/* jpge.cpp:164 DCT_DESCALE */
JPE_HD inline int dctDescale(int x, int n)
{
    return (x + (1 << (n - 1))) >> n;
}

/* jpge.cpp:166-191 DCT1D: s[0..7] in, the eight sums out; s[0] and s[4] come without the 13 fractional bits of the rest */
JPE_HD inline void dct1d(int s[8])
{
    const int t0 = s[0] + s[7], t7 = s[0] - s[7], t1 = s[1] + s[6], t6 = s[1] - s[6];
    const int t2 = s[2] + s[5], t5 = s[2] - s[5], t3 = s[3] + s[4], t4 = s[3] - s[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int e = dctMul(t12 + t13, 4433);
    s[2] = e + dctMul(t13, 6270);
    s[6] = e + dctMul(t12, -15137);
    const int z5 = dctMul((t4 + t6) + (t5 + t7), 9633);
    const int u1 = dctMul(t4 + t7, -7373), u2 = dctMul(t5 + t6, -20995);
    const int u3 = dctMul(t4 + t6, -16069) + z5, u4 = dctMul(t5 + t7, -3196) + z5;
    s[0] = t10 + t11;
    s[4] = t10 - t11;
    s[1] = dctMul(t7, 12299) + u1 + u4;
    s[3] = dctMul(t6, 25172) + u2 + u3;
    s[5] = dctMul(t5, 16819) + u2 + u4;
    s[7] = dctMul(t4, 2446) + u1 + u3;
}

/* first pass, one row (jpge.cpp:196-208): two fractional bits (ROW_BITS) are kept */
JPE_HD inline void dctRow(int s[8])
{
    dct1d(s);
    for (int i = 0; i < 8; ++i)
        s[i] = (i & 3) == 0 ? s[i] * 4 : dctDescale(s[i], 13 - 2);
}

/* second pass, one column of the first pass's results (jpge.cpp:209-222) */
JPE_HD inline void dctColumn(int s[8])
{
    dct1d(s);
    for (int i = 0; i < 8; ++i)
        s[i] = dctDescale(s[i], (i & 3) == 0 ? 2 + 3 : 13 + 2 + 3);
}

/* position in the block (row-major) of the k-th coefficient of the zigzag sequence: jpge.cpp:55-57 s_zag, ITU T.81
 * figure A.6 */
JPE_HD inline int zigzag(int k)
{
    static constexpr unsigned char order[64] = {
        0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return order[k];
}

/* The division of load_quantized_coefficients by a quantiser of 1..255 as a multiplication: for n <= MAX_MAGNITUDE
 * (< 2^15) and m = ceil(2^32 / q), n * m >> 32 is n / q exactly - the error of m is below q / 2^32 of a unit, n times
 * that stays below 2^23 / 2^32.  q = 1 has no such m in 32 bits and is marked by 0.  tests/test_jpeg_encoder.py goes
 * through every q and every n. */
JPE_HD inline u32 reciprocal(int q)
{
    return q <= 1 ? 0u : (u32)((0x100000000ull + (u32)q - 1u) / (u32)q);
}

/* jpge.cpp:783-806, one coefficient: j from the DCT, q the quantiser at its zigzag position, m = reciprocal(q) */
JPE_HD inline short quantise(int j, int q, u32 m)
{
    const int magnitude = (j < 0 ? -j : j) + (q >> 1);
    if (magnitude < q)
        return 0;
    const int quotient = m == 0u ? magnitude : (int)(((unsigned long long)(u32)magnitude * m) >> 32);
    return (short)(j < 0 ? -quotient : quotient);
}

/* jpge.cpp:565-578 compute_quant_table: component 0 is luma, anything else chroma; `table` in zigzag order, as jpge keeps
 * and writes it.  The base tables are those of ITU T.81 annex K.1 in that order (jpge.cpp:58-65). */
inline void quantTable(int quality, int component, unsigned short table[64])
{
    static const unsigned char luma[64] = {16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40,
                                           26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
                                           56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87,
                                           95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99};
    static const unsigned char chroma[16] = {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99};
    const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
    for (int i = 0; i < 64; ++i)
    {
        const int base = component == 0 ? luma[i] : (i < 16 ? chroma[i] : 99);
        const int v = (base * scale + 50) / 100;
        table[i] = (unsigned short)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
}

/* What the host-only engine runs and what the kernel is held to: the whole stage for one MCU.  `coefficients` receives
 * blocksPerMcu blocks of 64, `quant` and `recip` are [2][64] (luma, chroma). */
inline void encodeMcu(const unsigned char *rgb, int width, int height, int lumaH, int lumaV, int turned,
                      int swapRedBlue, int mcuX, int mcuY, const unsigned short quant[2][64], const u32 recip[2][64],
                      short *coefficients)
{
    unsigned char mcu[16 * 16 * 3];
    const int mcuWidth = 8 * lumaH, mcuHeight = 8 * lumaV;
    for (int y = 0; y < mcuHeight; ++y)
        for (int x = 0; x < mcuWidth; ++x)
            sample(rgb, width, height, turned, swapRedBlue, mcuX * mcuWidth + x, mcuY * mcuHeight + y,
                   &mcu[(y * mcuWidth + x) * 3]);
    const int lumaBlocks = lumaH * lumaV;
    for (int block = 0; block < lumaBlocks + 2; ++block)
    {
        int v[64];
        for (int row = 0; row < 8; ++row)
        {
            blockRow(mcu, lumaH, lumaV, block, row, &v[row * 8]);
            dctRow(&v[row * 8]);
        }
        for (int column = 0; column < 8; ++column)
        {
            int s[8];
            for (int i = 0; i < 8; ++i)
                s[i] = v[i * 8 + column];
            dctColumn(s);
            for (int i = 0; i < 8; ++i)
                v[i * 8 + column] = s[i];
        }
        const int table = block < lumaBlocks ? 0 : 1;
        for (int k = 0; k < 64; ++k)
            coefficients[block * 64 + k] = quantise(v[zigzag(k)], quant[table][k], recip[table][k]);
    }
}
} // namespace jpe
