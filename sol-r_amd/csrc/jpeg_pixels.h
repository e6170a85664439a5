/*
 * jpeg_pixels.h - the pixel stage of the JPEG texture loader: what turns Huffman-decoded coefficient blocks into RGB
 * bytes.  Integer arithmetic only, written once for both sides: the host-only engine runs it in a loop
 * (host/ImageLoader.cpp), the HIP engine in a kernel (csrc/solr_textures.hip).
 *
 * It restates the arithmetic of the reference's decoder, solr/images/jpgd.cpp, bit for bit - the reference's textures
 * are what its frames are compared on, and libjpeg-style decoders differ from it by several levels (they run the
 * columns of the inverse DCT first, and replicate 2x2 chroma where jpgd interpolates it in the frequency domain):
 *   dequantise      p[k] = (int16)(s * q[k])                                  jpgd.cpp:1944,1981
 *   inverse DCT     rows first (>> 11), then columns (+128, >> 18, clamp)     jpgd.cpp:103-263
 *   2x1 chroma      each sample covers two pixels                             jpgd.cpp:2058-2100 (H2V1Convert)
 *   2x2 chroma      the 8x8 chroma block becomes the four 8x8 blocks of the 16x16 MCU while still coefficients:
 *                   two passes of 4-term products with 10 fractional bits, rounded after each pass, the sums stored
 *                   in 16 bits, then an inverse DCT of the 4x4 low-frequency corner
 *                                                                             jpgd.cpp:786-985 (P_Q, R_S), 1670-1788
 *   colour          fixed-point YCbCr -> RGB with 16 fractional bits          jpgd.cpp:1614-1629, 2233-2265
 * jpgd's sparse variants (Row<N>, Col<N>, the DC-only shortcut, P_Q<rows, cols>) only leave out terms that are zero:
 * the general forms below give the same integers on zero-filled blocks WHILE EVERY SUM FITS IN 32 BITS AND EVERY 16-BIT
 * STORE KEEPS ITS VALUE - which holds for every coefficient a baseline file can carry (+-1023) with quantisers up to 2,
 * dense blocks included, and far beyond for what encoders write.  tests/golden/jpeg_synthetic.npz holds jpgd's output
 * for every last zigzag position in every component (each Row / Col pair, each of the fifteen P_Q / R_S instantiations)
 * and for dense blocks at that limit, tests/golden/texture_files.npz for files an encoder wrote.
 *
 * No floating point anywhere.  Sums that only a corrupt file can push past 32 bits wrap (unsigned arithmetic) instead of
 * being undefined; every 16-bit truncation is an explicit cast.  Out there the general forms and jpgd part: a shortcut
 * never forms the sum that wraps here (Col<1> only descales row 0 of the first pass, the general column pass shifts it
 * left by 13 first), and jpgd's own general forms are undefined.  The same npz pins the engine's bytes for such files
 * (its wrap tier); they are not jpgd's.
 */
#pragma once

#if defined(__HIPCC__)
#define JPX_HD __host__ __device__
#else
#define JPX_HD
#endif

namespace jpx
{
typedef unsigned int u32;

/* blocks of one MCU in scan order: the luma blocks row by row, then Cb, then Cr (ITU T.81 A.2.3) */
JPX_HD inline int blocksPerMcu(int lumaH, int lumaV) { return lumaH * lumaV + 2; }
/* 8x8 sample blocks the stage produces per MCU: 2x2 chroma comes out at full resolution (four blocks per component) */
JPX_HD inline int outputBlocksPerMcu(int lumaH, int lumaV) { return lumaV == 2 ? 12 : lumaH * lumaV + 2; }
/* the sampling factors the stage implements: 1x1, 2x1, 2x2 */
JPX_HD inline bool samplingSupported(int lumaH, int lumaV)
{
    return (lumaH == 1 && lumaV == 1) || (lumaH == 2 && lumaV == 1) || (lumaH == 2 && lumaV == 2);
}

JPX_HD inline short dequantise(short coefficient, unsigned short q)
{
    return (short)((int)coefficient * (int)q);
}

JPX_HD inline int clamp255(int i)
{
    return i < 0 ? 0 : (i > 255 ? 255 : i);
}

/* jpgd.cpp:120 DESCALE; the sum is reinterpreted as signed before the arithmetic shift */
JPX_HD inline int descale(u32 x, int n)
{
    return (int)(x + (1u << (n - 1))) >> n;
}

/* The 1-D inverse DCT both passes share (jpgd.cpp:136-160, constants :107-118 with CONST_BITS 13): eight inputs to the
 * eight sums out[0..7] that the passes then descale. */
JPX_HD inline void idct1d(const int in[8], u32 out[8])
{
    const u32 z2 = (u32)in[2], z3 = (u32)in[6];
    const u32 z1 = (z2 + z3) * 4433u;
    const u32 tmp2 = z1 - z3 * 15137u;
    const u32 tmp3 = z1 + z2 * 6270u;
    const u32 tmp0 = ((u32)in[0] + (u32)in[4]) << 13;
    const u32 tmp1 = ((u32)in[0] - (u32)in[4]) << 13;
    const u32 tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    const u32 atmp0 = (u32)in[7], atmp1 = (u32)in[5], atmp2 = (u32)in[3], atmp3 = (u32)in[1];
    const u32 bz1 = atmp0 + atmp3, bz2 = atmp1 + atmp2, bz3 = atmp0 + atmp2, bz4 = atmp1 + atmp3;
    const u32 bz5 = (bz3 + bz4) * 9633u;
    const u32 az1 = 0u - bz1 * 7373u;
    const u32 az2 = 0u - bz2 * 20995u;
    const u32 az3 = bz5 - bz3 * 16069u;
    const u32 az4 = bz5 - bz4 * 3196u;
    const u32 btmp0 = atmp0 * 2446u + az1 + az3;
    const u32 btmp1 = atmp1 * 16819u + az2 + az4;
    const u32 btmp2 = atmp2 * 25172u + az2 + az3;
    const u32 btmp3 = atmp3 * 12299u + az1 + az4;
    out[0] = tmp10 + btmp3;
    out[7] = tmp10 - btmp3;
    out[1] = tmp11 + btmp2;
    out[6] = tmp11 - btmp2;
    out[2] = tmp12 + btmp1;
    out[5] = tmp12 - btmp1;
    out[3] = tmp13 + btmp0;
    out[4] = tmp13 - btmp0;
}

/* first pass, one row of a dequantised block: CONST_BITS - PASS1_BITS = 11 (jpgd.cpp:162-169) */
JPX_HD inline void idctRow(const short row[8], int out[8])
{
    int in[8];
    u32 sums[8];
    for (int i = 0; i < 8; ++i)
        in[i] = row[i];
    idct1d(in, sums);
    for (int i = 0; i < 8; ++i)
        out[i] = descale(sums[i], 11);
}

/* second pass, one column of the first pass's results: +128, CONST_BITS + PASS1_BITS + 3 = 18, clamped
 * (jpgd.cpp:121 DESCALE_ZEROSHIFT, :239-261) */
JPX_HD inline void idctColumn(const int column[8], unsigned char out[8])
{
    u32 sums[8];
    idct1d(column, sums);
    for (int i = 0; i < 8; ++i)
        out[i] = (unsigned char)clamp255(descale(sums[i] + (128u << 18), 18));
}

/* 2x2 chroma in the frequency domain.  Both passes of jpgd's P_Q / R_S (jpgd.cpp:797-985) are the same step applied
 * along one axis of the block: of the eight coefficients v[0..7] along that axis, the even ones pass through and the
 * odd ones are folded by one of four 4-term rows with 10 fractional bits (F(x) = (int)(x * 1024 + .5f), which
 * truncates towards zero: F(-0.352443f) is -360), rounded by D() = (x + 512) >> 10.  Step t = 0..3 yields the pair
 *   t even: (v[2t], fold_t)     t odd: (fold_t, v[2t])
 * where the first of the pair goes to jpgd's X0.. / P / R and the second to X1.. / Q / S. */
JPX_HD inline void upsampleStep(int t, const int v[8], int *first, int *second)
{
    /* rows in the order of t: (0.906127, -0.318190, 0.212608, -0.180240), (0.415735, 0.791065, -0.352443, 0.277785),
     * (-0.074658, 0.513280, 0.768178, -0.375330), (0.022887, -0.097545, 0.490393, 0.865723) */
    const int k0 = t == 0 ? 928 : (t == 1 ? 426 : (t == 2 ? -75 : 23));
    const int k1 = t == 0 ? -325 : (t == 1 ? 810 : (t == 2 ? 526 : -99));
    const int k2 = t == 0 ? 218 : (t == 1 ? -360 : (t == 2 ? 787 : 502));
    const int k3 = t == 0 ? -184 : (t == 1 ? 284 : (t == 2 ? -383 : 887));
    const int fold = (k0 * v[1] + k1 * v[3] + k2 * v[5] + k3 * v[7] + 512) >> 10;
    const int pass = v[2 * t];
    *first = (t & 1) ? fold : pass;
    *second = (t & 1) ? pass : fold;
}

/* The four coefficients at column a, row j (both 0..3) of the four expanded blocks - upper left, upper right, lower left,
 * lower right of the 16x16 MCU - from P, Q, R, S at (a, j): jpgd.cpp:1763-1784 with Matrix44::add_and_store /
 * sub_and_store (:763-783), which truncate to 16 bits. */
JPX_HD inline void upsampleCombine(int p, int q, int r, int s, short out[4])
{
    const int a = p + q, b = p - q, c = r + s, d = r - s;
    out[0] = (short)(a + c);
    out[1] = (short)(a - c);
    out[2] = (short)(b + d);
    out[3] = (short)(b - d);
}

/* jpgd.cpp:1619-1629 (create_look_ups, FIX(x) = (int)(x * 65536 + 0.5f): 1.402 -> 91881, 1.772 -> 116130,
 * 0.71414 -> 46802, 0.34414 -> 22554) and :2254-2256 */
JPX_HD inline void colour(int y, int cb, int cr, unsigned char rgb[3])
{
    const int kb = cb - 128, kr = cr - 128;
    rgb[0] = (unsigned char)clamp255(y + ((91881 * kr + 32768) >> 16));
    rgb[1] = (unsigned char)clamp255(y + ((-46802 * kr - 22554 * kb + 32768) >> 16));
    rgb[2] = (unsigned char)clamp255(y + ((116130 * kb + 32768) >> 16));
}

/* Where pixel (x, y) of an MCU finds its three samples among the MCU's output blocks (each 64 bytes, row-major):
 * byte offsets from the MCU's first output block.  1x1 and 2x2 read all three at the same place of their own blocks
 * (jpgd.cpp:2237-2252, expanded_convert; 1x1 is H1V1Convert, :2031-2055); 2x1 halves x for chroma (:2058-2100). */
JPX_HD inline void sampleOffsets(int lumaH, int lumaV, int x, int y, int *offY, int *offCb, int *offCr)
{
    const int lumaBlocks = lumaH * lumaV;
    const int within = (y & 7) * 8 + (x & 7);
    const int block = (y >> 3) * lumaH + (x >> 3);
    *offY = block * 64 + within;
    if (lumaH == 2 && lumaV == 1)
    {
        *offCb = 2 * 64 + y * 8 + (x >> 1);
        *offCr = 3 * 64 + y * 8 + (x >> 1);
    }
    else
    {
        *offCb = (lumaBlocks + block) * 64 + within;
        *offCr = (2 * lumaBlocks + block) * 64 + within;
    }
}

/* the texture is stored turned by 180 degrees: pixel order reversed, R, G, B kept within a pixel (reference:
 * ImageLoader.cpp:170-190) */
JPX_HD inline long turnedPixel(int width, int height, int x, int y)
{
    return (long)width * height - 1 - ((long)y * width + x);
}
} // namespace jpx
