"""Generates tests/golden/jpeg_encoder.npz, which tests/test_jpeg_encoder.py and tests/test_jpeg_encoder_gpu.py load.

Run where the reference's tree exists (SOLR_REFERENCE, default /root/reference):

    python tests/golden/make_jpeg_encoder_fixtures.py

The screenshot writer (csrc/jpeg_encode.h, k_jpegCoefficients, host/JpegWriter.cpp) is held to the reference's own
encoder, solr/images/jpge.cpp, on pictures chosen for the paths they reach.  Three parts:

    the reference   jpge.cpp with a few lines of driver, compiled into a temporary directory outside the repository and
                    run on every picture with every sampling and quality listed below: `file/<name>` is what it wrote
    the model       the pixel stage - colour conversion, the edge rule, the block loads, the forward DCT, quantisation -
                    in numpy int64, which sees whether an operand of jpge's DCT_MUL leaves the 16 bits it is cast to
    the coder       a baseline entropy coder with the four standard tables and jpge's marker order

Per file the script asserts that model -> coder reproduces jpge's file byte for byte.  Huffman coding is injective, so
the model's blocks are then the ones jpge quantised: `blocks/<name>` (int16, blocks x 64 in MCU order, each in zigzag
order, as solr_hip_rgb_to_jpeg_blocks gives them).  It also asserts that no DCT_MUL operand left 16 bits.

A name is <picture>__<sampling>_q<quality>[_turned][_bgr]; `pixels/<picture>` (uint8, height x width x 3) is what the
encoder under test is handed, `params/<name>` (int32) width, height, luma H, luma V, quality, turned, swapRedBlue.  For
the turned / bgr names jpge was run on the pixels reordered in numpy by the rule of GPUKernel::generateScreenshot:
destination pixel p takes source pixel N - p (N itself clamped to N - 1), first and third channel swapped for bgr.

Data only: nothing compiled and none of the reference's source is written into the repository.  The output is the same
bytes on every run."""
import io
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import zipfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("SOLR_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "jpeg_encoder.npz")
LIMIT = 256 * 1024

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "jpge.h"
int main(int argc, char **argv)
{
    if (argc != 7)
        return 2;
    const int width = atoi(argv[3]), height = atoi(argv[4]);
    std::vector<unsigned char> pixels((size_t)width * height * 3);
    FILE *in = fopen(argv[1], "rb");
    if (!in || fread(pixels.data(), 1, pixels.size(), in) != pixels.size())
        return 3;
    fclose(in);
    jpge::params p;
    p.m_quality = atoi(argv[5]);
    p.m_subsampling = (jpge::subsampling_t)atoi(argv[6]);
    return jpge::compress_image_to_jpeg_file(argv[2], width, height, 3, pixels.data(), p) ? 0 : 1;
}
"""

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
SAMPLINGS = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}
JPGE_SUBSAMPLING = {(1, 1): 1, (2, 1): 2, (2, 2): 3}

# ITU T.81 annex K.1 in zigzag order, as jpge keeps them (jpge.cpp:58-65)
LUMA_QUANT = np.array([16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29,
                       40, 58, 51, 61, 60, 57, 51, 56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95,
                       98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99])
CHROMA_QUANT = np.array([17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66] + [99] * 50)

# ITU T.81 annex K.3: (BITS, HUFFVAL) of the DC and AC tables for luminance and chrominance
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


def grid(width, height, h, v):
    """MCUs per row, MCU rows, blocks per MCU"""
    return -(-width // (8 * h)), -(-height // (8 * v)), h * v + 2


def reordered(pixels, turned, bgr):
    """what GPUKernel::generateScreenshot hands the encoder (reference: GPUKernel.cpp:2819-2848)"""
    height, width, _ = pixels.shape
    flat = pixels.reshape(-1, 3)
    if turned:
        n = len(flat)
        flat = flat[np.minimum(n - np.arange(n), n - 1)]
    if bgr:
        flat = flat[:, ::-1]
    return np.ascontiguousarray(flat.reshape(height, width, 3))


def quant_tables(quality):
    """(2, 64), zigzag order: jpge.cpp:565-578"""
    scale = 5000 // quality if quality < 50 else 200 - quality * 2
    return np.stack([np.clip((base * scale + 50) // 100, 1, 255) for base in (LUMA_QUANT, CHROMA_QUANT)])


# ---- the model ------------------------------------------------------------------------------------------------------
class Model:
    def __init__(self):
        self.largest_operand = 0

    def mul(self, v, c):
        """DCT_MUL: the operand is cast to 16 bits; the largest one is noted, the cast itself is applied"""
        if v.size:
            self.largest_operand = max(self.largest_operand, int(np.abs(v).max()))
        return (((v + 2 ** 15) % 2 ** 16) - 2 ** 15) * c

    def dct1d(self, s):
        """(..., 8) -> (..., 8) sums, jpge.cpp:166-191"""
        s = [s[..., i] for i in range(8)]
        t0, t7, t1, t6 = s[0] + s[7], s[0] - s[7], s[1] + s[6], s[1] - s[6]
        t2, t5, t3, t4 = s[2] + s[5], s[2] - s[5], s[3] + s[4], s[3] - s[4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        u1 = self.mul(t12 + t13, 4433)
        s2 = u1 + self.mul(t13, 6270)
        s6 = u1 + self.mul(t12, -15137)
        u1, u2, u3, u4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = self.mul(u3 + u4, 9633)
        t4, t5, t6, t7 = self.mul(t4, 2446), self.mul(t5, 16819), self.mul(t6, 25172), self.mul(t7, 12299)
        u1, u2 = self.mul(u1, -7373), self.mul(u2, -20995)
        u3, u4 = self.mul(u3, -16069) + z5, self.mul(u4, -3196) + z5
        out = np.stack([t10 + t11, t7 + u1 + u4, s2, t6 + u2 + u3, t10 - t11, t5 + u2 + u4, s6, t4 + u1 + u3], axis=-1)
        assert np.abs(out).max() < 2 ** 31
        return out

    @staticmethod
    def descale(x, n):
        return (x + (1 << (n - 1))) >> n

    def dct(self, blocks):
        """(n, 8, 8) samples - 128 -> (n, 8, 8) coefficients: rows first, then columns (jpge.cpp:193-223)"""
        plain = np.array([True, False, False, False, True, False, False, False])
        rows = self.dct1d(blocks)
        rows = np.where(plain, rows << 2, self.descale(rows, 11))
        columns = self.dct1d(np.swapaxes(rows, 1, 2))
        columns = np.where(plain, self.descale(columns, 5), self.descale(columns, 18))
        return np.swapaxes(columns, 1, 2)

    def blocks(self, pixels, sampling, quality):
        """(height, width, 3) RGB as jpge receives it -> (blocks, 64) int16 in MCU order, zigzag order inside a block"""
        h, v = sampling
        height, width, _ = pixels.shape
        per_row, rows, per_mcu = grid(width, height, h, v)
        r, g, b = (pixels[..., i].astype(np.int64) for i in range(3))
        ycc = np.stack([(r * 19595 + g * 38470 + b * 7471 + 32768) >> 16,
                        np.clip(128 + ((r * -11059 + g * -21709 + b * 32768 + 32768) >> 16), 0, 255),
                        np.clip(128 + ((r * 32768 + g * -27439 + b * -5329 + 32768) >> 16), 0, 255)], axis=-1)
        assert ycc[..., 0].max() <= 255
        ycc = np.pad(ycc, ((0, rows * 8 * v - height), (0, per_row * 8 * h - width), (0, 0)), mode="edge")
        luma = ycc[..., 0] - 128
        if (h, v) == (1, 1):
            chroma = ycc[..., 1:] - 128
        elif (h, v) == (2, 1):
            chroma = ((ycc[:, 0::2, 1:] + ycc[:, 1::2, 1:]) >> 1) - 128
        else:
            total = ycc[0::2, 0::2, 1:] + ycc[0::2, 1::2, 1:] + ycc[1::2, 0::2, 1:] + ycc[1::2, 1::2, 1:]
            yy, xx = np.indices(total.shape[:2])
            chroma = ((total + (2 * ((yy + xx) & 1))[..., None]) >> 2) - 128

        def tiles(plane):                      # (8 R, 8 C) -> (R, C, 8, 8)
            return plane.reshape(plane.shape[0] // 8, 8, plane.shape[1] // 8, 8).transpose(0, 2, 1, 3)
        y = tiles(luma).reshape(rows, v, per_row, h, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(rows, per_row, h * v, 8, 8)
        mcus = np.concatenate([y, tiles(chroma[..., 0])[:, :, None], tiles(chroma[..., 1])[:, :, None]], axis=2)
        coefficients = self.dct(mcus.reshape(-1, 8, 8)).reshape(-1, per_mcu, 64)[:, :, ZIGZAG]
        q = quant_tables(quality)[np.array([0] * (h * v) + [1, 1])][None]
        magnitude = np.abs(coefficients) + (q >> 1)
        assert magnitude.max() <= 16384 + 127
        quantised = np.where(magnitude < q, 0, np.sign(coefficients) * (magnitude // q))
        return quantised.reshape(-1, 64).astype(np.int16)


# ---- the coder ------------------------------------------------------------------------------------------------------
def huffman_codes(bits, values):
    """symbol -> (code, length): ITU T.81 annex C"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[values[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


class Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, length):
        self.acc = (self.acc << length) | value
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1


def write_jpeg(width, height, sampling, quality, blocks):
    """jpge's file for these blocks: emit_markers (jpge.cpp:517-525), code_coefficients_pass_two (:883-952),
    terminate_pass_two (:1032-1039)"""
    h, v = sampling
    per_row, rows, per_mcu = grid(width, height, h, v)
    assert blocks.shape == (per_row * rows * per_mcu, 64)
    quant = quant_tables(quality)
    d = bytearray(b"\xff\xd8\xff\xe0" + struct.pack(">H", 16) + b"JFIF\x00\x01\x01\x00" + struct.pack(">HH", 1, 1) +
                  b"\x00\x00")
    for i in range(2):
        d += b"\xff\xdb" + struct.pack(">HB", 67, i) + bytes(int(x) for x in quant[i])
    d += b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, height, width, 3) + bytes([1, (h << 4) | v, 0, 2, 0x11, 1, 3, 0x11, 1])
    for (bits, values), index in ((DC_LUMA, 0x00), (AC_LUMA, 0x10), (DC_CHROMA, 0x01), (AC_CHROMA, 0x11)):
        d += b"\xff\xc4" + struct.pack(">HB", 19 + len(values), index) + bytes(bits) + bytes(values)
    d += b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    tables = [(huffman_codes(*DC_LUMA), huffman_codes(*AC_LUMA)), (huffman_codes(*DC_CHROMA), huffman_codes(*AC_CHROMA))]
    bits = Bits()
    prediction = [0, 0, 0]
    for index, block in enumerate(blocks.tolist()):
        b = index % per_mcu
        c = 0 if b < h * v else b - h * v + 1
        dc, ac = tables[c > 0]
        difference = block[0] - prediction[c]
        prediction[c] = block[0]
        size = abs(difference).bit_length()
        bits.put(*dc[size])
        if size:
            bits.put((difference if difference > 0 else difference - 1) & ((1 << size) - 1), size)
        run = 0
        for value in block[1:]:
            if value == 0:
                run += 1
                continue
            while run >= 16:
                bits.put(*ac[0xF0])
                run -= 16
            size = abs(value).bit_length()
            bits.put(*ac[(run << 4) | size])
            bits.put((value if value > 0 else value - 1) & ((1 << size) - 1), size)
            run = 0
        if run:
            bits.put(*ac[0x00])
    bits.put(0x7F, 7)
    return bytes(d) + bytes(bits.out) + b"\xff\xd9"


# ---- the pictures ---------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (4, 1), (17, 16), (16, 17), (37, 21), (40, 40), (4096, 1), (2, 4096)]


def picture(content, width, height):
    rng = np.random.RandomState(zlib.crc32(("%s_%dx%d" % (content, width, height)).encode()))
    yy, xx = np.indices((height, width))
    if content == "noise":
        return rng.randint(0, 256, (height, width, 3)).astype(np.uint8)
    if content == "ramp":
        span = max(width + height - 2, 1)
        return np.stack([255 * (xx + yy) // span, 255 * xx // max(width - 1, 1), 255 - 255 * yy // max(height - 1, 1)],
                        axis=-1).astype(np.uint8)
    if content == "constant":
        return np.full((height, width, 3), (90, 160, 30), np.uint8)
    if content in ("checker1", "checker8"):
        period = int(content[-1])
        return np.repeat((255 * ((xx // period + yy // period) & 1))[..., None], 3, axis=-1).astype(np.uint8)
    if content in ("red", "green", "blue"):
        out = np.zeros((height, width, 3), np.uint8)
        out[..., ("red", "green", "blue").index(content)] = 255
        return out
    if content == "edge":                 # the last column and the last row differ sharply from their neighbours
        out = np.full((height, width, 3), (40, 40, 200), np.uint8)
        out[:, -1] = (255, 230, 0)
        out[-1, :] = (0, 255, 40)
        return out
    raise KeyError(content)


CONTENTS = ["noise", "ramp", "constant", "checker1", "checker8", "red", "green", "blue", "edge"]


def cases():
    """[(picture name, content, width, height, sampling name, quality, turned, bgr)]: 2x2 at quality 85 with every size
    and every content; every other sampling and quality on a few of them; the two flags on three"""
    out = []

    def add(content, size, s="420", quality=85, turned=0, bgr=0):
        entry = ("%s_%dx%d" % (content, size[0], size[1]), content, size[0], size[1], s, quality, turned, bgr)
        if entry not in out:
            out.append(entry)

    long_content = {(4096, 1): "ramp", (2, 4096): "edge"}      # (noise that long would not fit the size limit)
    for size in SIZES:
        add(long_content.get(size, "noise"), size)
    for content in CONTENTS:
        add(content, (37, 21))
        add(content, (17, 16))
    add("checker8", (40, 40))
    add("checker1", (16, 17))
    add("noise", (4096, 1), quality=1)
    add("checker8", (2, 4096))
    for s in ("444", "422"):
        for size in ((1, 1), (4, 1), (17, 16), (16, 17), (37, 21), (40, 40)):
            add("noise", size, s)
        for content in ("checker1", "checker8", "blue", "red", "edge", "constant"):
            add(content, (37, 21), s)
        add("ramp", (4096, 1), s)
        add("edge", (2, 4096), s)
    for quality in (1, 49, 50, 100):
        for s in SAMPLINGS:
            add("noise", (37, 21), s, quality)
        add("checker1", (17, 16), "420", quality)
        add("ramp", (40, 40), "420", quality)
    for content, size in (("noise", (37, 21)), ("edge", (17, 16)), ("ramp", (40, 40)), ("noise", (1, 1))):
        add(content, size, turned=1)
        add(content, size, turned=1, bgr=1)
        add(content, size, bgr=1)
    add("noise", (37, 21), "422", 50, turned=1, bgr=1)
    add("noise", (37, 21), "444", 100, turned=1)
    return out


def save(path, arrays):
    """an .npz as numpy.savez_compressed writes it, without the time of day in it"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            buffer = io.BytesIO()
            np.lib.format.write_array(buffer, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buffer.getvalue())


def main():
    arrays = {}
    tmp = tempfile.mkdtemp(prefix="jpeg_encoder_")
    try:
        images = os.path.join(REFERENCE, "solr", "images")
        with open(os.path.join(tmp, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        exe = os.path.join(tmp, "encode")
        subprocess.run(["g++", "-O1", "-w", "-I", images, "-o", exe, os.path.join(tmp, "driver.cpp"),
                        os.path.join(images, "jpge.cpp")], check=True)
        largest = 0
        for pic, content, width, height, s, quality, turned, bgr in cases():
            name = "%s__%s_q%d%s%s" % (pic, s, quality, "_turned" if turned else "", "_bgr" if bgr else "")
            pixels = picture(content, width, height)
            arrays["pixels/" + pic] = pixels
            seen = reordered(pixels, turned, bgr)
            raw, out = os.path.join(tmp, "pixels.bin"), os.path.join(tmp, "out.jpg")
            seen.tofile(raw)
            subprocess.run([exe, raw, out, str(width), str(height), str(quality), str(JPGE_SUBSAMPLING[SAMPLINGS[s]])],
                           check=True)
            data = open(out, "rb").read()
            os.remove(out)
            model = Model()
            blocks = model.blocks(seen, SAMPLINGS[s], quality)
            assert model.largest_operand < 2 ** 15, (name, model.largest_operand)
            largest = max(largest, model.largest_operand)
            mine = write_jpeg(width, height, SAMPLINGS[s], quality, blocks)
            assert mine == data, "%s: model -> coder differs from jpge's file (%d / %d bytes)" % (name, len(mine), len(data))
            arrays["file/" + name] = np.frombuffer(data, np.uint8)
            arrays["blocks/" + name] = blocks
            arrays["params/" + name] = np.array([width, height, SAMPLINGS[s][0], SAMPLINGS[s][1], quality, turned, bgr],
                                                np.int32)
            print("%-44s %7d bytes %6d blocks, largest |coefficient| %5d" % (name, len(data), len(blocks),
                                                                            int(np.abs(blocks).max())))
    finally:
        shutil.rmtree(tmp)
    save(OUT, arrays)
    size = os.path.getsize(OUT)
    print("%s: %d files, %d bytes; largest DCT_MUL operand %d" % (OUT, sum(k.startswith("file/") for k in arrays), size,
                                                                largest))
    assert size <= LIMIT, "the npz must stay within %d bytes" % LIMIT


if __name__ == "__main__":
    sys.exit(main())
