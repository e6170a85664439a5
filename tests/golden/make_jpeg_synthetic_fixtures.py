"""Generates tests/golden/textures/synthetic/*.jpg and tests/golden/jpeg_synthetic.npz, which
tests/test_jpeg_synthetic.py and tests/test_jpeg_synthetic_gpu.py load.

Run where the reference's tree exists (SOLR_REFERENCE, default /root/reference):

    python tests/golden/make_jpeg_synthetic_fixtures.py

The files of tests/golden/textures/ were written by an encoder from smooth pictures, so they reach few of the paths of the
JPEG pixel stage (csrc/jpeg_pixels.h, k_jpegPixels) and of the Huffman stage (host/ImageLoader.cpp).  The files made here
are written from COEFFICIENT BLOCKS chosen for the paths they reach: every last zigzag position in every component, the
clamps, widths that take the dword store path or not, one-pixel images, long rows and columns of workgroups, ZRL runs to
coefficient 63, blocks without an end-of-block code, DC differences of category 11, restart markers past RST7, stuffed
0xFF bytes.  Three parts:

    the writer      a baseline JPEG writer: three components in one interleaved scan, one DC table with the 16 categories
                    as 5-bit codes, one AC table with EOB, ZRL and every (run, size >= 1) as 8-bit codes
    the reference   the reference's solr/images/jpgd.cpp with a few lines of driver, compiled into a temporary directory
                    outside the repository - twice, the second time with -fsanitize=signed-integer-overflow.  Expected
                    bytes are the plain build's decoded[::-1, ::-1, :] (the reference's ImageLoader::loadJPEG turns the
                    picture by 180 degrees); the sanitised build must give the same bytes and tells whether jpgd's own
                    arithmetic stayed defined
    the model       the general two-pass inverse DCT and the 2x2 chroma expansion evaluated in numpy int64, which sees
                    whether every sum fits in 32 bits and every 16-bit store (dequantise, add_and_store / sub_and_store)
                    keeps its value

A file is in the EXACT tier when the sanitised jpgd reports no signed overflow and the model keeps every sum within int32
and every 16-bit store untruncated; there the loader is held to jpgd's bytes.  The WRAP tier (wrap_*: +-1023 with
quantisers up to 255) is beyond that: jpgd's sparse variants (Col<1>, Row<1>, ...) skip sums that the general forms make,
so the two differ once a sum wraps.  There the loader is held to `wrapped/<name>`: the model's output with the engine's
documented semantics - sums modulo 2^32, reinterpreted as signed where they are shifted, 16-bit stores as explicit casts;
`jpgd/<name>` holds jpgd's bytes for information.  The script asserts that every file lands in the tier it was written
for, and that the model reproduces jpgd byte for byte on every exact-tier file.

Per file the npz holds expected/<name> (or wrapped/<name> and jpgd/<name>), coefficients/<name> (int16, blocks x 64 in
scan order, each block row-major, as solr_hip_jpeg_to_rgb takes them) and frame/<name> (int32: width, height, luma H, luma
V, then the three quantisation tables row-major).  Data only: nothing compiled and none of the reference's source is
written into the repository.  The output is the same bytes on every run."""
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
SYNTHETIC = os.path.join(HERE, "textures", "synthetic")
REFERENCE = os.environ.get("SOLR_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "jpeg_synthetic.npz")

DRIVER = r"""
#include <cstdio>
#include "jpgd.h"
int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    int width = 0, height = 0, actual = 0;
    unsigned char *pixels = jpgd::decompress_jpeg_image_from_file(argv[1], &width, &height, &actual, 3);
    if (!pixels)
        return 1;
    FILE *out = fopen(argv[2], "wb");
    int header[2] = {width, height};
    fwrite(header, sizeof(header), 1, out);
    fwrite(pixels, 1, (size_t)width * height * 3, out);
    fclose(out);
    return 0;
}
"""

# position in the block (row-major) of the k-th coefficient of the zigzag sequence (ITU T.81 figure A.6)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
SAMPLINGS = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}


def grid(width, height, h, v):
    """MCUs per row, MCU rows, blocks per MCU"""
    return -(-width // (8 * h)), -(-height // (8 * v)), h * v + 2


# ---- the writer -----------------------------------------------------------------------------------------------------
EOB, ZRL = 0x00, 0xF0
AC_SYMBOLS = [EOB, ZRL] + [(run << 4) | size for run in range(16) for size in range(1, 16)]
AC_CODE = {symbol: code for code, symbol in enumerate(AC_SYMBOLS)}          # 242 codes of 8 bits


class Bits:
    """the entropy-coded segment: bits first-in at the top of a byte, a zero byte stuffed after every 0xFF"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, length):
        assert 0 <= value < (1 << length)
        self.acc = (self.acc << length) | value
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def pad(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)

    def marker(self, byte):
        self.pad()
        self.out += bytes([0xFF, byte])


def magnitude(bits, value, size):
    if size:
        bits.put(value if value > 0 else value + (1 << size) - 1, size)


def write_jpeg(width, height, sampling, quant, blocks, restart_interval=0, zrl_before_eob=()):
    """`quant`: (3, 64) row-major, 1..255; `blocks`: (MCUs * blocks per MCU, 64) in scan order, each row-major;
    `zrl_before_eob`: blocks that get a ZRL code in front of their end-of-block code, as no encoder writes it"""
    h, v = sampling
    per_row, rows, per_mcu = grid(width, height, h, v)
    assert blocks.shape == (per_row * rows * per_mcu, 64) and quant.shape == (3, 64)
    assert quant.min() >= 1 and quant.max() <= 255
    d = bytearray(b"\xff\xd8")
    d += b"\xff\xdb" + struct.pack(">H", 2 + 3 * 65)
    for c in range(3):
        d += bytes([c]) + bytes(int(quant[c][ZIGZAG[k]]) for k in range(64))
    d += b"\xff\xc0" + struct.pack(">HBHHB", 8 + 3 * 3, 8, height, width, 3)
    d += bytes([1, (h << 4) | v, 0, 2, 0x11, 1, 3, 0x11, 2])
    dc_table = bytes([0x00] + [16 if length == 5 else 0 for length in range(1, 17)] + list(range(16)))
    ac_table = bytes([0x10] + [len(AC_SYMBOLS) if length == 8 else 0 for length in range(1, 17)] + AC_SYMBOLS)
    d += b"\xff\xc4" + struct.pack(">H", 2 + len(dc_table) + len(ac_table)) + dc_table + ac_table
    if restart_interval:
        d += b"\xff\xdd" + struct.pack(">HH", 4, restart_interval)
    d += b"\xff\xda" + struct.pack(">HB", 6 + 2 * 3, 3) + bytes([1, 0x00, 2, 0x00, 3, 0x00, 0, 63, 0])

    bits = Bits()
    prediction = [0, 0, 0]
    for index, block in enumerate(blocks):
        mcu, b = divmod(index, per_mcu)
        if b == 0 and mcu and restart_interval and mcu % restart_interval == 0:
            bits.marker(0xD0 + (mcu // restart_interval - 1) % 8)
            prediction = [0, 0, 0]
        c = 0 if b < h * v else b - h * v + 1
        difference = int(block[0]) - prediction[c]
        prediction[c] = int(block[0])
        size = abs(difference).bit_length()
        bits.put(size, 5)
        magnitude(bits, difference, size)
        run = 0
        for k in range(1, 64):
            value = int(block[ZIGZAG[k]])
            if value == 0:
                run += 1
                continue
            while run > 15:
                bits.put(AC_CODE[ZRL], 8)
                run -= 16
            size = abs(value).bit_length()
            bits.put(AC_CODE[(run << 4) | size], 8)
            magnitude(bits, value, size)
            run = 0
        if run:
            if index in zrl_before_eob:
                assert run >= 16
                bits.put(AC_CODE[ZRL], 8)
                run -= 16
            if run:                              # (a ZRL that reaches coefficient 63 ends the block by itself)
                bits.put(AC_CODE[EOB], 8)
    bits.pad()
    return bytes(d) + bytes(bits.out) + b"\xff\xd9", bytes(bits.out)


# ---- the model ------------------------------------------------------------------------------------------------------
class Model:
    """jpgd's general forms in int64 (jpgd.cpp: Row<8> / Col<8> :128-263, P_Q<8, 8> / R_S<8, 8> :797-985, Matrix44
    add_and_store / sub_and_store :763-783, H1V1Convert / H2V1Convert / expanded_convert :2031-2265).  It notes whether
    any sum left int32 or any 16-bit store lost bits; where one does, it goes on as the engine does: modulo 2^32, signed
    where shifted, 16-bit stores as casts."""

    def __init__(self):
        self.beyond32 = False
        self.truncated16 = False

    def s32(self, x):
        """a sum jpgd keeps in an int"""
        if x.size and (x.min() < -2 ** 31 or x.max() > 2 ** 31 - 1):
            self.beyond32 = True
        return x

    @staticmethod
    def wrap32(x):
        return ((x + 2 ** 31) % 2 ** 32) - 2 ** 31

    def store16(self, x):
        wrapped = ((x + 2 ** 15) % 2 ** 16) - 2 ** 15
        if (wrapped != x).any():
            self.truncated16 = True
        return wrapped

    def idct1d(self, v):
        """v: (..., 8) -> the eight sums before their descale"""
        s = self.s32
        c = [v[..., i] for i in range(8)]
        z2, z3 = c[2], c[6]
        z1 = s(s(z2 + z3) * 4433)
        tmp2 = s(z1 + s(z3 * -15137))
        tmp3 = s(z1 + s(z2 * 6270))
        tmp0 = s(s(c[0] + c[4]) * 8192)
        tmp1 = s(s(c[0] - c[4]) * 8192)
        tmp10, tmp13, tmp11, tmp12 = s(tmp0 + tmp3), s(tmp0 - tmp3), s(tmp1 + tmp2), s(tmp1 - tmp2)
        atmp0, atmp1, atmp2, atmp3 = c[7], c[5], c[3], c[1]
        bz1, bz2, bz3, bz4 = s(atmp0 + atmp3), s(atmp1 + atmp2), s(atmp0 + atmp2), s(atmp1 + atmp3)
        bz5 = s(s(bz3 + bz4) * 9633)
        az1 = s(bz1 * -7373)
        az2 = s(bz2 * -20995)
        az3 = s(s(bz3 * -16069) + bz5)
        az4 = s(s(bz4 * -3196) + bz5)
        btmp0 = s(s(s(atmp0 * 2446) + az1) + az3)
        btmp1 = s(s(s(atmp1 * 16819) + az2) + az4)
        btmp2 = s(s(s(atmp2 * 25172) + az2) + az3)
        btmp3 = s(s(s(atmp3 * 12299) + az1) + az4)
        return np.stack([s(tmp10 + btmp3), s(tmp11 + btmp2), s(tmp12 + btmp1), s(tmp13 + btmp0), s(tmp13 - btmp0),
                         s(tmp12 - btmp1), s(tmp11 - btmp2), s(tmp10 - btmp3)], axis=-1)

    def idct(self, blocks):
        """(n, 8, 8) dequantised coefficients -> (n, 8, 8) samples"""
        rows = self.wrap32(self.s32(self.idct1d(blocks) + (1 << 10))) >> 11
        sums = self.idct1d(np.swapaxes(rows, 1, 2))                 # [n, column, i]: i runs down the column
        sums = self.wrap32(self.s32(self.s32(sums + (128 << 18)) + (1 << 17))) >> 18
        return np.clip(np.swapaxes(sums, 1, 2), 0, 255)

    FOLD = np.array([[928, -325, 218, -184], [426, 810, -360, 284], [-75, 526, 787, -383], [23, -99, 502, 887]])

    def fold(self, v):
        """one pass of P_Q / R_S along the last axis: (..., 8) -> first (..., 4) and second (..., 4), see
        upsampleStep of csrc/jpeg_pixels.h.  F(x) = (int)(x * 1024 + .5f) truncates towards zero."""
        folded = self.s32(self.s32(v[..., 1::2] @ self.FOLD.T) + 512) >> 10
        passed = v[..., 0::2]
        odd = np.arange(4) % 2 == 1
        return np.where(odd, folded, passed), np.where(odd, passed, folded)

    def expand(self, blocks):
        """(n, 8, 8) dequantised chroma blocks of a 2x2 file -> (n, 4, 8, 8) samples: upper left, upper right, lower
        left, lower right of the 16x16 MCU"""
        x0, x1 = self.fold(blocks)                                  # [n, r, t]
        p, q = self.fold(np.swapaxes(x0, 1, 2))                     # [n, a, j]
        r, s = self.fold(np.swapaxes(x1, 1, 2))
        a, b, c, d = p + q, p - q, r + s, r - s
        out = np.zeros((blocks.shape[0], 4, 8, 8), np.int64)
        for k, m in enumerate((a + c, a - c, b + d, b - d)):
            out[:, k, :4, :4] = np.swapaxes(self.store16(m), 1, 2)  # row j, column a
        return self.idct(out.reshape(-1, 8, 8)).reshape(-1, 4, 8, 8)

    def decode(self, width, height, sampling, quant, blocks):
        """what the loader stores: (height, width, 3), turned by 180 degrees"""
        h, v = sampling
        per_row, rows, per_mcu = grid(width, height, h, v)
        luma = h * v
        mcus = blocks.astype(np.int64).reshape(per_row * rows, per_mcu, 64)
        component = np.array([0] * luma + [1, 2])
        mcus = self.store16(mcus * quant.astype(np.int64)[component][None]).reshape(-1, per_mcu, 8, 8)
        n = mcus.shape[0]
        y = self.idct(mcus[:, :luma].reshape(-1, 8, 8)).reshape(n, v, h, 8, 8)
        y = y.transpose(0, 1, 3, 2, 4).reshape(n, 8 * v, 8 * h)
        planes = [y]
        for c in (1, 2):
            if v == 2:
                e = self.expand(mcus[:, luma + c - 1]).reshape(n, 2, 2, 8, 8)
                planes.append(e.transpose(0, 1, 3, 2, 4).reshape(n, 16, 16))
            else:
                planes.append(np.repeat(self.idct(mcus[:, luma + c - 1]), h, axis=2))
        full = [p.reshape(rows, per_row, 8 * v, 8 * h).transpose(0, 2, 1, 3).reshape(rows * 8 * v, per_row * 8 * h)
                [:height, :width] for p in planes]
        yy, kb, kr = full[0], full[1] - 128, full[2] - 128
        rgb = np.stack([yy + ((91881 * kr + 32768) >> 16), yy + ((-46802 * kr - 22554 * kb + 32768) >> 16),
                        yy + ((116130 * kb + 32768) >> 16)], axis=-1)
        return np.ascontiguousarray(np.clip(rgb, 0, 255).astype(np.uint8)[::-1, ::-1, :])


# ---- the blocks -----------------------------------------------------------------------------------------------------
def last_positions(blocks):
    """the last non-zero zigzag position of every block (0: nothing beyond the DC coefficient)"""
    nonzero = blocks[:, ZIGZAG] != 0
    nonzero[:, 0] = True
    return 63 - np.argmax(nonzero[:, ::-1], axis=1)


def nonzero_values(rng, amplitude, n):
    return rng.randint(1, amplitude + 1, n) * rng.choice([-1, 1], n)


def make_blocks(rng, width, height, sampling, last, ac=12, dc=(200, 80)):
    """Every AC coefficient up to the block's last position non-zero, uniform in +-ac; DC uniform in +-dc[luma or
    chroma].  `last(block, component, mcu, luma_index)` gives the last zigzag position.  The default amplitudes are the
    "moderate" ones: with quantisers of 1..3 they leave well under 5 % of the decoded bytes at 0 or 255 for all three
    samplings (+-24 and +-300 / +-100 left 8.5 % of zag_444 there)."""
    h, v = sampling
    per_row, rows, per_mcu = grid(width, height, h, v)
    blocks = np.zeros((per_row * rows * per_mcu, 64), np.int16)
    luma_index = 0
    for index in range(len(blocks)):
        mcu, b = divmod(index, per_mcu)
        c = 0 if b < h * v else b - h * v + 1
        position = last(index, c, mcu, luma_index)
        luma_index += c == 0
        limit = dc[0] if c == 0 else dc[1]
        blocks[index, 0] = rng.randint(-limit, limit + 1)
        blocks[index, ZIGZAG[1:position + 1]] = nonzero_values(rng, ac, position)
    return blocks


def cycling(index, c, mcu, luma_index):
    return (luma_index if c == 0 else mcu if c == 1 else mcu + 32) % 64


def quantisers(rng, low, high):
    return rng.randint(low, high + 1, (3, 64)).astype(np.uint16)


def files():
    """name -> (tier, moderate, width, height, sampling, quant, blocks, writer options)"""
    out = {}

    def add(name, tier, moderate, width, height, s, quant, blocks, **options):
        out[name] = (tier, moderate, width, height, SAMPLINGS[s], quant, blocks, options)

    def rng_for(name, attempt=0):
        return np.random.RandomState(zlib.crc32(name.encode()) + attempt)

    def settled(name, width, height, s, build, **options):
        """a moderate file: `build(rng)` gives the blocks, the quantisers are 1..3.  At most 5 % of the picture's bytes
        may be 0 or 255, so that a comparison sees nearly every byte move; a seed that breaks that (one byte of the
        three of a 1x1 picture is 33 %) is passed over for the next one."""
        for attempt in range(64):
            rng = rng_for(name, attempt)
            quant = quantisers(rng, 1, 3)
            blocks = build(rng)
            picture = Model().decode(width, height, SAMPLINGS[s], quant, blocks)
            if np.isin(picture, (0, 255)).mean() <= 0.05:
                return add(name, "exact", True, width, height, s, quant, blocks, **options)
        raise AssertionError("%s: no seed keeps the saturated share within 5 %%" % name)

    def moderate(name, width, height, s, last=None, **options):
        settled(name, width, height, s, lambda rng: make_blocks(rng, width, height, SAMPLINGS[s],
                                                                 last or (lambda *_: rng.randint(0, 64))), **options)

    sizes = lambda *three: zip(("444", "422", "420"), three)
    for s, (w, h) in sizes((67, 61), (139, 61), (139, 125)):
        moderate("zag_" + s, w, h, s, cycling)
    for s, (w, h) in sizes((37, 39), (77, 39), (77, 79)):
        rng = rng_for("full_" + s)
        add("full_" + s, "exact", False, w, h, s, quantisers(rng, 1, 2),
            make_blocks(rng, w, h, SAMPLINGS[s], cycling, ac=1023, dc=(1023, 1023)))
    for s, (w, h) in sizes((20, 9), (36, 9), (36, 20)):
        moderate("dwords_" + s, w, h, s)
    # two 16x16 MCUs in one workgroup and a width that is no multiple of 4: the second MCU's last group of four pixels
    # hangs over the edge, and what it would write there lies in rows the first MCU wrote earlier in the same wave
    moderate("pair_420_21x9", 21, 9, "420")
    for s in SAMPLINGS:
        for w, h in ((1, 1), (3, 1), (4, 1), (5, 3)):
            moderate("tiny_%s_%dx%d" % (s, w, h), w, h, s)
    few = lambda index, *_: 2 + index % 2
    moderate("row_444_4096x1", 4096, 1, "444", few)
    moderate("column_420_2x4096", 2, 4096, "420", few)

    # -- the Huffman stage --
    name = "huffman_zrl_to_63_16x8"          # the only AC coefficient is the last one: ZRL, ZRL, ZRL, (14, size)

    def only_the_last(rng):
        blocks = make_blocks(rng, 16, 8, (1, 1), lambda *_: 0)
        blocks[:, 63] = nonzero_values(rng, 12, len(blocks))
        return blocks
    settled(name, 16, 8, "444", only_the_last)

    name = "huffman_no_eob_16x8"             # 63 non-zero AC coefficients: the block ends without an end-of-block code
    moderate(name, 16, 8, "444", lambda *_: 63)

    name = "huffman_zrl_then_eob_16x8"       # a ZRL in front of the end-of-block code; after position 47 the ZRL
    positions = [0, 1, 5, 20, 46, 47]        # reaches coefficient 63 and there is no end-of-block code
    moderate(name, 16, 8, "444", lambda index, *_: positions[index], zrl_before_eob=set(range(6)))

    name = "huffman_dc_category_11_24x24"    # DC -1023, +1023, ...: differences of +-2046
    rng = rng_for(name)
    blocks = make_blocks(rng, 24, 24, (1, 1), lambda *_: rng.randint(0, 64))
    for c in range(3):
        blocks[c::3, 0] = np.where(np.arange(9) % 2 == 0, -1023, 1023)
    add(name, "exact", False, 24, 24, "444", np.ones((3, 64), np.uint16), blocks)

    moderate("huffman_restart_444_32x24", 32, 24, "444", restart_interval=1)       # 12 MCUs: RST0 .. RST7, RST0 .. RST2
    moderate("huffman_restart_420_40x56", 40, 56, "420", restart_interval=1)       # 12 MCUs

    # byte-aligned codes whose magnitude bits are 0xFF: DC differences of +5, -5 (5 + 3 bits), then +255, which is the
    # code of (0, 8) and eight one bits (-255: eight zeros)
    blocks = np.zeros((27, 64), np.int16)
    for c in range(3):
        blocks[c::3, 0] = np.where(np.arange(9) % 2 == 0, 5, 0)
    blocks[:, ZIGZAG[1]] = 255 * (1 - 2 * (np.arange(27) // 3 % 2))
    blocks[:, ZIGZAG[2]] = 255
    add("huffman_stuffing_24x24", "exact", False, 24, 24, "444", np.ones((3, 64), np.uint16), blocks)

    # -- beyond 32 bits --
    for s, (w, h) in sizes((21, 13), (37, 13), (37, 21)):
        rng = rng_for("wrap_" + s)
        add("wrap_" + s, "wrap", False, w, h, s, quantisers(rng, 1, 255),
            make_blocks(rng, w, h, SAMPLINGS[s], lambda *_: 63, ac=1023, dc=(1023, 1023)))
    # Two coefficients a block and no 16-bit store truncated (1023 * 32 = 32736).  The first pass leaves up to
    # (32736 + 1.387 * 32736) * 4 = 312 564 in row 0, the only row that is not zero.  jpgd takes Col<1>, which only
    # descales that number; the general column pass shifts it left by 13 first, past 2^31.
    blocks = np.zeros((3, 64), np.int16)
    blocks[:, 0] = (1023, -1023, 1023)
    blocks[:, 1] = (1023, -1023, -1023)
    add("wrap_444_1x1", "wrap", False, 1, 1, "444", np.full((3, 64), 32, np.uint16), blocks)
    return out


# ---- the reference --------------------------------------------------------------------------------------------------
def build_decoders(tmp):
    images = os.path.join(REFERENCE, "solr", "images")
    with open(os.path.join(tmp, "driver.cpp"), "w") as f:
        f.write(DRIVER)
    built = []
    for exe, flags in (("decode", []), ("decode_sanitised", ["-fsanitize=signed-integer-overflow"])):
        exe = os.path.join(tmp, exe)
        subprocess.run(["g++", "-O1", "-w"] + flags + ["-I", images, "-o", exe, os.path.join(tmp, "driver.cpp"),
                                                      os.path.join(images, "jpgd.cpp")], check=True)
        built.append(exe)
    return built


def decode(exe, tmp, path):
    """the decoded picture and the number of places in jpgd where the sanitiser saw a signed overflow"""
    out = os.path.join(tmp, "pixels.bin")
    done = subprocess.run([exe, path, out], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    assert done.returncode == 0, (path, done.stderr)
    raw = open(out, "rb").read()
    w, h = struct.unpack("<2i", raw[:8])
    overflows = done.stderr.decode(errors="replace").count("signed integer overflow")
    return np.frombuffer(raw[8:], np.uint8).reshape(h, w, 3).copy(), overflows


def save(path, arrays):
    """an .npz as numpy.savez_compressed writes it, without the time of day in it"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buffer = io.BytesIO()
            np.lib.format.write_array(buffer, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buffer.getvalue())


def main():
    if os.path.isdir(SYNTHETIC):
        shutil.rmtree(SYNTHETIC)
    os.makedirs(SYNTHETIC)
    arrays = {}
    tmp = tempfile.mkdtemp(prefix="jpeg_synthetic_")
    try:
        plain, sanitised = build_decoders(tmp)
        print("%-32s %-5s %9s %9s %9s  %s" % ("file", "tier", "bytes", "overflows", "saturated", "differs from jpgd"))
        for name, (tier, moderate, width, height, sampling, quant, blocks, options) in files().items():
            data, entropy = write_jpeg(width, height, sampling, quant, blocks, **options)
            path = os.path.join(SYNTHETIC, name + ".jpg")
            with open(path, "wb") as f:
                f.write(data)
            assert len(data) < 64 * 1024, name
            decoded, _ = decode(plain, tmp, path)
            checked, overflows = decode(sanitised, tmp, path)
            jpgd = np.ascontiguousarray(decoded[::-1, ::-1, :])
            assert jpgd.shape == (height, width, 3), name
            model = Model()
            modelled = model.decode(width, height, sampling, quant, blocks)
            exact = overflows == 0 and not model.beyond32 and not model.truncated16
            assert exact == (tier == "exact"), "%s was written for the %s tier: %d overflows in jpgd, beyond 32 bits: " \
                "%s, 16-bit stores truncated: %s" % (name, tier, overflows, model.beyond32, model.truncated16)
            saturated = np.isin(jpgd, (0, 255)).mean()
            if tier == "exact":
                assert np.array_equal(decoded, checked), name
                assert np.array_equal(modelled, jpgd), "%s: the model differs from jpgd in the exact tier" % name
                assert not moderate or saturated <= 0.05, "%s: %.1f %% of jpgd's bytes are 0 or 255" % (
                    name, 100 * saturated)
                arrays["expected/" + name] = jpgd
            else:
                arrays["wrapped/" + name] = modelled
                arrays["jpgd/" + name] = jpgd
            if name == "huffman_stuffing_24x24":
                assert entropy.count(b"\xff\x00") >= 32, entropy.count(b"\xff\x00")
            arrays["coefficients/" + name] = blocks
            arrays["frame/" + name] = np.concatenate([[width, height, sampling[0], sampling[1]],
                                                      quant.ravel()]).astype(np.int32)
            print("%-32s %-5s %9d %9d %8.1f%%  %s" % (
                name, tier, len(data), overflows, 100 * saturated,
                "" if tier == "exact" else "%d of %d bytes" % ((modelled != jpgd).sum(), jpgd.size)))
    finally:
        shutil.rmtree(tmp)
    save(OUT, arrays)
    total = os.path.getsize(OUT) + sum(os.path.getsize(os.path.join(SYNTHETIC, n)) for n in os.listdir(SYNTHETIC))
    print("%s: %d arrays, %d bytes; with the .jpg files %d bytes" % (OUT, len(arrays), os.path.getsize(OUT), total))


if __name__ == "__main__":
    sys.exit(main())
