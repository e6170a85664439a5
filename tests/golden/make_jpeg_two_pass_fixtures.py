"""Generates tests/golden/jpeg_two_pass.npz, which tests/test_jpeg_two_pass.py and tests/test_jpeg_two_pass_gpu.py load.

Run where the reference's tree exists (SOLR_REFERENCE, default /root/reference):

    python tests/golden/make_jpeg_two_pass_fixtures.py

The optimised mode of the JPEG writer (csrc/jpeg_entropy.h optimiseTable, host/JpegWriter.cpp, k_jpegSymbolCounts and
k_jpegOptimiseTables) is held to the two-pass mode of the reference's encoder, solr/images/jpge.cpp
(params::m_two_pass_flag).  Two tiers, both made by a few lines of driver compiled against jpge.cpp in a temporary
directory outside the repository:

    the file tier    `file/<name>`: jpge's own file with m_two_pass_flag = true for every case of jpeg_encoder.npz - the same
                     pictures, parameters and reorderings (make_jpeg_encoder_fixtures.py: cases, picture, reordered); the
                     blocks it codes are that file's `blocks/<name>`
    the table tier   `table/<name>/counts` (uint32), `/bits` (uint8, 16), `/values` (uint8): optimize_huffman_table itself
                     (jpge.cpp:353-397) on the histograms of histograms() below - chosen for ties, the dummy symbol and the
                     16-bit limit, see there

Data only: nothing compiled and none of the reference's source is written into the repository.  The output is the same
bytes on every run."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_jpeg_encoder_fixtures as one_pass  # noqa: E402

REFERENCE = one_pass.REFERENCE
OUT = os.path.join(HERE, "jpeg_two_pass.npz")
LIMIT = 256 * 1024

FILE_DRIVER = r"""
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
    p.m_two_pass_flag = true;
    return jpge::compress_image_to_jpeg_file(argv[2], width, height, 3, pixels.data(), p) ? 0 : 1;
}
"""

# a histogram per line on standard input: the table's length, then that many counts; per line of output the 16 bits, then
# the values
TABLE_DRIVER = r"""
#include <cstdio>
#define private public
#include "jpge.h"
#undef private
int main()
{
    int length;
    while (scanf("%d", &length) == 1)
    {
        jpge::jpeg_encoder encoder;
        const int table = length == 12 ? 0 : 2;
        for (int i = 0; i < 256; ++i)
            encoder.m_huff_count[table][i] = 0;
        for (int i = 0; i < length; ++i)
            if (scanf("%u", &encoder.m_huff_count[table][i]) != 1)
                return 3;
        encoder.optimize_huffman_table(table, length);
        int total = 0;
        for (int l = 1; l <= 16; ++l)
        {
            printf("%d ", (int)encoder.m_huff_bits[table][l]);
            total += encoder.m_huff_bits[table][l];
        }
        for (int i = 0; i < total; ++i)
            printf("%d ", (int)encoder.m_huff_val[table][i]);
        printf("\n");
    }
    return 0;
}
"""


def fibonacci(n):
    """1, 2, 3, 5, 8 ...: the counts that make the deepest tree a total allows"""
    out = [1, 2]
    while len(out) < n:
        out.append(out[-1] + out[-2])
    return out[:n]


# the 18 symbols of "limit_18": the end of block, then (run 1, size 1 ... 8), then (run 0, size 1 ... 9) - symbols that
# coefficient blocks can be made of, the frequent ones a single position long (tests/jpeg_two_pass_cases.py makes them)
LIMIT_18_SYMBOLS = [0x00] + [0x10 + s for s in range(1, 9)] + [s for s in range(1, 10)]


def histograms():
    """[(name, counts)]: counts has 12 (a DC table) or 256 entries"""
    out = []

    def add(name, length, pairs):
        counts = np.zeros(length, np.uint32)
        for symbol, count in pairs:
            counts[symbol] = count
        out.append((name, counts))

    add("one_symbol_dc", 12, [(3, 7)])                          # one code of length 1
    add("one_symbol_ac", 256, [(0x00, 5)])
    add("one_symbol_count_1", 256, [(0xF0, 1)])                 # ... that ties with the dummy
    add("two_symbols", 256, [(0x01, 10), (0x11, 3)])
    add("two_symbols_equal", 12, [(0, 4), (11, 4)])
    add("dc_all_twelve", 12, [(i, c) for i, c in enumerate([120, 340, 560, 410, 300, 150, 90, 40, 12, 5, 2, 1])])
    add("dc_all_ones", 12, [(i, 1) for i in range(12)])         # every count ties with the dummy's
    add("ones_among_others", 256, [(5, 1), (9, 1), (200, 1), (0x11, 2), (0x21, 3), (0x00, 1), (0xF0, 40)])
    add("all_256_equal", 256, [(i, 7) for i in range(256)])     # 255 codes of 8 bits and one of 9
    add("all_256_ones", 256, [(i, 1) for i in range(256)])
    ties = []
    for start, n, count in ((0, 40, 3), (40, 50, 10), (100, 30, 100), (140, 20, 1), (200, 33, 10), (250, 6, 3)):
        ties += [(start + i, count) for i in range(n)]
    add("runs_of_ties", 256, ties)
    add("limit_18", 256, list(zip(LIMIT_18_SYMBOLS, fibonacci(18))))        # unlimited depth 18: the limit engages
    add("limit_22", 256, [(11 * i + 3, c) for i, c in enumerate(fibonacci(22))])
    add("limit_22_descending", 256, [(250 - 7 * i, c) for i, c in enumerate(fibonacci(22))])
    add("limit_12_dc_is_free", 12, list(enumerate(fibonacci(12))))          # depth 12: no limit in a DC table
    add("powers_of_two_27", 256, [(9 * i + 1, 1 << i) for i in range(27)])  # counts above 2^24: every radix digit is live
    # two long codes beside a short tree: the limit's repair step has several occupied lengths to choose from
    add("limit_repair_choice", 256, list(zip(range(10, 30), fibonacci(20))) + [(100 + i, 9000) for i in range(6)])
    rng = np.random.RandomState(20251)
    add("random_dc", 12, [(i, int(rng.randint(0, 5000))) for i in range(12)])
    used = rng.permutation(256)[:40]
    add("random_sparse", 256, [(int(i), int(rng.geometric(0.02))) for i in used])
    add("random_dense", 256, [(i, int(2 ** rng.uniform(0, 20))) for i in range(256)])
    add("random_small_counts", 256, [(i, int(rng.randint(0, 4))) for i in range(256)])
    return out


def main():
    arrays = {}
    tmp = tempfile.mkdtemp(prefix="jpeg_two_pass_")
    try:
        images = os.path.join(REFERENCE, "solr", "images")
        exes = {}
        for name, text in (("file", FILE_DRIVER), ("table", TABLE_DRIVER)):
            source = os.path.join(tmp, name + "_driver.cpp")
            with open(source, "w") as f:
                f.write(text)
            exes[name] = os.path.join(tmp, name)
            subprocess.run(["g++", "-O1", "-w", "-I", images, "-o", exes[name], source, os.path.join(images, "jpge.cpp")],
                           check=True)
        # ---- the file tier ----
        committed = np.load(one_pass.OUT)
        total = [0, 0]
        for pic, content, width, height, s, quality, turned, bgr in one_pass.cases():
            name = "%s__%s_q%d%s%s" % (pic, s, quality, "_turned" if turned else "", "_bgr" if bgr else "")
            seen = one_pass.reordered(one_pass.picture(content, width, height), turned, bgr)
            raw, out = os.path.join(tmp, "pixels.bin"), os.path.join(tmp, "out.jpg")
            seen.tofile(raw)
            subprocess.run([exes["file"], raw, out, str(width), str(height), str(quality),
                            str(one_pass.JPGE_SUBSAMPLING[one_pass.SAMPLINGS[s]])], check=True)
            data = open(out, "rb").read()
            os.remove(out)
            single = committed["file/" + name]
            assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9" and data != single.tobytes(), name
            arrays["file/" + name] = np.frombuffer(data, np.uint8)
            total[0] += len(data)
            total[1] += len(single)
            print("%-44s %7d bytes, %.2f of the one-pass file" % (name, len(data), len(data) / len(single)))
        # ---- the table tier ----
        cases = histograms()
        text = "".join("%d %s\n" % (len(counts), " ".join(str(int(c)) for c in counts)) for _, counts in cases)
        lines = subprocess.run([exes["table"]], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(lines) == len(cases)
        for (name, counts), line in zip(cases, lines):
            numbers = [int(x) for x in line.split()]
            bits, values = numbers[:16], numbers[16:]
            assert len(values) == sum(bits) == int((counts > 0).sum()), name
            arrays["table/%s/counts" % name] = counts
            arrays["table/%s/bits" % name] = np.array(bits, np.uint8)
            arrays["table/%s/values" % name] = np.array(values, np.uint8)
            print("%-24s %3d symbols, bits %s" % (name, len(values), bits))
    finally:
        shutil.rmtree(tmp)
    one_pass.save(OUT, arrays)
    size = os.path.getsize(OUT)
    print("%s: %d files (%d bytes, %.2f of the one-pass files'), %d tables, %d bytes" % (
        OUT, sum(k.startswith("file/") for k in arrays), total[0], total[0] / total[1], len(cases), size))
    assert size <= LIMIT, "the npz must stay within %d bytes" % LIMIT


if __name__ == "__main__":
    sys.exit(main())
