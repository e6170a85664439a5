/*
 * jpeg_entropy_check.cpp - sol-r_amd/csrc/jpeg_entropy.h as a program of its own, for the address and undefined-behaviour
 * sanitizers (tests/test_jpeg_entropy.py builds it together with host/JpegWriter.cpp and runs it): the header's loops in the
 * decomposed order (JpegWriter::scan) on the cases it is handed in a file, every intermediate array - bits, offsets, the
 * unstuffed words, the chunk counts, the stuffed bytes - allocated at exactly the size the stage says it needs, so that a
 * write one element too far lands in a red zone.  Each result is compared with the bytes the file expects and with the
 * one-pass coder's (JpegWriter::encode between its header and its EOI).  Host code only.  Exit status 0 when everything
 * holds.
 *
 * The file: int32 number of cases, then per case int32 lumaH, lumaV, width, height, int64 nbBlocks, int64 nbBytes, the
 * blocks (nbBlocks * 64 int16), the expected entropy-coded segment (nbBytes bytes).
 */
#include <cstdio>
#include <cstring>
#include <vector>

#include "../sol-r_amd/csrc/jpeg_encode.h"
#include "../sol-r_amd/csrc/jpeg_entropy.h"
#include "../sol-r_amd/host/JpegWriter.h"

static int failures = 0;
#define CHECK(condition)                                                                                             \
    do                                                                                                               \
    {                                                                                                                \
        if (!(condition))                                                                                            \
        {                                                                                                            \
            fprintf(stderr, "jpeg_entropy_check: %s fails (line %d, case %d)\n", #condition, __LINE__, current);     \
            ++failures;                                                                                              \
        }                                                                                                            \
    } while (0)

template <class T>
static bool get(FILE *f, T *to, size_t n = 1)
{
    return fread(to, sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    int current = -1;
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f)
    {
        fprintf(stderr, "usage: jpeg_entropy_check <cases file>\n");
        return 2;
    }
    int nbCases = 0;
    CHECK(get(f, &nbCases));
    long nbBlocksTotal = 0;
    for (current = 0; current < nbCases && !failures; ++current)
    {
        int head[4];
        long long nbBlocks = 0, nbBytes = 0;
        CHECK(get(f, head, 4) && get(f, &nbBlocks) && get(f, &nbBytes));
        if (failures)
            break;
        std::vector<short> blocks((size_t)nbBlocks * 64);
        std::vector<unsigned char> expected((size_t)nbBytes);
        CHECK(get(f, blocks.data(), blocks.size()) && (nbBytes == 0 || get(f, expected.data(), expected.size())));
        const int lumaH = head[0], lumaV = head[1];

        /* the decomposed loops */
        std::vector<unsigned char> scan;
        CHECK(solr::JpegWriter::scan(lumaH, lumaV, blocks.data(), (long)nbBlocks, scan));
        CHECK(scan == expected);

        /* the one-pass coder: header + segment + EOI */
        unsigned short quant[2][64];
        jpe::quantTable(85, 0, quant[0]);
        jpe::quantTable(85, 1, quant[1]);
        const std::vector<unsigned char> header = solr::JpegWriter::header(head[2], head[3], lumaH, lumaV, quant);
        const std::vector<unsigned char> file =
            solr::JpegWriter::encode(head[2], head[3], lumaH, lumaV, quant, blocks.data(), (long)nbBlocks);
        CHECK(file.size() == header.size() + scan.size() + 2);
        CHECK(file.size() >= header.size() + 2 && memcmp(file.data(), header.data(), header.size()) == 0);
        CHECK(file.size() == header.size() + scan.size() + 2 &&
              memcmp(file.data() + header.size(), scan.data(), scan.size()) == 0);

        /* the bound of a block, and what is outside the domain, block by block */
        for (long long i = 0; i < nbBlocks; ++i)
        {
            jpn::u32 bits = 0;
            const long before = jpn::predecessor((long)i, lumaH * lumaV);
            CHECK(before < (long)i);
            CHECK(jpn::blockBits(&blocks[(size_t)i * 64], before < 0 ? 0 : blocks[(size_t)before * 64],
                                 jpn::chromaOf((long)i, lumaH * lumaV), &bits));
            CHECK(bits >= 4 && bits <= (jpn::u32)jpn::MAX_BLOCK_BITS);
        }
        nbBlocksTotal += (long)nbBlocks;
    }
    fclose(f);
    current = -1;

    /* outside the domain: reported, and the walk still takes exactly the bits it counts */
    {
        short block[64] = {0};
        jpn::u32 bits = 0;
        block[0] = 2048;
        CHECK(!jpn::blockBits(block, 0, 0, &bits));
        block[0] = 2047;
        CHECK(jpn::blockBits(block, 0, 0, &bits) && bits == 9 + 11 + 4);
        block[0] = 1024;
        CHECK(!jpn::blockBits(block, -1024, 1, &bits));
        block[0] = 0;
        block[63] = -1024;
        CHECK(!jpn::blockBits(block, 0, 0, &bits));
        std::vector<jpn::u32> words((size_t)jpn::streamWords(bits), 0u);
        jpn::blockEmit(block, 0, 0, 0, words.data());
        block[63] = -1023;
        CHECK(jpn::blockBits(block, 0, 1, &bits));
        std::vector<unsigned char> out(3, 0x5A);
        CHECK(!solr::JpegWriter::scan(1, 1, std::vector<short>(192, 3000).data(), 3, out));
        CHECK(out.size() == 3 && out[0] == 0x5A && out[2] == 0x5A);
    }

    /* a word of 0xFF bytes into a buffer of exactly eight */
    {
        std::vector<unsigned char> out(8, 1);
        CHECK(jpn::countFF(0xFFFFFFFFu, 4) == 4 && jpn::stuffWord(0xFFFFFFFFu, 4, out.data()) == 8);
        CHECK(out[0] == 0xFF && out[1] == 0 && out[6] == 0xFF && out[7] == 0);
        std::vector<unsigned char> one(2, 1);
        CHECK(jpn::countFF(0xFF000000u, 1) == 1 && jpn::stuffWord(0xFFFFFFFFu, 1, one.data()) == 2);
        CHECK(jpn::bytesOfWord(0, 0) == 0 && jpn::bytesOfWord(1, 5) == 1 && jpn::bytesOfWord(1, 8) == 4 &&
              jpn::bytesOfWord(2, 8) == 0);
    }

    /* offsets beyond 2^32 */
    {
        std::vector<jpn::u32> lengths(4, 0xC0000000u);
        std::vector<jpn::u64> offsets(5);
        jpn::exclusiveSum(lengths.data(), 4, offsets.data());
        CHECK(offsets[0] == 0 && offsets[2] == 0x180000000ull && offsets[4] == 0x300000000ull);
    }

    if (!failures)
        printf("%d cases, %ld blocks: the decomposed loops give the one-pass coder's bytes\n", nbCases, nbBlocksTotal);
    return failures ? 1 : 0;
}
