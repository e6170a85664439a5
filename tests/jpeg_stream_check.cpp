/*
 * jpeg_stream_check.cpp - the resident entropy pipeline of sol-r_amd/csrc/jpeg_entropy.h (planScan, planBytesOfWord,
 * chunkCountFF, chunkStuff: what k_jpegPlan, k_jpegCountFFResident and k_jpegStuffResident of csrc/solr_jpeg_entropy.hip
 * run a lane per word) as a program of its own, for the address and undefined-behaviour sanitizers
 * (tests/test_jpeg_stream.py builds and runs it).  The cases of the file go, in the file's order and then once more,
 * through ONE set of buffers that is never zeroed in between - sized once for the largest case by the bounds the slots
 * are sized by (maxStreamChunks, maxStuffedBytes), exactly, so that a write one element too far lands in a red zone - with
 * the loops over the bound and the extent from the plan.  After every use the stream must be all zeros again (the clearing
 * behind a use that the next emit relies on), the segment must be the file's, and nothing behind it may be written.  A
 * flagged plan must leave everything untouched.  Host code only.  Exit status 0 when everything holds.
 *
 * The file: as jpeg_entropy_check.cpp's.
 */
#include <cstdio>
#include <cstring>
#include <vector>

#include "../sol-r_amd/csrc/jpeg_encode.h"
#include "../sol-r_amd/csrc/jpeg_entropy.h"

static int failures = 0;
#define CHECK(condition)                                                                                             \
    do                                                                                                               \
    {                                                                                                                \
        if (!(condition))                                                                                            \
        {                                                                                                            \
            fprintf(stderr, "jpeg_stream_check: %s fails (line %d, use %d)\n", #condition, __LINE__, current);       \
            ++failures;                                                                                              \
        }                                                                                                            \
    } while (0)

template <class T>
static bool get(FILE *f, T *to, size_t n = 1)
{
    return fread(to, sizeof(T), n, f) == n;
}

struct Case
{
    int lumaBlocks;
    long nbBlocks;
    std::vector<short> blocks;
    std::vector<unsigned char> expected;
};

int main(int argc, char **argv)
{
    int current = -1;
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f)
    {
        fprintf(stderr, "usage: jpeg_stream_check <cases file>\n");
        return 2;
    }
    int nbCases = 0;
    CHECK(get(f, &nbCases));
    std::vector<Case> cases;
    long largest = 0;
    for (int i = 0; i < nbCases && !failures; ++i)
    {
        int head[4];
        long long nbBlocks = 0, nbBytes = 0;
        CHECK(get(f, head, 4) && get(f, &nbBlocks) && get(f, &nbBytes));
        if (failures)
            break;
        Case c;
        c.lumaBlocks = head[0] * head[1];
        c.nbBlocks = (long)nbBlocks;
        c.blocks.resize((size_t)nbBlocks * 64);
        c.expected.resize((size_t)nbBytes);
        CHECK(get(f, c.blocks.data(), c.blocks.size()) && (nbBytes == 0 || get(f, c.expected.data(), c.expected.size())));
        largest = c.nbBlocks > largest ? c.nbBlocks : largest;
        cases.push_back(std::move(c));
    }
    fclose(f);
    if (failures || cases.empty())
        return 1;

    /* the slot: cut once, for the largest case */
    const jpn::u64 slotChunks = jpn::maxStreamChunks(largest);
    std::vector<jpn::u32> stream((size_t)slotChunks * (jpn::STUFF_CHUNK_BYTES / 4), 0u);
    std::vector<jpn::u64> counts((size_t)slotChunks + 1), before((size_t)slotChunks + 1);
    std::vector<unsigned char> out((size_t)jpn::maxStuffedBytes(largest));
    std::vector<jpn::u32> bits((size_t)largest);
    std::vector<jpn::u64> offsets((size_t)largest + 1);
    long uses = 0;
    for (int round = 0; round < 2; ++round)
        for (size_t which = 0; which < cases.size(); ++which)
        {
            current = (int)(round * cases.size() + which);
            const Case &c = cases[which];
            const long n = c.nbBlocks;
            const jpn::u64 boundChunks = jpn::maxStreamChunks(n); /* what the host knows at submission */
            CHECK(boundChunks <= slotChunks && jpn::maxStuffedBytes(n) <= out.size());
            bool inside = true;
            for (long i = 0; i < n; ++i)
            {
                const long prior = jpn::predecessor(i, c.lumaBlocks);
                inside &= jpn::blockBits(&c.blocks[(size_t)i * 64], prior < 0 ? 0 : c.blocks[(size_t)prior * 64],
                                         jpn::chromaOf(i, c.lumaBlocks), &bits[(size_t)i]);
            }
            CHECK(inside);
            jpn::exclusiveSum(bits.data(), n, offsets.data());
            const jpn::ScanPlan plan = jpn::planScan(offsets[(size_t)n], 0);
            CHECK(plan.totalBits <= jpn::maxStreamBits(n) && plan.unstuffedBytes == jpn::streamBytes(plan.totalBits));
            CHECK(plan.streamWords == jpn::streamWords(plan.totalBits + (jpn::u64)jpn::tailBits(plan.totalBits)));
            CHECK(plan.nbChunks <= boundChunks && plan.nbChunks * jpn::STUFF_CHUNK_BYTES >= plan.unstuffedBytes);
            CHECK(plan.nbChunks == 0 || (plan.nbChunks - 1) * jpn::STUFF_CHUNK_BYTES < plan.unstuffedBytes);
            /* emit into whatever the use before left: it must have left zeros */
            for (long i = 0; i < n; ++i)
            {
                const long prior = jpn::predecessor(i, c.lumaBlocks);
                jpn::blockEmit(&c.blocks[(size_t)i * 64], prior < 0 ? 0 : c.blocks[(size_t)prior * 64],
                               jpn::chromaOf(i, c.lumaBlocks), offsets[(size_t)i], stream.data());
            }
            if (const int tail = jpn::tailBits(plan.totalBits))
            {
                jpn::WordWriter writer = {stream.data(), plan.totalBits};
                writer.put((1u << tail) - 1u, tail);
            }
            /* count and stuff over the bound, the extent from the plan */
            for (jpn::u64 chunk = 0; chunk < boundChunks; ++chunk)
            {
                counts[(size_t)chunk] = jpn::chunkCountFF(stream.data(), plan, chunk);
                CHECK(chunk < plan.nbChunks || counts[(size_t)chunk] == 0);
            }
            counts[(size_t)boundChunks] = 0;
            jpn::u64 sum = 0;
            for (jpn::u64 chunk = 0; chunk <= boundChunks; ++chunk)
            {
                before[(size_t)chunk] = sum;
                sum += counts[(size_t)chunk];
            }
            const jpn::u64 stuffed = plan.unstuffedBytes + before[(size_t)boundChunks];
            CHECK(stuffed <= jpn::maxStuffedBytes(n));
            memset(out.data(), 0x5A, out.size());
            for (jpn::u64 chunk = 0; chunk < boundChunks; ++chunk)
                jpn::chunkStuff(stream.data(), plan, chunk, before[(size_t)chunk], out.data(), true);
            CHECK(stuffed == c.expected.size() && memcmp(out.data(), c.expected.data(), c.expected.size()) == 0);
            bool untouched = true;
            for (size_t i = (size_t)stuffed; i < out.size(); ++i)
                untouched &= out[i] == 0x5A;
            CHECK(untouched);
            bool zero = true;
            for (const jpn::u32 word : stream)
                zero &= word == 0u;
            CHECK(zero);
            ++uses;
        }
    current = -1;

    /* a flagged plan: no extent, nothing read, nothing written - whatever the total says */
    {
        const jpn::ScanPlan plan = jpn::planScan(123456, 1);
        CHECK(plan.flag == 1 && plan.totalBits == 0 && plan.unstuffedBytes == 0 && plan.streamWords == 0 && plan.nbChunks == 0);
        std::vector<jpn::u32> words(jpn::STUFF_CHUNK_BYTES / 4, 0xFFFFFFFFu);
        std::vector<unsigned char> none(1, 0x5A);
        CHECK(jpn::chunkCountFF(words.data(), plan, 0) == 0 && jpn::planBytesOfWord(plan, 0) == 0);
        jpn::chunkStuff(words.data(), plan, 0, 0, none.data(), true);
        CHECK(none[0] == 0x5A && words[0] == 0xFFFFFFFFu);
    }
    /* the extent ends inside a word and inside a chunk; the chunk count around a chunk's bytes */
    {
        const jpn::ScanPlan plan = jpn::planScan(8 * 257 - 3, 0);
        CHECK(plan.unstuffedBytes == 257 && plan.nbChunks == 2 && plan.streamWords == 65);
        CHECK(jpn::planBytesOfWord(plan, 63) == 4 && jpn::planBytesOfWord(plan, 64) == 1 && jpn::planBytesOfWord(plan, 65) == 0 &&
              jpn::planBytesOfWord(plan, 128) == 0);
        CHECK(jpn::chunksOf(0) == 0 && jpn::chunksOf(255) == 1 && jpn::chunksOf(256) == 1 && jpn::chunksOf(257) == 2);
    }

    if (!failures)
        printf("%ld uses of one slot: every segment the expected one, the stream zero behind each\n", uses);
    return failures ? 1 : 0;
}
