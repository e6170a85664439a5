/*
 * jpeg_two_pass_check.cpp - the optimised tables of sol-r_amd/csrc/jpeg_entropy.h as a program of its own, for the address
 * and undefined-behaviour sanitizers (tests/test_jpeg_two_pass.py builds it together with host/JpegWriter.cpp and runs it):
 * optimiseTable on the histograms of the table tier, and on every case's blocks the census, the four tables, the coder with
 * those tables as data in the decomposed order - bits, offsets and unstuffed words allocated at exactly the size the stage
 * says it needs, so that a write one element too far lands in a red zone - held to the one-pass writer in its optimised
 * mode (JpegWriter::encode between its header and its EOI) and to JpegWriter::scan.  Host code only.  Exit status 0 when
 * everything holds.
 *
 * The file: int32 number of tables, then per table int32 length, int32 number of values, the counts (length uint32), bits
 * (16 bytes), the values; int32 number of cases, then per case int32 lumaH, lumaV, width, height, int64 nbBlocks, the
 * blocks (nbBlocks * 64 int16), the expected census (536 uint32).
 */
#include <cstdio>
#include <cstring>
#include <memory>
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
            fprintf(stderr, "jpeg_two_pass_check: %s fails (line %d, item %d)\n", #condition, __LINE__, current);    \
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
        fprintf(stderr, "usage: jpeg_two_pass_check <cases file>\n");
        return 2;
    }
    /* ---- the table tier: counts and values in buffers of exactly their length ---- */
    int nbTables = 0;
    CHECK(get(f, &nbTables));
    for (current = 0; current < nbTables && !failures; ++current)
    {
        int length = 0, nbValues = 0;
        CHECK(get(f, &length) && get(f, &nbValues) && length >= 1 && length <= 256 && nbValues <= length);
        if (failures)
            break;
        std::vector<jpn::u32> counts((size_t)length);
        std::vector<jpn::u8> wantBits(16), wantValues((size_t)nbValues), bits(16), values((size_t)nbValues);
        CHECK(get(f, counts.data(), counts.size()) && get(f, wantBits.data(), 16) &&
              (nbValues == 0 || get(f, wantValues.data(), wantValues.size())));
        CHECK(jpn::optimiseTable(counts.data(), length, bits.data(), values.data()) == nbValues);
        CHECK(bits == wantBits && values == wantValues);
    }
    /* ---- the cases ---- */
    int nbCases = 0;
    CHECK(get(f, &nbCases));
    long nbBlocksTotal = 0;
    for (current = 0; current < nbCases && !failures; ++current)
    {
        int head[4];
        long long nbBlocks = 0;
        CHECK(get(f, head, 4) && get(f, &nbBlocks));
        if (failures)
            break;
        std::vector<short> blocks((size_t)nbBlocks * 64);
        std::vector<jpn::u32> wantCensus(jpn::CENSUS_COUNTERS);
        CHECK(get(f, blocks.data(), blocks.size()) && get(f, wantCensus.data(), wantCensus.size()));
        const int lumaH = head[0], lumaV = head[1], lumaBlocks = lumaH * lumaV;
        auto previousDc = [&](long index) {
            const long before = jpn::predecessor(index, lumaBlocks);
            return before < 0 ? 0 : (int)blocks[(size_t)before * 64];
        };

        /* census, on the heap so that its ends are red zones */
        std::unique_ptr<jpn::Census> census(new jpn::Census());
        bool inside = true;
        for (long i = 0; i < nbBlocks; ++i)
            inside &= jpn::blockCensus(blocks.data() + i * 64, previousDc(i), jpn::chromaOf(i, lumaBlocks), *census);
        CHECK(inside && memcmp(census.get(), wantCensus.data(), sizeof(jpn::Census)) == 0);

        /* tables: bits and values of exactly the lengths a table can need */
        std::unique_ptr<jpn::Huffman> huffman(new jpn::Huffman());
        std::unique_ptr<jpn::Tables> tables(new jpn::Tables());
        jpn::optimiseTables(*census, *huffman);
        jpn::tablesOf(*huffman, *tables);
        for (int slot = 0; slot < jpn::TABLE_SLOTS; ++slot)
        {
            int codes = 0, used = 0;
            for (int l = 0; l < 16; ++l)
                codes += huffman->bits[slot][l];
            for (int i = 0; i < jpn::slotLength(slot); ++i)
                used += jpn::slotCounts(*census, slot)[i] ? 1 : 0;
            CHECK(codes == used && huffman->nbValues[slot] == used);
            /* every used symbol has a code of 1 ... 16 bits that is not all ones, no other symbol has one */
            for (int i = 0; i < jpn::slotLength(slot); ++i)
            {
                const jpn::u32 entry = jpn::slotEntries(*tables, slot)[i];
                const int length = (int)(entry >> 16);
                if (jpn::slotCounts(*census, slot)[i])
                    CHECK(length >= 1 && length <= jpn::MAX_CODE_BITS && (entry & 0xffffu) != (1u << length) - 1u);
                else
                    CHECK(entry == 0);
            }
        }

        /* the coder with these tables, in the decomposed order */
        std::vector<jpn::u32> bits((size_t)nbBlocks);
        for (long i = 0; i < nbBlocks; ++i)
        {
            CHECK(jpn::blockBits(*tables, blocks.data() + i * 64, previousDc(i), jpn::chromaOf(i, lumaBlocks), &bits[(size_t)i]));
            CHECK(bits[(size_t)i] <= (jpn::u32)jpn::MAX_BLOCK_BITS_ANY_TABLE);
        }
        std::vector<jpn::u64> offsets((size_t)nbBlocks + 1);
        jpn::exclusiveSum(bits.data(), (long)nbBlocks, offsets.data());
        const jpn::u64 totalBits = offsets[(size_t)nbBlocks];
        std::vector<jpn::u32> words((size_t)jpn::streamWords(totalBits), 0u);
        for (long i = 0; i < nbBlocks; ++i)
            jpn::blockEmit(*tables, blocks.data() + i * 64, previousDc(i), jpn::chromaOf(i, lumaBlocks), offsets[(size_t)i],
                           words.data());
        if (const int tail = jpn::tailBits(totalBits))
        {
            jpn::WordWriter writer = {words.data(), totalBits};
            writer.put((1u << tail) - 1u, tail);
        }
        std::vector<unsigned char> unstuffed;
        for (jpn::u64 j = 0; j < jpn::streamBytes(totalBits); ++j)
            unstuffed.push_back((unsigned char)(words[(size_t)(j >> 2)] >> (24 - 8 * (int)(j & 3))));

        /* the writer: scan in its optimised mode, and the one-pass coder's file around the same segment */
        std::vector<unsigned char> scan;
        std::unique_ptr<jpn::Huffman> fromScan(new jpn::Huffman());
        CHECK(solr::JpegWriter::scan(lumaH, lumaV, blocks.data(), (long)nbBlocks, scan, fromScan.get()));
        for (int slot = 0; slot < jpn::TABLE_SLOTS; ++slot)
            CHECK(fromScan->nbValues[slot] == huffman->nbValues[slot] &&
                  memcmp(fromScan->bits[slot], huffman->bits[slot], 16) == 0 &&
                  memcmp(fromScan->values[slot], huffman->values[slot], (size_t)huffman->nbValues[slot]) == 0);
        std::vector<unsigned char> stuffed;
        for (unsigned char b : unstuffed)
        {
            stuffed.push_back(b);
            if (b == 0xFF)
                stuffed.push_back(0);
        }
        CHECK(stuffed == scan);
        unsigned short quant[2][64];
        jpe::quantTable(85, 0, quant[0]);
        jpe::quantTable(85, 1, quant[1]);
        const std::vector<unsigned char> header =
            solr::JpegWriter::header(head[2], head[3], lumaH, lumaV, quant, fromScan.get());
        const std::vector<unsigned char> file =
            solr::JpegWriter::encode(head[2], head[3], lumaH, lumaV, quant, blocks.data(), (long)nbBlocks, true);
        CHECK(file.size() == header.size() + scan.size() + 2);
        if (file.size() == header.size() + scan.size() + 2)
        {
            CHECK(memcmp(file.data(), header.data(), header.size()) == 0);
            CHECK(memcmp(file.data() + header.size(), scan.data(), scan.size()) == 0);
            CHECK(file[file.size() - 2] == 0xFF && file[file.size() - 1] == 0xD9);
        }
        /* the standard header is longer than any optimised one has to be: 4 x (2 + 2 + 1 + 16) + 2 x 12 + 2 x 162 */
        CHECK(header.size() <= solr::JpegWriter::header(head[2], head[3], lumaH, lumaV, quant).size() + 2 * (256 - 162));
        nbBlocksTotal += (long)nbBlocks;
    }
    /* outside the domain: refused, the output and the tables untouched */
    {
        std::vector<unsigned char> out(3, 0x5A);
        std::unique_ptr<jpn::Huffman> untouched(new jpn::Huffman());
        memset(untouched.get(), 0x5A, sizeof(jpn::Huffman));
        CHECK(!solr::JpegWriter::scan(1, 1, std::vector<short>(192, 3000).data(), 3, out, untouched.get()));
        CHECK(out.size() == 3 && out[0] == 0x5A && untouched->bits[0][0] == 0x5A && untouched->nbValues[3] == 0x5A5A5A5A);
    }
    fclose(f);
    if (!failures)
        printf("jpeg_two_pass_check: %d tables, %d cases, %ld blocks\n", nbTables, nbCases, nbBlocksTotal);
    return failures ? 1 : 0;
}
