/*
 * stick_pairs_check.cpp - sol-r_amd/csrc/stick_pairs.h as a program of its own, for the address and undefined-behaviour
 * sanitizers (tests/test_stick_pairs.py builds and runs it): the threshold against the root, and the loops and the list
 * builder on the sizes at the wave and tile edges, the list whole and cut short by its capacity.  No device code, nothing
 * of the engine: what is checked here is the header.
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../sol-r_amd/csrc/stick_pairs.h"

#define CHECK(condition)                                                                                             \
    do                                                                                                               \
    {                                                                                                                \
        if (!(condition))                                                                                            \
        {                                                                                                            \
            fprintf(stderr, "stick_pairs_check: %s fails (line %d)\n", #condition, __LINE__);                        \
            exit(1);                                                                                                 \
        }                                                                                                            \
    } while (0)

static unsigned gState = 12345u;
static float uniform(float side)
{
    gState = gState * 1664525u + 1013904223u;
    return ((float)(gState >> 8) / 16777216.f - 0.5f) * side;
}

int main()
{
    /* the threshold: the verdict of the root for the floats about it */
    const float reaches[] = {1.7f, 3.4f, 1.f, 1e-20f, 3e19f};
    for (float reach : reaches)
    {
        const float limit = sticks::squaredReach(reach);
        float s = limit;
        for (int k = 0; k < 1000; ++k)
            s = nextafterf(s, 0.f);
        for (int k = 0; k < 2000; ++k, s = nextafterf(s, INFINITY))
            CHECK((sqrtf(s) < reach) == (s < limit));
        CHECK(!(sqrtf(INFINITY) < reach) && !(INFINITY < limit) && !(NAN < limit));
    }
    CHECK(sticks::bonded({0.f, 0.f, 0.f}, {nextafterf(1.7f, 0.f), 0.f, 0.f}, 1.7f));
    CHECK(!sticks::bonded({0.f, 0.f, 0.f}, {1.7f, 0.f, 0.f}, 1.7f));

    const int sizes[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 4099};
    long long pairs = 0;
    for (int n : sizes)
    {
        /* exactly n records: a read past the last one is the sanitizer's to find */
        std::vector<float> atoms((size_t)n * 4);
        std::vector<unsigned char> backbone((size_t)n);
        const float side = 2.f * cbrtf((float)(n > 0 ? n : 1));
        for (int i = 0; i < n; ++i)
        {
            for (int c = 0; c < 3; ++c)
                atoms[(size_t)i * 4 + c] = uniform(side);
            atoms[(size_t)i * 4 + 3] = NAN;
            backbone[(size_t)i] = (unsigned char)((gState >> 20) & 1 ? 0x80 : 0);
        }
        if (n > 2)
            atoms[4] = NAN, atoms[9] = INFINITY;
        std::vector<long long> start((size_t)n + 1, -1), again((size_t)n + 1, -1);
        const long long total = sticks::pairsLoop(atoms.data(), backbone.data(), n, 1.7f, 3.4f, start.data(), nullptr, 0);
        CHECK(total >= 0 && start[0] == 0 && start[(size_t)n] == total);
        std::vector<int> partners((size_t)total);
        CHECK(sticks::pairsLoop(atoms.data(), backbone.data(), n, 1.7f, 3.4f, again.data(), partners.data(), total) == total);
        CHECK(again == start);
        for (int i = 0; i < n; ++i)
        {
            CHECK(start[(size_t)i] <= start[(size_t)i + 1]);
            for (long long at = start[(size_t)i]; at < start[(size_t)i + 1]; ++at)
            {
                const int j = partners[(size_t)at];
                CHECK(j >= 0 && j < n && j != i && (backbone[(size_t)j] != 0) == (backbone[(size_t)i] != 0));
                CHECK(at == start[(size_t)i] || partners[(size_t)at - 1] < j);
                const sticks::Point a = {atoms[(size_t)i * 4], atoms[(size_t)i * 4 + 1], atoms[(size_t)i * 4 + 2]};
                const sticks::Point b = {atoms[(size_t)j * 4], atoms[(size_t)j * 4 + 1], atoms[(size_t)j * 4 + 2]};
                CHECK(sticks::bonded(a, b, backbone[(size_t)i] ? 3.4f : 1.7f));
                bool back = false; /* i is j's partner too */
                for (long long other = start[(size_t)j]; other < start[(size_t)j + 1]; ++other)
                    back = back || partners[(size_t)other] == i;
                CHECK(back);
            }
        }
        if (n > 2)
            CHECK(start[1] == start[2] && start[2] == start[3]); /* the atoms that are not finite have no partner */
        /* cut short: exactly that many are written */
        if (total > 0)
        {
            std::vector<int> some((size_t)total - 1);
            CHECK(sticks::pairsLoop(atoms.data(), backbone.data(), n, 1.7f, 3.4f, again.data(), some.data(), total - 1) ==
                  total);
            for (size_t at = 0; at < some.size(); ++at)
                CHECK(some[at] == partners[at]);
        }
        pairs += total;
    }
    CHECK(pairs > 4099);
    CHECK(sticks::refusal(nullptr, nullptr, 0, 1.7f, 3.4f, nullptr, nullptr, 0) != nullptr);
    printf("12 sizes, the lists whole and cut short: %lld pairs\n", pairs);
    return 0;
}
