/*
 * iso_surface_check.cpp - sol-r_amd/csrc/iso_surface.h as a program of its own, for the address and undefined-behaviour
 * sanitizers (tests/test_iso_surface.py builds and runs it): the generator of the case table, the field loop, and the
 * surface loop on the all-cases grid - N = 15, the 512 cubes at even coordinates with disjoint corners taking each of the
 * 256 cases twice - into buffers of exactly the size asked for.  Host code only.  Exit status 0 when everything holds.
 */
#include <cstdio>
#include <cstring>
#include <vector>

#include "../sol-r_amd/csrc/iso_surface.h"

static int failures = 0;
#define CHECK(condition)                                                                                             \
    do                                                                                                               \
    {                                                                                                                \
        if (!(condition))                                                                                            \
        {                                                                                                            \
            fprintf(stderr, "iso_surface_check: %s fails (line %d)\n", #condition, __LINE__);                        \
            ++failures;                                                                                              \
        }                                                                                                            \
    } while (0)

static unsigned lcgState = 12345u;
static float uniform(float lo, float hi)
{
    lcgState = lcgState * 1664525u + 1013904223u;
    return lo + (hi - lo) * (float)((lcgState >> 8) % 100000u) / 100000.f;
}

int main()
{
    /* ---- the table ---- */
    iso::CaseTable table;
    CHECK(iso::buildCaseTable(table));
    CHECK(iso::caseTable() != nullptr);
    int total = 0, most = 0, histogram[iso::MAX_CASE_TRIANGLES + 1] = {0, 0, 0, 0, 0, 0};
    for (int c = 0; c < 256; ++c)
    {
        const int count = table.count[c];
        CHECK(count <= iso::MAX_CASE_TRIANGLES);
        if (count > iso::MAX_CASE_TRIANGLES)
            continue;
        total += count;
        most = count > most ? count : most;
        ++histogram[count];
        bool used[12] = {false};
        for (int t = 0; t < count; ++t)
        {
            const unsigned char *e = &table.edges[c][3 * t];
            CHECK(e[0] < 12 && e[1] < 12 && e[2] < 12);
            CHECK(e[0] != e[1] && e[1] != e[2] && e[0] != e[2]);
            for (int v = 0; v < 3; ++v)
                if (e[v] < 12)
                    used[e[v]] = true;
        }
        for (int e = 0; e < 12; ++e)
            CHECK(used[e] == (((c >> iso::edgeFirst(e)) & 1) != ((c >> iso::edgeSecond(e)) & 1)));
    }
    CHECK(total == 820 && most == 5);
    CHECK(histogram[0] == 2 && histogram[1] == 16 && histogram[2] == 50 && histogram[3] == 80 && histogram[4] == 76 &&
          histogram[5] == 32);
    printf("%d triangles in the table\n", total);

    /* ---- the field loop, into a buffer of exactly (N+1)^3 records ---- */
    {
        SolrIsoGrid grid = {5, {10.f, 12.f, 14.f}, 1.f, {1.f, -2.f, 3.5f}, {2.f, 3.f, 0.5f}, 40.f};
        const float balls[3][4] = {{0.3f, -0.4f, 0.2f, 30.f}, {5.f, -6.f, 7.f, 25.f} /* on a vertex */, {-2.f, 1.f, 0.f, 9.f}};
        CHECK(iso::refusal(&grid, 3, 0) == nullptr);
        std::vector<float> field((size_t)6 * 6 * 6 * 4);
        iso::fieldLoop(grid, &balls[0][0], 3, field.data());
        const int count = iso::surfaceLoop(grid, table, field.data(), nullptr, 0);
        CHECK(count > 0);
        std::vector<SolrIsoTriangle> triangles((size_t)count);
        CHECK(iso::surfaceLoop(grid, table, field.data(), triangles.data(), count) == count);
        iso::fieldLoop(grid, &balls[0][0], 0, field.data());
        CHECK(iso::surfaceLoop(grid, table, field.data(), nullptr, 0) == 0);
        grid.gridSize = 0;
        CHECK(iso::refusal(&grid, 3, 0) != nullptr);
    }

    /* ---- the all-cases grid ---- */
    {
        const int n = 15, side = n + 1;
        const SolrIsoGrid grid = {n, {30.f, 30.f, 30.f}, 1.f, {0.f, 0.f, -2500.f}, {40.f, 40.f, 40.f}, 40.f};
        std::vector<float> field((size_t)side * side * side * 4);
        for (float &f : field)
            f = uniform(-1.f, 1.f);
        int number = 0, wanted = 0;
        for (int i = 0; i < side; i += 2)
            for (int j = 0; j < side; j += 2)
                for (int k = 0; k < side; k += 2, ++number)
                {
                    const int c = number % 256;
                    for (int corner = 0; corner < 8; ++corner)
                        field[4 * iso::vertexIndex(n, i + iso::cornerI(corner), j + iso::cornerJ(corner),
                                                   k + iso::cornerK(corner)) +
                              3] = ((c >> corner) & 1) ? uniform(0.05f, 0.95f) : uniform(1.05f, 3.f);
                    CHECK(iso::cubeCase(field.data(), n, i, j, k, 1.f) == c);
                    wanted += table.count[c];
                }
        CHECK(number == 512 && wanted == 2 * 820);
        const int count = iso::surfaceLoop(grid, table, field.data(), nullptr, 0);
        CHECK(count >= wanted);
        std::vector<SolrIsoTriangle> triangles((size_t)count);
        CHECK(iso::surfaceLoop(grid, table, field.data(), triangles.data(), count) == count);
        int previous = -1;
        for (const SolrIsoTriangle &t : triangles)
        {
            CHECK(t.cube >= previous && t.cube < n * n * n);
            previous = t.cube;
            for (int v = 0; v < 3; ++v)
                CHECK(t.edge[v] >= 0 && t.edge[v] < 3 * side * side * side);
        }
        /* a capacity below the count: only that many are written */
        std::vector<SolrIsoTriangle> some((size_t)count / 2);
        CHECK(iso::surfaceLoop(grid, table, field.data(), some.data(), count / 2) == count);
        CHECK(memcmp(some.data(), triangles.data(), some.size() * sizeof(SolrIsoTriangle)) == 0);
        printf("%d triangles on the all-cases grid\n", count);
    }
    return failures == 0 ? 0 : 1;
}
