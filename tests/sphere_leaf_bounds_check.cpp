/*
 * sphere_leaf_bounds_check.cpp - sol-r_amd/csrc/build_bounds.h leafBuildBounds on the CPU, as solr_arena.hip k_tightenLeaves
 * calls it: for tests/test_sphere_leaves_model.py, which compares what it writes with the numpy model of
 * tests/sphere_leaves_model.py bit for bit.  A program of its own, compiled under the address and undefined-behaviour
 * sanitizers:
 *   g++ -std=c++17 -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include -o check tests/sphere_leaf_bounds_check.cpp
 *   check IN OUT
 * IN:  int32 nodes, prims, byKind; float32 margin, reach; nodes x 8 float32 node rows; nodes int32 start indices;
 *      prims x 32 float32 primitive records (scene_layout.h).
 * OUT: nodes x 8 float32 - the leaves of the thin copy (inner nodes copied); then nodes int32 - leafBuildBounds' answer.
 */
#include <cstdio>
#include <vector>

#include "../sol-r_amd/csrc/build_bounds.h"

using namespace solreng;

int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in)
        return 2;
    int head[3];
    float knobs[2];
    if (fread(head, 4, 3, in) != 3 || fread(knobs, 4, 2, in) != 2 || head[0] < 0 || head[1] < 0)
        return 2;
    const size_t nodes = (size_t)head[0], nbPrims = (size_t)head[1];
    std::vector<float4> rows(2 * nodes), prims(8 * nbPrims);
    std::vector<int> start(nodes), answer(nodes, 0);
    if (fread(rows.data(), 16, 2 * nodes, in) != 2 * nodes || fread(start.data(), 4, nodes, in) != nodes ||
        fread(prims.data(), 16, 8 * nbPrims, in) != 8 * nbPrims)
        return 2;
    fclose(in);
    for (size_t i = 0; i < nodes; ++i)
    {
        float4 &row0 = rows[2 * i], &row1 = rows[2 * i + 1];
        int count;
        memcpy(&count, &row1.z, 4);
        if (count <= 0)
            continue;
        if (start[i] < 0 || (size_t)start[i] + (size_t)count > nbPrims)
            return 3; /* (a leaf that names primitives the file does not hold) */
        float lo[3], hi[3];
        if (leafBuildBounds(row0, row1, prims.data(), start[i], count, knobs[0], lo, hi, head[2] != 0, knobs[1]))
        {
            answer[i] = 1;
            row0 = make_float4(lo[0], lo[1], lo[2], hi[2]);
            row1 = make_float4(hi[0], hi[1], row1.z, row1.w);
        }
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out || fwrite(rows.data(), 16, 2 * nodes, out) != 2 * nodes || fwrite(answer.data(), 4, nodes, out) != nodes)
        return 2;
    fclose(out);
    return 0;
}
