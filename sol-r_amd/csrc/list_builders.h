/*
 * list_builders.h - the host builders of the engine's node lists (list_builders.cpp): plain C++17 over std::vector, no
 * engine state, no environment, no HIP call.  The engine's scene units (solr_uploads.hip,
 * solr_arena.hip, solr_rotation.hip) call them for the walk-order list of every upload, for the order-free lists where the
 * device builders (solr_lists.hip) are switched off or decline, and for the refit plan; they
 * are the reference the device builders are held to (tests/test_lists_gpu.py, tests/test_list_builders_device_gpu.py), and tests/list_builders_check.cpp runs
 * them on their own.
 * A node list: two float4 rows per node, { min.xyz, max.z } { max.xy, nbPrimitives, skip } (scene_layout.h); `start`: the
 * first primitive of every node; `origin`: the node of the reference's list every node is, -1 for a node made here.
 */
#ifndef SOLR_LIST_BUILDERS_H
#define SOLR_LIST_BUILDERS_H

#include <hip/hip_vector_types.h>

#include <cstring>
#include <functional>
#include <vector>

#include "../../include/solr_types.h"
#include "build_bounds.h"

namespace solreng
{
inline int bitsi(float v)
{
    int i;
    memcpy(&i, &v, sizeof(i));
    return i;
}
inline float bitsf(int v)
{
    float f;
    memcpy(&f, &v, 4);
    return f;
}

/* the facts of a primitive record (scene_layout.h, device code) that listEnclosesOnHost reads; solr_uploads.hip holds them
 * to that header */
enum ListBuilderPrimRow
{
    LB_ROW_P0_TYPE = 0,
    LB_ROW_SIZE_MAT = 1,
    LB_ROW_P1_INDEX = 2,
    LB_ROW_P2 = 3,
    LB_PRIM_ROWS = 8,
    LB_PRIM_TYPE_MASK = 0xff
};

/* what SOLR_HIP_PRUNE, SOLR_HIP_GROUP_FLAT and SOLR_HIP_GROUP_LEVELS set (tools/README.md); the defaults are the engine's */
struct ListKnobs
{
    double pruneThreshold = 1.0; /* tests an inner node has to save to stay; <= 0: nothing is pruned */
    int groupFlat = 4;           /* runs of siblings up to this length stay as they are */
    int groupLevels = -1;        /* rounds of binary splits per group, 1 ... 4; < 0: by the length of the list */
};

/* pruneInnerNodes' decisions made elsewhere (the device, solr_lists.hip): keep[i] = 0 for the inner nodes left out.
 * Returns how many, or -1 to leave them to the host. */
typedef std::function<int(const float4 *rows, int n, double threshold, std::vector<char> &keep)> PruneDecider;

int validateNesting(const BoundingBox *boxes, int n);
int collapseChains(const std::vector<float4> &rows, const std::vector<int> &start, bool nested, std::vector<float4> &outRows,
                   std::vector<int> &outStart, std::vector<int> &outOrigin, int *orderedExact, int *orderedWalk);
int pruneInnerNodes(std::vector<float4> &rows, std::vector<int> &start, std::vector<int> &origin, int *nbPruned, double threshold,
                    const PruneDecider &decider = nullptr);
int groupSiblings(std::vector<float4> &rows, std::vector<int> &start, std::vector<int> &origin, const ListKnobs &knobs);
int buildWalkOrderList(std::vector<float4> &rows, std::vector<int> &start, std::vector<int> &origin, const ListKnobs &knobs,
                       const PruneDecider &decider, int *prunedBefore, int *prunedAfter,
                       const std::function<void(const char *)> &mark = nullptr);
int buildFreeOrderLists(const std::vector<float4> &rows, const std::vector<int> &start, const std::vector<int> &origin,
                        std::vector<float4> &outRows, std::vector<int> &outStart, std::vector<int> &outOrigin, int *nbPruned,
                        double threshold, const PruneDecider &decider = nullptr, const BuildBounds &build = BuildBounds());
bool listEnclosesOnHost(const std::vector<float4> &rows, const std::vector<int> &start, const std::vector<float4> &prims);
void planRefit(const std::vector<float4> &exact, const std::vector<float4> &walk, const std::vector<int> &origin,
               const std::vector<float4> &free, const std::vector<int> &freeOrigin, std::vector<int> &plan,
               std::vector<int> &exactLevels, std::vector<int> &walkLevels, std::vector<int> &freeLevels);
} // namespace solreng

#endif
