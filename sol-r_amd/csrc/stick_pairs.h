/*
 * stick_pairs.h - which atoms of a molecule are joined by a stick: the pair search of the reference's PDB reader
 * (solr/io/PDBReader.cpp:616-660) as a rule over an array of atoms.  IEEE binary32 in source order, written once for both
 * sides: the host-only engine runs it in loops (GPUKernel::stickPairs), the HIP engine in kernels (csrc/solr_sticks.hip).
 * Both are compiled without contraction and with a correctly rounded square root (the Makefile's NUMERIC flags), so both
 * give the same pairs.
 *
 * The rule.  Atoms have ranks 0 ... n - 1 (the reader's: the order of its map).  Atom j is a partner of atom i when
 *   i != j                                   by rank, never by position: two atoms at one place are partners
 *   backbone[i] == backbone[j]               as truth values
 *   bonded(i, j, reach[backbone[i]])         sqrtf((ax*ax + ay*ay) + az*az) < reach, a = i - j component by component
 * A coordinate that is not finite makes the sum infinite or not a number and the comparison false: no partner.
 *
 * The root is not taken in the loops.  sqrtf is correctly rounded and therefore monotone over the sums (which are never
 * negative), so there is one binary32 number T = squaredReach(reach) with  sqrtf(s) < reach  <=>  s < T  for every s, the
 * infinities and NaN included (both sides false).  squaredReach finds it on the host by stepping floats about
 * reach * reach; within() compares the sum with it.  tests/test_stick_pairs.py steps the floats about T for both reaches.
 *
 * The pairs as a list (CSR): start[i] ... start[i + 1] are atom i's places in partner[], its partners' ranks ascending;
 * start has n + 1 entries of 64 bits, start[n] the number of pairs.
 */
#pragma once

#include <cmath>

#include "../../include/solr_types.h"

#if defined(__HIPCC__)
#define STICKS_HD __host__ __device__
#else
#define STICKS_HD
#endif

namespace sticks
{
struct Point
{
    float x, y, z;
};

/* ---- the rule (PDBReader.cpp:640-646) ------------------------------------------------------------------------------ */
STICKS_HD inline float squaredDistance(const Point &a, const Point &b)
{
    const float ax = a.x - b.x, ay = a.y - b.y, az = a.z - b.z;
    return (ax * ax + ay * ay) + az * az;
}

STICKS_HD inline bool bonded(const Point &a, const Point &b, float reach)
{
    return sqrtf(squaredDistance(a, b)) < reach;
}

/* the same verdict from the threshold on the sum: limit = squaredReach(reach) */
STICKS_HD inline bool within(const Point &a, const Point &b, float limit)
{
    return squaredDistance(a, b) < limit;
}

/* the smallest binary32 number whose root is not below `reach` (finite, > 0): every sum below it bonds, no other does */
inline float squaredReach(float reach)
{
    float t = reach * reach;
    if (!(t < INFINITY))
        t = 3.4028234663852886e38f; /* the product overflowed: start at the largest finite sum */
    while (t > 0.f && !(sqrtf(nextafterf(t, 0.f)) < reach))
        t = nextafterf(t, 0.f);
    while (t < INFINITY && sqrtf(t) < reach)
        t = nextafterf(t, INFINITY);
    return t;
}

inline bool isFinite(float v) { return v - v == 0.f; }

/* why a search is refused, nullptr when it is not */
inline const char *refusal(const float *atoms, const unsigned char *backbone, int n, float reachPlain, float reachBackbone,
                           const long long *start, const int *partners, long long capacity)
{
    if (!atoms || !backbone || !start)
        return "null atoms, backbone or start";
    if (n < 0 || n > NB_MAX_PRIMITIVES)
        return "n must be 0 ... NB_MAX_PRIMITIVES";
    if (!isFinite(reachPlain) || !isFinite(reachBackbone) || !(reachPlain > 0.f) || !(reachBackbone > 0.f))
        return "a reach must be finite and positive";
    if (capacity < 0)
        return "negative capacity";
    if (!partners && capacity != 0)
        return "null partners with a capacity";
    return nullptr;
}

/* ---- the loops of the host-only engine ----------------------------------------------------------------------------- */
/* atoms: n records of x, y, z, spare; limit[f]: squaredReach of the reach of flag f.  start is written whole, every pair
 * handed to sink(rank of the pair in the list, partner) in the list's order; the number of pairs */
template <class Sink>
inline long long walk(const float *atoms, const unsigned char *backbone, int n, const float limit[2], long long *start,
                      Sink sink)
{
    long long total = 0;
    for (int i = 0; i < n; ++i)
    {
        start[i] = total;
        const Point a = {atoms[4 * (size_t)i], atoms[4 * (size_t)i + 1], atoms[4 * (size_t)i + 2]};
        const bool flag = backbone[i] != 0;
        const float mine = limit[flag ? 1 : 0];
        for (int j = 0; j < n; ++j)
        {
            const Point b = {atoms[4 * (size_t)j], atoms[4 * (size_t)j + 1], atoms[4 * (size_t)j + 2]};
            if (j != i && (backbone[j] != 0) == flag && within(a, b, mine))
                sink(total++, j);
        }
    }
    start[n] = total;
    return total;
}

/* the list into a buffer of `capacity` partners: the number of pairs there are, the first min(total, capacity) written */
inline long long pairsLoop(const float *atoms, const unsigned char *backbone, int n, float reachPlain, float reachBackbone,
                           long long *start, int *partners, long long capacity)
{
    const float limit[2] = {squaredReach(reachPlain), squaredReach(reachBackbone)};
    return walk(atoms, backbone, n, limit, start, [&](long long at, int partner) {
        if (at < capacity)
            partners[at] = partner;
    });
}
}
