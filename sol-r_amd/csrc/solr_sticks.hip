/*
 * solr_sticks.hip - which atoms of a molecule are joined by a stick, found on the device (include/solr_hip.h:
 * solr_hip_stick_pairs).  The rule is stick_pairs.h - the pair search of the reference's PDB reader, binary32 in source
 * order - and this file is only its lane mapping; the host-only engine runs the same header in loops
 * (host/GPUKernel.cpp) and gives the same pairs.  gfx950 only.
 *
 *   layout         a lane per atom i, its record in registers.  The atoms j come past in tiles of 256 records (4 KiB of
 *                  LDS: x, y, z and the flag in the fourth word), loaded by the group's 256 lanes, one record each.  In
 *                  the walk every lane reads the same tile address in the same trip: a broadcast, no bank conflict
 *   k_stickCount   the number of partners of each atom, as 64 bits for the scan
 *   (scan)         hipcub::DeviceScan::ExclusiveSum over n + 1 counts (the last one 0): start[], whole.  Not an atomic
 *                  counter: the order of the list is part of the contract and the same in every run
 *   k_stickEmit    the same walk again; a lane meets j in ascending order and stores the partners at its start as it
 *                  goes, so its list comes out ascending with no sort
 * The last tile is part-filled: what lies past the last atom's rank bonds with nothing because of its rank, not because
 * of what the record holds.
 * A group whose lanes are all past the last atom does not exist (the grid is ceil(n / 256) groups, 9 766 for the largest
 * n); the lanes past n in the last group load tiles with the others and keep nothing.
 */
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <atomic>
#include <string>

#include "engine.h"
#include "stick_pairs.h"

namespace
{
constexpr int GROUP = 256;
constexpr long long MOST_PAIRS = 2147483647LL;

constexpr int BATCH = 8;

/* atom i against record t of a tile whose first record has rank i - self: all of the rule, no branch in it */
__device__ __forceinline__ unsigned partnerAt(const float4 *tile, const int t, const int self, const sticks::Point &a,
                                              const int flag, const float limit)
{
    const float4 b = tile[t];
    const sticks::Point other = {b.x, b.y, b.z};
    return (unsigned)(t != self) & (unsigned)(__float_as_int(b.w) == flag) & (unsigned)sticks::within(a, other, limit);
}

/* atom i against the atoms of one tile, `m` of them, the first of rank `base`, eight records at a time: their reads are
 * under way together and their verdicts come as one mask, bit u for rank first + u - hits(first, mask).  A whole tile is
 * walked with a constant trip count; in the last, part-filled one a record past the last atom's rank is read (it is
 * inside the tile, left over from the tile before or never written) and discarded by its rank, whatever it holds */
template <class Hits>
__device__ __forceinline__ void walkTile(const float4 *tile, const int m, const int base, const int i,
                                         const sticks::Point &a, const int flag, const float limit, Hits hits)
{
    const int self = i - base;
    if (m == GROUP)
        for (int t = 0; t < GROUP; t += BATCH)
        {
            unsigned mask = 0;
#pragma unroll
            for (int u = 0; u < BATCH; ++u)
                mask |= partnerAt(tile, t + u, self, a, flag, limit) << u;
            hits(base + t, mask);
        }
    else
        for (int t = 0; t < m; t += BATCH)
        {
            unsigned mask = 0;
#pragma unroll
            for (int u = 0; u < BATCH; ++u)
                mask |= ((unsigned)(t + u < m) & partnerAt(tile, t + u, self, a, flag, limit)) << u;
            hits(base + t, mask);
        }
}

/* the walk both kernels make.  EMIT false: counts[i] = the number of partners of atom i.  EMIT true: the partners of atom i
 * stored from start[i] on, those at places below `room` only */
template <bool EMIT>
__device__ __forceinline__ void walkAtoms(const float4 *__restrict__ atoms, const unsigned char *__restrict__ backbone,
                                          const int n, const float limitPlain, const float limitBackbone,
                                          long long *__restrict__ counts, const long long *__restrict__ start,
                                          int *__restrict__ partners, const long long room)
{
    __shared__ float4 tile[GROUP];
    const int i = blockIdx.x * GROUP + threadIdx.x;
    const bool live = i < n;
    sticks::Point a = {0.f, 0.f, 0.f};
    int flag = 0;
    if (live)
    {
        const float4 mine = atoms[i];
        a.x = mine.x, a.y = mine.y, a.z = mine.z;
        flag = backbone[i] != 0 ? 1 : 0;
    }
    const float limit = flag ? limitBackbone : limitPlain;
    long long at = 0;
    if (EMIT && live)
        at = start[i];
    int found = 0;
    for (int base = 0; base < n; base += GROUP)
    {
        const int j = base + (int)threadIdx.x;
        __syncthreads(); /* the tile before has been walked by every wave */
        if (j < n)
        {
            const float4 r = atoms[j];
            tile[threadIdx.x] = make_float4(r.x, r.y, r.z, __int_as_float(backbone[j] != 0 ? 1 : 0));
        }
        __syncthreads();
        const int m = n - base < GROUP ? n - base : GROUP;
        if (live)
            walkTile(tile, m, base, i, a, flag, limit, [&](int first, unsigned mask) {
                if (EMIT)
                    for (; mask != 0; mask &= mask - 1, ++at) /* lowest rank first */
                    {
                        if (at < room)
                            partners[at] = first + __ffs(mask) - 1;
                    }
                else
                    found += __popc(mask);
            });
    }
    if (!EMIT && live)
        counts[i] = found;
}

__global__ __launch_bounds__(GROUP) void k_stickCount(const float4 *__restrict__ atoms,
                                                      const unsigned char *__restrict__ backbone, const int n,
                                                      const float limitPlain, const float limitBackbone,
                                                      long long *__restrict__ counts)
{
    walkAtoms<false>(atoms, backbone, n, limitPlain, limitBackbone, counts, nullptr, nullptr, 0);
}

__global__ __launch_bounds__(GROUP) void k_stickEmit(const float4 *__restrict__ atoms,
                                                     const unsigned char *__restrict__ backbone, const int n,
                                                     const float limitPlain, const float limitBackbone,
                                                     const long long *__restrict__ start, int *__restrict__ partners,
                                                     const long long room)
{
    walkAtoms<true>(atoms, backbone, n, limitPlain, limitBackbone, nullptr, start, partners, room);
}

std::atomic<unsigned long long> gPairTests{0};

inline size_t roundUp(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
}

extern "C" {

long long solr_hip_stick_pairs(const float *atoms, const unsigned char *backbone, int n, float reachPlain,
                               float reachBackbone, long long *start, int *partners, long long capacity)
{
    using namespace solreng;
    if (!ok())
        return -1;
    /* ---- arguments: nothing is launched, no device touched, for a call that fails here ---- */
    if (const char *why = sticks::refusal(atoms, backbone, n, reachPlain, reachBackbone, start, partners, capacity))
    {
        setError(-1, (std::string("solr_hip_stick_pairs: ") + why).c_str(), __FILE__, __LINE__);
        return -1;
    }
    if (n == 0)
    {
        start[0] = 0;
        return 0;
    }
    const float limitPlain = sticks::squaredReach(reachPlain), limitBackbone = sticks::squaredReach(reachBackbone);

    int before = -1;
    if (hipGetDevice(&before) != hipSuccess)
        before = -1;
    HIPCHECK(hipSetDevice(solr_hip_get_device()));

    const size_t atomBytes = roundUp((size_t)n * 4 * sizeof(float)), flagBytes = roundUp((size_t)n);
    const size_t countBytes = roundUp(((size_t)n + 1) * sizeof(long long));
    size_t scanBytes = 0;
    unsigned char *pool = nullptr;
    int *dPartners = nullptr;
    hipStream_t stream = nullptr;
    long long total = 0;
    bool declined = false;
    if (ok())
        HIPCHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    if (ok())
        HIPCHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, scanBytes, (const long long *)nullptr, (long long *)nullptr,
                                                  n + 1, stream));
    if (ok())
        HIPCHECK(hipMalloc((void **)&pool, atomBytes + flagBytes + 2 * countBytes + roundUp(scanBytes)));
    if (ok())
    {
        float4 *dAtoms = reinterpret_cast<float4 *>(pool);
        unsigned char *dFlags = pool + atomBytes;
        long long *dCounts = reinterpret_cast<long long *>(pool + atomBytes + flagBytes);
        long long *dStart = reinterpret_cast<long long *>(pool + atomBytes + flagBytes + countBytes);
        unsigned char *dScan = pool + atomBytes + flagBytes + 2 * countBytes;
        const dim3 grid((unsigned)((n + GROUP - 1) / GROUP)), group(GROUP);

        HIPCHECK(hipMemcpyAsync(dAtoms, atoms, (size_t)n * 4 * sizeof(float), hipMemcpyHostToDevice, stream));
        if (ok())
            HIPCHECK(hipMemcpyAsync(dFlags, backbone, (size_t)n, hipMemcpyHostToDevice, stream));
        if (ok())
            HIPCHECK(hipMemsetAsync(dCounts + n, 0, sizeof(long long), stream));
        if (ok())
        {
            k_stickCount<<<grid, group, 0, stream>>>(dAtoms, dFlags, n, limitPlain, limitBackbone, dCounts);
            HIPCHECK(hipGetLastError());
        }
        size_t tb = scanBytes;
        if (ok())
            HIPCHECK(hipcub::DeviceScan::ExclusiveSum(dScan, tb, dCounts, dStart, n + 1, stream));
        if (ok())
            HIPCHECK(hipMemcpyAsync(start, dStart, ((size_t)n + 1) * sizeof(long long), hipMemcpyDeviceToHost, stream));
        if (ok())
            HIPCHECK(hipStreamSynchronize(stream));
        if (ok())
        {
            gPairTests += (unsigned long long)n * (unsigned long long)n;
            total = start[n];
            declined = total > MOST_PAIRS;
        }
        const long long room = total < capacity ? total : capacity;
        if (ok() && !declined && room > 0)
            HIPCHECK(hipMalloc((void **)&dPartners, (size_t)room * sizeof(int)));
        if (ok() && !declined && room > 0)
        {
            k_stickEmit<<<grid, group, 0, stream>>>(dAtoms, dFlags, n, limitPlain, limitBackbone, dStart, dPartners,
                                                    room);
            HIPCHECK(hipGetLastError());
            if (ok())
                HIPCHECK(hipMemcpyAsync(partners, dPartners, (size_t)room * sizeof(int), hipMemcpyDeviceToHost, stream));
            if (ok())
                HIPCHECK(hipStreamSynchronize(stream));
            if (ok())
                gPairTests += (unsigned long long)n * (unsigned long long)n;
        }
    }
    if (dPartners)
        (void)hipFree(dPartners);
    if (pool)
        (void)hipFree(pool);
    if (stream)
        (void)hipStreamDestroy(stream);
    if (before >= 0)
        (void)hipSetDevice(before);
    return ok() && !declined ? total : -1;
}

unsigned long long solr_hip_stick_pair_tests(void)
{
    return gPairTests.load();
}

} /* extern "C" */
