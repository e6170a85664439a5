/*
 * solr_iso.hip - the iso-surface of a field of metaballs on the device (include/solr_hip.h: solr_hip_iso_field,
 * solr_hip_iso_surface, solr_hip_metaballs).  The arithmetic is iso_surface.h - that of the reference's
 * apps/scenes/animation/MetaballsScene.cpp, binary32 in source order - and this file is only its lane mapping; the
 * host-only engine runs the same header in loops (host/GPUKernel.cpp) and gives the same bits.  gfx950 only.
 *
 *   k_isoField   a lane per grid vertex, k fastest: a wave stores 64 consecutive 16-byte records.  Every lane walks the
 *                balls in order; the ball index is the loop counter, the same in every lane, and the balls come through
 *                a const __restrict__ pointer, so the compiler fetches a ball once per wave into scalar registers
 *   k_isoCount   a lane per cube: the case from the eight corner values, the case and its number of triangles out
 *   (scan)       hipcub::DeviceScan::ExclusiveSum of the counts: where each cube's triangles begin.  Not an atomic
 *                counter: the order of the triangles is part of the contract and the same in every run
 *   k_isoEmit    a lane per cube with triangles: each one built in registers and stored as seven 16-byte stores
 * The case table (4 KiB, iso::CaseTable) is built on the host by the header's generator and uploaded once per device to
 * global memory; every lane reads the entry of its own case, so it is no constant-memory broadcast.
 */
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <atomic>
#include <mutex>
#include <string>

#include "engine.h"
#include "iso_surface.h"

namespace
{
constexpr int GROUP = 256;
constexpr int MAX_DEVICES = 64;

static_assert(sizeof(SolrIsoTriangle) == 112, "SolrIsoTriangle is seven 16-byte stores");
static_assert(sizeof(iso::CaseTable) == 4096, "the case table is 4 KiB");

__global__ __launch_bounds__(GROUP) void k_isoField(const SolrIsoGrid grid, const float *__restrict__ balls,
                                                    const int nbBalls, const int nbVertices, float4 *__restrict__ field)
{
    const int vertex = blockIdx.x * GROUP + threadIdx.x;
    if (vertex >= nbVertices)
        return;
    const int side = grid.gridSize + 1;
    const int k = vertex % side, ij = vertex / side, j = ij % side, i = ij / side;
    float out[4];
    iso::fieldAt(iso::coordinate(i, grid.size[0], grid.gridSize), iso::coordinate(j, grid.size[1], grid.gridSize),
                 iso::coordinate(k, grid.size[2], grid.gridSize), balls, nbBalls, out);
    field[vertex] = make_float4(out[0], out[1], out[2], out[3]);
}

__global__ __launch_bounds__(GROUP) void k_isoCount(const int n, const float threshold, const int nbCubes,
                                                    const iso::CaseTable *__restrict__ table,
                                                    const float *__restrict__ field, unsigned char *__restrict__ cases,
                                                    int *__restrict__ counts)
{
    const int cube = blockIdx.x * GROUP + threadIdx.x;
    if (cube >= nbCubes)
        return;
    const int k = cube % n, ij = cube / n, j = ij % n, i = ij / n;
    const int c = iso::cubeCase(field, n, i, j, k, threshold);
    cases[cube] = (unsigned char)c;
    counts[cube] = table->count[c];
}

/* limit: how many triangles `triangles` has room for (min(count, capacity)); a cube's triangles beyond it are not built */
__global__ __launch_bounds__(GROUP) void k_isoEmit(const SolrIsoGrid grid, const int nbCubes, const int limit,
                                                   const iso::CaseTable *__restrict__ table,
                                                   const float *__restrict__ field,
                                                   const unsigned char *__restrict__ cases,
                                                   const int *__restrict__ offsets, uint4 *__restrict__ triangles)
{
    const int cube = blockIdx.x * GROUP + threadIdx.x;
    if (cube >= nbCubes)
        return;
    const int c = cases[cube];
    const int count = table->count[c];
    if (count == 0)
        return;
    const int n = grid.gridSize;
    const int k = cube % n, ij = cube / n, j = ij % n, i = ij / n;
    const int first = offsets[cube];
    for (int t = 0; t < count && first + t < limit; ++t)
    {
        union
        {
            SolrIsoTriangle triangle;
            uint4 words[7];
        } record;
        iso::cubeTriangle(grid, table, field, i, j, k, c, t, &record.triangle);
        uint4 *to = triangles + (size_t)(first + t) * 7;
#pragma unroll
        for (int w = 0; w < 7; ++w)
            to[w] = record.words[w];
    }
}

std::atomic<unsigned long long> gIsoCubes{0};
std::mutex gTableMutex;
iso::CaseTable *gTables[MAX_DEVICES];

inline size_t roundUp(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
inline dim3 groups(long n) { return dim3((unsigned)((n + GROUP - 1) / GROUP)); }

/* the case table on the current device: built and uploaded on the first call, kept from then on */
const iso::CaseTable *deviceTable(int device, hipStream_t stream)
{
    using namespace solreng;
    const iso::CaseTable *host = iso::caseTable();
    if (!host || device < 0 || device >= MAX_DEVICES)
    {
        setError(-1, "solr_iso: no case table", __FILE__, __LINE__);
        return nullptr;
    }
    std::lock_guard<std::mutex> lock(gTableMutex);
    if (!gTables[device])
    {
        iso::CaseTable *table = nullptr;
        HIPCHECK(hipMalloc((void **)&table, sizeof(iso::CaseTable)));
        if (ok())
            HIPCHECK(hipMemcpyAsync(table, host, sizeof(iso::CaseTable), hipMemcpyHostToDevice, stream));
        if (ok())
            HIPCHECK(hipStreamSynchronize(stream));
        if (!ok())
        {
            if (table)
                (void)hipFree(table);
            return nullptr;
        }
        gTables[device] = table;
    }
    return gTables[device];
}

/* balls -> field and / or field -> triangles.  hostBalls: field from the balls (else uploaded from hostFieldIn);
 * hostFieldOut: the field copied back; surface: the cubes run.  The number of triangles, 0 for the field alone, -1 */
int run(const char *who, const SolrIsoGrid *grid, const float *hostBalls, int nbBalls, const float *hostFieldIn,
        float *hostFieldOut, bool surface, SolrIsoTriangle *hostTriangles, int capacity)
{
    using namespace solreng;
    if (!ok())
        return -1;
    /* ---- arguments: nothing is launched for a call that fails here ---- */
    const bool fromBalls = hostFieldIn == nullptr;
    const char *why = iso::refusal(grid, nbBalls, capacity);
    if (!why && fromBalls && !hostBalls)
        why = "null balls";
    if (!why && !surface && !hostFieldOut)
        why = "null field";
    if (!why && surface && !hostTriangles && capacity != 0)
        why = "null triangles with a capacity";
    if (why)
    {
        setError(-1, (std::string(who) + ": " + why).c_str(), __FILE__, __LINE__);
        return -1;
    }
    const int n = grid->gridSize;
    const long nbVertices = (long)(n + 1) * (n + 1) * (n + 1), nbCubes = (long)n * n * n;

    int before = -1;
    if (hipGetDevice(&before) != hipSuccess)
        before = -1;
    const int device = solr_hip_get_device();
    HIPCHECK(hipSetDevice(device));

    const size_t fieldBytes = roundUp((size_t)nbVertices * 4 * sizeof(float));
    const size_t ballBytes = roundUp((size_t)(nbBalls > 0 ? nbBalls : 1) * 4 * sizeof(float));
    const size_t countBytes = roundUp((size_t)nbCubes * sizeof(int)), caseBytes = roundUp((size_t)nbCubes);
    size_t scanBytes = 0;
    unsigned char *pool = nullptr, *dTriangles = nullptr;
    hipStream_t stream = nullptr;
    int count = 0;
    if (ok())
        HIPCHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    if (ok() && surface)
        HIPCHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, scanBytes, (const int *)nullptr, (int *)nullptr, (int)nbCubes,
                                                  stream));
    const size_t surfaceBytes = surface ? 2 * countBytes + caseBytes + roundUp(scanBytes) : 0;
    if (ok())
        HIPCHECK(hipMalloc((void **)&pool, fieldBytes + ballBytes + surfaceBytes));
    if (ok())
    {
        float *dField = reinterpret_cast<float *>(pool);
        float *dBalls = reinterpret_cast<float *>(pool + fieldBytes);
        int *dCounts = reinterpret_cast<int *>(pool + fieldBytes + ballBytes);
        int *dOffsets = reinterpret_cast<int *>(pool + fieldBytes + ballBytes + countBytes);
        unsigned char *dCases = pool + fieldBytes + ballBytes + 2 * countBytes;
        unsigned char *dScan = dCases + caseBytes;

        if (fromBalls)
        {
            if (nbBalls > 0)
                HIPCHECK(hipMemcpyAsync(dBalls, hostBalls, (size_t)nbBalls * 4 * sizeof(float), hipMemcpyHostToDevice,
                                        stream));
            if (ok())
            {
                k_isoField<<<groups(nbVertices), dim3(GROUP), 0, stream>>>(*grid, dBalls, nbBalls, (int)nbVertices,
                                                                           reinterpret_cast<float4 *>(dField));
                HIPCHECK(hipGetLastError());
            }
            if (ok() && hostFieldOut)
                HIPCHECK(hipMemcpyAsync(hostFieldOut, dField, (size_t)nbVertices * 4 * sizeof(float),
                                        hipMemcpyDeviceToHost, stream));
        }
        else
            HIPCHECK(hipMemcpyAsync(dField, hostFieldIn, (size_t)nbVertices * 4 * sizeof(float), hipMemcpyHostToDevice,
                                    stream));

        const iso::CaseTable *dTable = ok() && surface ? deviceTable(device, stream) : nullptr;
        if (ok() && surface && dTable)
        {
            k_isoCount<<<groups(nbCubes), dim3(GROUP), 0, stream>>>(n, grid->threshold, (int)nbCubes, dTable, dField,
                                                                    dCases, dCounts);
            HIPCHECK(hipGetLastError());
            size_t tb = scanBytes;
            if (ok())
                HIPCHECK(hipcub::DeviceScan::ExclusiveSum(dScan, tb, dCounts, dOffsets, (int)nbCubes, stream));
            int lastOffset = 0, lastCount = 0;
            if (ok())
                HIPCHECK(hipMemcpyAsync(&lastOffset, dOffsets + (nbCubes - 1), sizeof(int), hipMemcpyDeviceToHost,
                                        stream));
            if (ok())
                HIPCHECK(hipMemcpyAsync(&lastCount, dCounts + (nbCubes - 1), sizeof(int), hipMemcpyDeviceToHost,
                                        stream));
            if (ok())
                HIPCHECK(hipStreamSynchronize(stream));
            count = lastOffset + lastCount;
            const int limit = count < capacity ? count : capacity;
            if (ok() && limit > 0)
                HIPCHECK(hipMalloc((void **)&dTriangles, (size_t)limit * sizeof(SolrIsoTriangle)));
            if (ok() && limit > 0)
            {
                k_isoEmit<<<groups(nbCubes), dim3(GROUP), 0, stream>>>(*grid, (int)nbCubes, limit, dTable, dField,
                                                                       dCases, dOffsets,
                                                                       reinterpret_cast<uint4 *>(dTriangles));
                HIPCHECK(hipGetLastError());
                if (ok())
                    HIPCHECK(hipMemcpyAsync(hostTriangles, dTriangles, (size_t)limit * sizeof(SolrIsoTriangle),
                                            hipMemcpyDeviceToHost, stream));
            }
        }
        HIPCHECK(hipStreamSynchronize(stream));
        if (ok() && surface)
            gIsoCubes += (unsigned long long)nbCubes;
    }
    if (dTriangles)
        (void)hipFree(dTriangles);
    if (pool)
        (void)hipFree(pool);
    if (stream)
        (void)hipStreamDestroy(stream);
    if (before >= 0)
        (void)hipSetDevice(before);
    return ok() ? count : -1;
}
}

extern "C" {

int solr_hip_iso_field(const SolrIsoGrid *grid, const float *balls, int nbBalls, float *field)
{
    return run("solr_hip_iso_field", grid, balls, nbBalls, nullptr, field, false, nullptr, 0);
}

int solr_hip_iso_surface(const SolrIsoGrid *grid, const float *field, SolrIsoTriangle *triangles, int capacity)
{
    if (!field)
    {
        if (solreng::ok())
            solreng::setError(-1, "solr_hip_iso_surface: null field", __FILE__, __LINE__);
        return -1;
    }
    return run("solr_hip_iso_surface", grid, nullptr, 0, field, nullptr, true, triangles, capacity);
}

int solr_hip_metaballs(const SolrIsoGrid *grid, const float *balls, int nbBalls, SolrIsoTriangle *triangles,
                       int capacity)
{
    return run("solr_hip_metaballs", grid, balls, nbBalls, nullptr, nullptr, true, triangles, capacity);
}

unsigned long long solr_hip_iso_cubes(void)
{
    return gIsoCubes.load();
}

} /* extern "C" */
