/*
 * iso_surface.h - the iso-surface of a field of metaballs as triangles: the scalar field on a cubic grid and marching
 * cubes over it.  IEEE binary32 in source order, written once for both sides: the host-only engine runs it in loops
 * (GPUKernel::isoField / isoTriangles), the HIP engine in kernels (csrc/solr_iso.hip).  Both are compiled without
 * contraction and with correctly rounded division (the Makefile's NUMERIC flags), so both give the same bits.
 *
 * It restates the arithmetic of the reference's animated scene, apps/scenes/animation/MetaballsScene.cpp:
 *   grid            vertex positions                                                          :92-109
 *   cubes           the eight corners of a cube, their order                                  :115-133
 *   field           value and gradient summed over the balls, ball after ball                 :266-296
 *   case            bit c set when corner c is below the threshold                            :309-324
 *   edge vertices   linear interpolation from the first end of an edge to the second          :334-351
 *   output          centre + scale * p, texture coordinates from x and z                      :355-393
 * The reference sums the balls in an OpenMP loop that shares its temporaries between threads (:260-296), so what it
 * computes is not defined; the definition here is the serial loop, ball 0 first.
 *
 * The table of triangles per case is NOT the reference's (MetaballsScene.h:103-377).  It is made by buildCaseTable()
 * below from the cube's geometry alone; see there.
 */
#pragma once

#include "../../include/solr_hip.h"

#if defined(__HIPCC__)
#define ISO_HD __host__ __device__
#else
#define ISO_HD
#endif

namespace iso
{
constexpr int MAX_CASE_TRIANGLES = 5;

/* triangles of every case: count[c] of them, edges[c][3 * t + v] the cube edge of vertex v of triangle t */
struct CaseTable
{
    unsigned char count[256];
    unsigned char edges[256][3 * MAX_CASE_TRIANGLES];
};

/* ---- the cube (MetaballsScene.cpp:122-130, MetaballsScene.h:100) -------------------------------------------------- */
/* corner c of a cube sits at (i + ci, j + cj, k + ck): 0 (0,0,0), 1 (0,0,1), 2 (0,1,1), 3 (0,1,0), 4 ... 7 with ci = 1 */
ISO_HD inline int cornerI(int c) { return c >> 2; }
ISO_HD inline int cornerJ(int c) { return (c >> 1) & 1; }
ISO_HD inline int cornerK(int c) { return (c ^ (c >> 1)) & 1; }
/* the two ends of edge e, in the direction it is interpolated: rings 0-1-2-3-0 and 4-5-6-7-4, then the uprights c - (c+4) */
ISO_HD inline int edgeFirst(int e) { return e < 8 ? (e & 4) + (e & 3) : e - 8; }
ISO_HD inline int edgeSecond(int e) { return e < 8 ? (e & 4) + ((e + 1) & 3) : e - 4; }

ISO_HD inline long vertexIndex(int n, int i, int j, int k) { return ((long)i * (n + 1) + j) * (n + 1) + k; }

/* the grid edge a cube's edge lies on: axis * (N+1)^3 + index of its lower grid vertex, axis 0 / 1 / 2 for i / j / k */
ISO_HD inline int gridEdge(int n, int i, int j, int k, int e)
{
    const int a = edgeFirst(e), b = edgeSecond(e);
    const int ai = cornerI(a), aj = cornerJ(a), ak = cornerK(a);
    const int bi = cornerI(b), bj = cornerJ(b), bk = cornerK(b);
    const int axis = ai != bi ? 0 : (aj != bj ? 1 : 2);
    const long lower = vertexIndex(n, i + (ai < bi ? ai : bi), j + (aj < bj ? aj : bj), k + (ak < bk ? ak : bk));
    return (int)((long)axis * (n + 1) * (n + 1) * (n + 1) + lower);
}

/* ---- the grid (MetaballsScene.cpp:99-101) ------------------------------------------------------------------------ */
ISO_HD inline float coordinate(int index, float size, int n)
{
    return ((float)index * size) / (float)n - size / 2.f;
}

/* ---- the field at one grid vertex (MetaballsScene.cpp:266-296): out = {normal x, y, z, value} ---------------------- */
/* balls: nbBalls records of x, y, z, squared radius */
ISO_HD inline void fieldAt(float px, float py, float pz, const float *balls, int nbBalls, float out[4])
{
    float value = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    for (int b = 0; b < nbBalls; ++b)
    {
        const float sr = balls[4 * b + 3] / 4.f;
        const float dx = px - balls[4 * b + 0];
        const float dy = py - balls[4 * b + 1];
        const float dz = pz - balls[4 * b + 2];
        float d2 = dx * dx + dy * dy + dz * dz;
        if (d2 == 0.0f)
            d2 = 0.0001f;
        value += sr / d2;
        const float ns = sr / (d2 * d2);
        nx += dx * ns;
        ny += dy * ns;
        nz += dz * ns;
    }
    out[0] = nx;
    out[1] = ny;
    out[2] = nz;
    out[3] = value;
}

/* ---- a cube's case (MetaballsScene.cpp:309-324) ------------------------------------------------------------------- */
/* field: (N+1)^3 records of {nx, ny, nz, value} */
ISO_HD inline int cubeCase(const float *field, int n, int i, int j, int k, float threshold)
{
    int c = 0;
    for (int corner = 0; corner < 8; ++corner)
        if (field[4 * vertexIndex(n, i + cornerI(corner), j + cornerJ(corner), k + cornerK(corner)) + 3] < threshold)
            c |= 1 << corner;
    return c;
}

/* ---- one vertex of the surface (MetaballsScene.cpp:338-349, :367-373) ---------------------------------------------- */
/* on edge e of cube (i, j, k): position transformed, normal as interpolated, texture coordinates */
ISO_HD inline void edgeVertex(const SolrIsoGrid &grid, const float *field, int i, int j, int k, int e, float p[3],
                              float normal[3], float vt[2])
{
    const int n = grid.gridSize;
    const int a = edgeFirst(e), b = edgeSecond(e);
    const int i1 = i + cornerI(a), j1 = j + cornerJ(a), k1 = k + cornerK(a);
    const int i2 = i + cornerI(b), j2 = j + cornerJ(b), k2 = k + cornerK(b);
    const float *v1 = field + 4 * vertexIndex(n, i1, j1, k1);
    const float *v2 = field + 4 * vertexIndex(n, i2, j2, k2);
    const float delta = (grid.threshold - v1[3]) / (v2[3] - v1[3]);
    const float p1[3] = {coordinate(i1, grid.size[0], n), coordinate(j1, grid.size[1], n),
                         coordinate(k1, grid.size[2], n)};
    const float p2[3] = {coordinate(i2, grid.size[0], n), coordinate(j2, grid.size[1], n),
                         coordinate(k2, grid.size[2], n)};
    float q[3];
    for (int c = 0; c < 3; ++c)
    {
        q[c] = p1[c] + delta * (p2[c] - p1[c]);
        normal[c] = v1[c] + delta * (v2[c] - v1[c]);
    }
    /* the reference multiplies y by scale.x (:373); its scale is uniform, so scale.y is the same number there */
    for (int c = 0; c < 3; ++c)
        p[c] = grid.center[c] + grid.scale[c] * q[c];
    vt[0] = q[0] / grid.textureGrid + 1.5f;
    vt[1] = q[2] / grid.textureGrid + 1.5f;
}

/* triangle t of a cube of case c */
ISO_HD inline void cubeTriangle(const SolrIsoGrid &grid, const CaseTable *table, const float *field, int i, int j, int k,
                                int c, int t, SolrIsoTriangle *out)
{
    const int n = grid.gridSize;
    out->cube = (i * n + j) * n + k;
    for (int v = 0; v < 3; ++v)
    {
        const int e = table->edges[c][3 * t + v];
        edgeVertex(grid, field, i, j, k, e, out->p[v], out->n[v], out->vt[v]);
        out->edge[v] = gridEdge(n, i, j, k, e);
    }
}

/* ---- arguments both engines refuse (include/solr_hip.h) ------------------------------------------------------------ */
ISO_HD inline bool isFinite(float x) { return x - x == 0.f; }
inline const char *refusal(const SolrIsoGrid *grid, int nbBalls, int capacity)
{
    if (!grid)
        return "null grid";
    if (grid->gridSize < 1 || grid->gridSize > SOLR_ISO_MAX_GRID)
        return "gridSize must be 1 ... SOLR_ISO_MAX_GRID";
    if (nbBalls < 0 || nbBalls > SOLR_ISO_MAX_BALLS)
        return "nbBalls must be 0 ... SOLR_ISO_MAX_BALLS";
    if (!isFinite(grid->threshold) || !isFinite(grid->size[0]) || !isFinite(grid->size[1]) || !isFinite(grid->size[2]))
        return "the threshold and the size must be finite";
    if (capacity < 0)
        return "negative capacity";
    return nullptr;
}

/* ---- the table of cases ------------------------------------------------------------------------------------------- */
/*
 * For each of the 256 cases, from the cube's geometry alone:
 *   - an edge is crossed when its two ends differ in their bit
 *   - on each of the six faces 0, 2 or 4 edges are crossed.  Two: one segment joins them.  Four: the face is ambiguous,
 *     its diagonal corners alike; two segments, each joining the two face edges that meet at a corner whose bit is SET.
 *     The rule reads the face's four bits only, so the two cubes that share a face draw the same segments on it and the
 *     surface has no holes
 *   - every crossed edge lies in two faces and so has two segments: the segments fall into closed loops, taken in order
 *     of their lowest-numbered edge and each begun there
 *   - a loop's direction: with the crossing points at the edge midpoints of the unit cube, A = sum P[n] x P[n+1] is its
 *     area vector and d = sum over its edges of (end with bit clear - end with bit set); the loop runs so that A . d > 0
 *   - a loop e[0 ... m-1] gives the fan (e[0], e[n], e[n+1]), n = 1 ... m-2
 * All in integers (midpoints doubled).  False when a property the construction rests on fails - it never does: the
 * counts it checks were measured once (no case above 5 triangles, 820 in all, no loop above 7 edges, A . d never 0).
 */
inline bool buildCaseTable(CaseTable &table)
{
    int faceEdges[6][4], faceCorners[6][4];
    for (int f = 0; f < 6; ++f)
    {
        const int axis = f >> 1, side = f & 1;
        int nc = 0, ne = 0;
        for (int c = 0; c < 8; ++c)
            if ((axis == 0 ? cornerI(c) : axis == 1 ? cornerJ(c) : cornerK(c)) == side)
                faceCorners[f][nc++] = c;
        for (int e = 0; e < 12; ++e)
        {
            bool first = false, second = false;
            for (int c = 0; c < 4; ++c)
            {
                first |= faceCorners[f][c] == edgeFirst(e);
                second |= faceCorners[f][c] == edgeSecond(e);
            }
            if (first && second)
            {
                if (ne == 4)
                    return false;
                faceEdges[f][ne++] = e;
            }
        }
        if (nc != 4 || ne != 4)
            return false;
    }

    int total = 0, longest = 0;
    for (int c = 0; c < 256; ++c)
    {
        int link[12][2], links[12];
        bool crossed[12], seen[12];
        for (int e = 0; e < 12; ++e)
        {
            crossed[e] = ((c >> edgeFirst(e)) & 1) != ((c >> edgeSecond(e)) & 1);
            links[e] = 0;
            seen[e] = false;
        }
        for (int f = 0; f < 6; ++f)
        {
            int on[4], nOn = 0;
            for (int s = 0; s < 4; ++s)
                if (crossed[faceEdges[f][s]])
                    on[nOn++] = faceEdges[f][s];
            int segments[2][2], nSegments = 0;
            if (nOn == 2)
            {
                segments[0][0] = on[0];
                segments[0][1] = on[1];
                nSegments = 1;
            }
            else if (nOn == 4)
            {
                for (int s = 0; s < 4; ++s)
                {
                    const int corner = faceCorners[f][s];
                    if (!((c >> corner) & 1))
                        continue;
                    int at[2], nAt = 0;
                    for (int q = 0; q < 4; ++q)
                    {
                        const int e = faceEdges[f][q];
                        if (edgeFirst(e) == corner || edgeSecond(e) == corner)
                        {
                            if (nAt == 2)
                                return false;
                            at[nAt++] = e;
                        }
                    }
                    if (nAt != 2 || nSegments == 2)
                        return false;
                    segments[nSegments][0] = at[0];
                    segments[nSegments][1] = at[1];
                    ++nSegments;
                }
                if (nSegments != 2)
                    return false;
            }
            else if (nOn != 0)
                return false;
            for (int s = 0; s < nSegments; ++s)
                for (int side = 0; side < 2; ++side)
                {
                    const int e = segments[s][side];
                    if (links[e] == 2)
                        return false;
                    link[e][links[e]++] = segments[s][1 - side];
                }
        }
        for (int e = 0; e < 12; ++e)
            if (crossed[e] && links[e] != 2)
                return false;

        int nbTriangles = 0;
        for (int e0 = 0; e0 < 12; ++e0)
        {
            if (!crossed[e0] || seen[e0])
                continue;
            int loop[12], m = 0, previous = -1, current = e0;
            for (;;)
            {
                if (m == 12)
                    return false;
                loop[m++] = current;
                seen[current] = true;
                const int next = link[current][0] == previous ? link[current][1] : link[current][0];
                if (next == e0)
                    break;
                if (seen[next])
                    return false;
                previous = current;
                current = next;
            }
            if (m < 3)
                return false;
            if (m > longest)
                longest = m;
            /* twice the midpoints: whole numbers */
            int P[12][3], d[3] = {0, 0, 0};
            for (int n = 0; n < m; ++n)
            {
                const int a = edgeFirst(loop[n]), b = edgeSecond(loop[n]);
                P[n][0] = cornerI(a) + cornerI(b);
                P[n][1] = cornerJ(a) + cornerJ(b);
                P[n][2] = cornerK(a) + cornerK(b);
                const int set = ((c >> a) & 1) ? a : b, clear = ((c >> a) & 1) ? b : a;
                d[0] += cornerI(clear) - cornerI(set);
                d[1] += cornerJ(clear) - cornerJ(set);
                d[2] += cornerK(clear) - cornerK(set);
            }
            int A[3] = {0, 0, 0};
            for (int n = 0; n < m; ++n)
            {
                const int *p = P[n], *q = P[(n + 1) % m];
                A[0] += p[1] * q[2] - p[2] * q[1];
                A[1] += p[2] * q[0] - p[0] * q[2];
                A[2] += p[0] * q[1] - p[1] * q[0];
            }
            const int dot = A[0] * d[0] + A[1] * d[1] + A[2] * d[2];
            if (dot == 0)
                return false;
            if (dot < 0)
                for (int lo = 1, hi = m - 1; lo < hi; ++lo, --hi)
                {
                    const int swap = loop[lo];
                    loop[lo] = loop[hi];
                    loop[hi] = swap;
                }
            for (int n = 1; n + 1 < m; ++n)
            {
                if (nbTriangles == MAX_CASE_TRIANGLES)
                    return false;
                table.edges[c][3 * nbTriangles + 0] = (unsigned char)loop[0];
                table.edges[c][3 * nbTriangles + 1] = (unsigned char)loop[n];
                table.edges[c][3 * nbTriangles + 2] = (unsigned char)loop[n + 1];
                ++nbTriangles;
            }
        }
        table.count[c] = (unsigned char)nbTriangles;
        for (int s = 3 * nbTriangles; s < 3 * MAX_CASE_TRIANGLES; ++s)
            table.edges[c][s] = 0;
        total += nbTriangles;
    }
    const unsigned char *one = table.edges[1], *three = table.edges[3];
    return total == 820 && longest == 7 && table.count[1] == 1 && one[0] == 0 && one[1] == 8 && one[2] == 3 &&
           table.count[3] == 2 && three[0] == 1 && three[1] == 9 && three[2] == 8 && three[3] == 1 && three[4] == 8 &&
           three[5] == 3;
}

/* the table, built on first use; null when buildCaseTable failed (it does not) */
inline const CaseTable *caseTable()
{
    static CaseTable table;
    static const bool good = buildCaseTable(table);
    return good ? &table : nullptr;
}

/* ---- the loops of the host-only engine ----------------------------------------------------------------------------- */
/* field: (N+1)^3 records of {nx, ny, nz, value}, vertex (i, j, k) at (i * (N+1) + j) * (N+1) + k */
inline void fieldLoop(const SolrIsoGrid &grid, const float *balls, int nbBalls, float *field)
{
    const int n = grid.gridSize;
    for (int i = 0; i <= n; ++i)
        for (int j = 0; j <= n; ++j)
            for (int k = 0; k <= n; ++k)
                fieldAt(coordinate(i, grid.size[0], n), coordinate(j, grid.size[1], n), coordinate(k, grid.size[2], n),
                        balls, nbBalls, field + 4 * vertexIndex(n, i, j, k));
}

/* cubes in index order, a cube's triangles in table order (what the reference's serial loop over the cubes produces):
 * the number of triangles the surface has; the first min(count, capacity) are written */
inline int surfaceLoop(const SolrIsoGrid &grid, const CaseTable &table, const float *field, SolrIsoTriangle *triangles,
                       int capacity)
{
    const int n = grid.gridSize;
    int count = 0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            for (int k = 0; k < n; ++k)
            {
                const int c = cubeCase(field, n, i, j, k, grid.threshold);
                for (int t = 0; t < table.count[c]; ++t, ++count)
                    if (count < capacity)
                        cubeTriangle(grid, &table, field, i, j, k, c, t, triangles + count);
            }
    return count;
}
}
