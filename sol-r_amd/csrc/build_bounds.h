/*
 * build_bounds.h - the box of a leaf that the order-free hierarchy is BUILT on (list_builders.cpp buildFreeOrderLists,
 * solr_lists.hip): the box a long ray will test, which for a leaf of axis-plane rectangles is not the box as uploaded
 * (the reference boxes a wall as p0 +- size on all three axes) but the rectangles' own, one margin thick - the
 * arithmetic of the thin copy (solr_arena.hip k_tightenLeaves calls the same function), decided by primitive type alone: materials may arrive
 * after the lists, and any hierarchy over the leaves is correct.  What the lists hold is never this box: leaves are
 * emitted as uploaded, inner nodes as the unions of those.
 * One function for the host and the device builder, which have to make the same lists bit for bit; plain float
 * arithmetic, no contraction possible (no product feeds a sum but products by a power of two, which are exact).
 * For the thin copy alone (byKind, with a `reach`) the same goes for a leaf of spheres that is boxed larger than its
 * spheres (the reference's light cell: one lamp of radius 10 in +-viewDistance, GPUKernel.cpp:1189) - see
 * sphereBuildExtent.  The hierarchy is still built on such a leaf's box as uploaded: the builders pass no reach.
 */
#ifndef SOLR_BUILD_BOUNDS_H
#define SOLR_BUILD_BOUNDS_H

#include <hip/hip_vector_types.h>

#include <cmath>
#include <cstring>

#include "../../include/solr_types.h"

#if defined(__HIPCC__)
#define SOLR_BUILD_BOUNDS_FN __host__ __device__ inline
#else
#define SOLR_BUILD_BOUNDS_FN inline
#endif

namespace solreng
{
/* Which share of its range's surface measure (xy + yz + zx of the union of the build boxes) makes a leaf dominant:
 * it is taken out of the range before the binned split and emitted as a sibling of the subtree over the rest
 * (profiles/r15/free_list_topology.txt has the counts behind the number).  A wall of a cubic room is 1/3 of the room. */
#define SOLR_DOMINANT_SHARE 0.25

/* How the order-free hierarchy is built.  prims == nullptr: on the boxes as uploaded, nothing set apart - the lists of
 * every build before this one.  Otherwise `prims` are the primitive records (8 rows each: p0 | type word, size | ...),
 * tagged or not, on the side of the caller (host memory for the host builder, device memory for the device's). */
struct BuildBounds
{
    const float4 *prims = nullptr;
    float margin = 0.f;                 /* scene extent / 1024, as the thin copies take it */
    double dominantShare = SOLR_DOMINANT_SHARE; /* <= 0: no leaf is set apart */
};

/* the kinds a primitive record's tag holds for a PLAIN axis plane and for a sphere whose test is sphereHit alone - ptSphere,
 * not procedural, whatever else its material is (the lamps' emissive one included; ptEnvironment and ptCamera are other
 * types and never get it) - (scene_layout.h PrimKind, bits 24 ... 27 of the type word; solr_arena.hip holds these to that
 * header) */
enum BuildBoundsPlainKind
{
    BB_KIND_SHIFT = 24,
    BB_KIND_SPHERE = 1,
    BB_KIND_PLANE_XY = 2,
    BB_KIND_PLANE_YZ = 3,
    BB_KIND_PLANE_XZ = 4
};

/* The bin of a leaf's centre c among the `bins` bins of a node whose centres begin at `origin`, scale = bins / extent:
 * the one place where both builders turn a float into an integer.  Clamped in float BEFORE the conversion, so that it
 * is defined on both sides whatever the product: once the extent of the centres is below about 4.7e-38 the scale is
 * infinite and the product +inf or (0 x inf) NaN - (int) of those is undefined on the host (x86 gives INT_MIN: bin 0)
 * and saturates on the device (bin 0 or the last).  Here NaN is bin 0 and +inf the last bin.  Any product in [0, bins),
 * which is every one of a scene with ordinary extents, gets the bin min(bins - 1, max(0, (int)product)) always gave. */
SOLR_BUILD_BOUNDS_FN int centreBin(float c, float origin, float scale, int bins)
{
    const float at = (c - origin) * scale;
    const float last = (float)(bins - 1);
    return (int)(at > 0.f ? (at < last ? at : last) : 0.f);
}

/* How far the thin box of a sphere (centre p, radius |r|) reaches from p on every axis, for rays whose origins lie within
 * `reach` of zero on every axis (rt_device.h tightRay: the frame's viewDistance): every ray that the sphere test
 * (rt_device.h sphereHit) says hits has to pass the slab test of that box.  A true hit lies on the sphere, inside p +- |r|.
 * But the test decides by the sign of d = b b - 2 a c, a difference of two numbers of the size 4 s^2, s = |o - p|, each
 * with a few roundings behind it: |d - 4 |n|^2 (r^2 - q^2)| <= 64 u s^2 |n|^2 (u = 2^-24, q the distance of the ray's line
 * from p, n the normalised direction as computed; 28 u from b b, 36 u from 2 a c), so a ray that passes the sphere at up to
 * q - |r| < 16 u s^2 / (q + |r|) <= 8 u s^2 / |r| = 2^-21 s^2 / |r| can be called a hit, and the parameter of that hit is
 * off by up to sqrt(64 u) s / 2 = 2^-10 s along the ray - the origin may lie that far behind the sphere.  With
 * s^2 <= 3 far^2, far = reach + max |p.xyz|, the box p +- (|r| + 3 far^2 2^-21 / |r| + far 2^-9) (sqrt(3) 2^-10 rounded up)
 * holds every such ray's closest point to p, its origin if that lies behind it, and every such hit point; the margin on top
 * covers the slab test's own rounding as it does for the rectangles (rt_device.h, TIGHT LEAVES).  For the Cornell scene's
 * lamp (radius 10 at (8000, 8000, -8000), reach 55 000) that is +- 755 where the box as uploaded is +- 50 000;
 * tests/test_sphere_leaf_margin.py puts the claim to grazing rays in
 * numpy's binary32.  Not a number, infinite, or a radius of zero: not finite, and the caller keeps the box as uploaded. */
SOLR_BUILD_BOUNDS_FN float sphereBuildExtent(const float4 &p, float radius, float margin, float reach)
{
    const float r = fabsf(radius);
    const float far = reach + fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fabsf(p.z));
    return ((r + margin) + (3.f * far * 0x1p-21f) / (r / far)) + far * 0x1p-9f;
}

/* The build box of the leaf { row0, row1 } whose `count` primitives begin at prims[8 * start].  true: the leaf holds
 * nothing but axis-plane rectangles - or, byKind and with a reach, nothing but spheres - and lo / hi are their thin box cut with the
 * leaf's own; false: lo / hi are the leaf's box as uploaded (a leaf that mixes the two among them).  A leaf whose box
 * as uploaded already is its spheres' p0 +- r - what the reference's builder gives every sphere but the lamps - comes
 * out of the cut as it went in.  byKind: a rectangle is what the record's tag calls a plain plane, not what its type says -
 * the thin copy's rule (solr_arena.hip k_tightenLeaves, which is this function: one arithmetic for the box a ray
 * tests and the box the hierarchy is built on) - and, with a reach, a sphere what it calls KIND_SPHERE.  By type there is
 * no clause for spheres: a procedural sphere's surface is displaced, and the type does not say which are. */
SOLR_BUILD_BOUNDS_FN bool leafBuildBounds(const float4 &row0, const float4 &row1, const float4 *prims, int start, int count, float margin,
                                          float lo[3], float hi[3], bool byKind = false, float reach = 0.f)
{
    lo[0] = row0.x, lo[1] = row0.y, lo[2] = row0.z;
    hi[0] = row1.x, hi[1] = row1.y, hi[2] = row0.w;
    if (prims == nullptr || count <= 0 || start < 0)
        return false;
    float lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
    bool spheres = false;
    for (int k = 0; k < count; ++k)
    {
        const float4 p = prims[8 * (size_t)(start + k)], s = prims[8 * (size_t)(start + k) + 1];
        int word;
        memcpy(&word, &p.w, 4);
        const int type = word & 0xff, kind = (word >> BB_KIND_SHIFT) & 15;
        /* the axis the rectangle lies across */
        const int across = byKind ? (kind == BB_KIND_PLANE_YZ ? 0 : kind == BB_KIND_PLANE_XZ ? 1 : kind == BB_KIND_PLANE_XY ? 2 : -1)
                                  : (type == ptYZPlane ? 0 : type == ptXZPlane ? 1 : type == ptXYPlane ? 2 : -1);
        const bool sphere = reach > 0.f && byKind && kind == BB_KIND_SPHERE;
        if ((across < 0 && !sphere) || (k > 0 && sphere != spheres))
            return false;
        spheres = sphere;
        /* (a size is compared with a distance: its sign cannot make the rectangle larger than |size|) */
        float ex = across == 0 ? margin : fabsf(s.x) + margin;
        float ey = across == 1 ? margin : fabsf(s.y) + margin;
        float ez = across == 2 ? margin : fabsf(s.z) + margin;
        if (sphere)
        {
            ex = ey = ez = sphereBuildExtent(p, s.x, margin, reach);
            if (!(ex < 3.0e38f && fabsf(p.x) < 3.0e38f && fabsf(p.y) < 3.0e38f && fabsf(p.z) < 3.0e38f))
                return false;
        }
        lx = fminf(lx, p.x - ex), hx = fmaxf(hx, p.x + ex);
        ly = fminf(ly, p.y - ey), hy = fmaxf(hy, p.y + ey);
        lz = fminf(lz, p.z - ez), hz = fmaxf(hz, p.z + ez);
    }
    /* (finite, ordered bounds only: anything else keeps the box as uploaded) */
    if (!(lx <= hx && ly <= hy && lz <= hz && fabsf(lx) < 3.0e38f && fabsf(hx) < 3.0e38f && fabsf(ly) < 3.0e38f && fabsf(hy) < 3.0e38f &&
          fabsf(lz) < 3.0e38f && fabsf(hz) < 3.0e38f))
        return false;
    const float nlx = fmaxf(lo[0], lx), nly = fmaxf(lo[1], ly), nlz = fmaxf(lo[2], lz);
    const float nhx = fminf(hi[0], hx), nhy = fminf(hi[1], hy), nhz = fminf(hi[2], hz);
    if (!(nlx <= nhx && nly <= nhy && nlz <= nhz))
        return false;
    lo[0] = nlx, lo[1] = nly, lo[2] = nlz;
    hi[0] = nhx, hi[1] = nhy, hi[2] = nhz;
    return true;
}
} // namespace solreng

#endif
