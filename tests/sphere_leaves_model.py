"""The thin copy of a node list with the clause for leaves of spheres (test infrastructure, no test functions): the model of
tests/list_copies_model.py, which stays as it is, with sol-r_amd/csrc/build_bounds.h's sphere clause added in numpy's
binary32, operation for operation - sphereBuildExtent and the part of leafBuildBounds that calls it.  A leaf that holds
nothing but KIND_SPHERE records becomes the union of p0 -+ extent of its spheres, cut with its box as uploaded; anything
not finite or not ordered keeps that box; a leaf that mixes spheres and planes keeps it too.  reach == 0 is the model of
list_copies_model.py itself (solr_hip_set_variant(18)).

Also here: what the engine takes for the reach (solr_arena.hip thinReachWanted), and which leaves of spheres are `loose` -
boxed larger than their spheres (solr_uploads.hip retagPrimitives) - the fact that makes a copy worth making where a scene
has no plain plane."""
import numpy as np

import list_copies_model as M

f4, i4 = np.float32, np.int32
KIND_SPHERE = 1
PLANES = (M.KIND_PLANE_XY, M.KIND_PLANE_YZ, M.KIND_PLANE_XZ)


def sphere_kinds(prims, materials):
    """per primitive: KIND_SPHERE for a ptSphere whose material has no fast transparency (attributes.x == 0) and is not
    procedural (attributes.y == 0), whatever else it is - emissive like a lamp's, transparent; 0 for everything else"""
    out = np.zeros(len(prims), i4)
    for i, p in enumerate(prims):
        m = materials[int(p["materialId"])]
        if (int(p["type"]) & 0xff) == M.ptSphere and int(m["attributes"][0]) == 0 and int(m["attributes"][1]) == 0:
            out[i] = KIND_SPHERE
    return out


def kinds(prims, materials):
    """the kinds the thin copy goes by: plain planes and spheres"""
    return M.plain_kinds(prims, materials) + sphere_kinds(prims, materials)


def reach_of(scene_extent, view_distance=0.0):
    """the reach the engine makes the thin boxes of sphere leaves for: the frame's viewDistance where that lies beyond the
    scene's extent, else the extent"""
    return f4(view_distance) if f4(view_distance) > f4(scene_extent) else f4(scene_extent)


def sphere_extent(p0, radius, margin, reach):
    """sphereBuildExtent: ((|r| + margin) + (3 far 2^-21) / (|r| / far)) + far 2^-9, far = reach + max |p0|"""
    with np.errstate(all="ignore"):
        r = np.abs(f4(radius))
        a = [np.abs(f4(c)) for c in p0]
        far = f4(f4(reach) + M.fmax(M.fmax(a[0], a[1]), a[2]))
        slack = f4(f4(f4(f4(3.0) * far) * f4(2.0 ** -21)) / f4(r / far))
        return f4(f4(f4(r + f4(margin)) + slack) + f4(far * f4(2.0 ** -9)))


def thin_leaves(rows, start, records, kinds_, margin, reach):
    """M.thin_leaves with the clause for leaves of nothing but spheres (reach > 0)"""
    out = M.thin_leaves(rows, start, records, np.where(np.isin(kinds_, PLANES), kinds_, 0), margin)
    if not f4(reach) > 0:
        return out
    cnt = M.counts(rows)
    for i in range(len(rows)):
        nb = int(cnt[i])
        if nb <= 0 or int(start[i]) < 0:
            continue
        mine = range(int(start[i]), int(start[i]) + nb)
        if not all(kinds_[k] == KIND_SPHERE for k in mine):
            continue
        l, h = [f4(np.inf)] * 3, [f4(-np.inf)] * 3
        finite = True
        with np.errstate(all="ignore"):
            for k in mine:
                p0 = records[k, M.ROW_P0_TYPE, :3]
                e = sphere_extent(p0, records[k, M.ROW_SIZE_MAT, 0], margin, reach)
                if not (e < M.BIG and all(np.abs(f4(c)) < M.BIG for c in p0)):
                    finite = False
                    break
                l = [M.fmin(l[a], f4(f4(p0[a]) - e)) for a in range(3)]
                h = [M.fmax(h[a], f4(f4(p0[a]) + e)) for a in range(3)]
        if not finite or not M._ordered_and_finite(l, h):
            continue
        cut = M._cut(rows[i], l, h)
        if cut is not None:
            out[i] = M._with_bounds(rows[i], *cut)
    return out


def thin_copy(rows, start, records, kinds_, margin, reach, list_length=None):
    return M.thin_inner(thin_leaves(rows, start, records, kinds_, margin, reach), list_length or len(rows))


def loose_sphere_leaves(rows, start, records, kinds_):
    """the leaves of nothing but spheres whose box reaches beyond the union of p0 -+ |r| (retagPrimitives: looseSpheres)"""
    found = []
    cnt = M.counts(rows)
    for i in range(len(rows)):
        nb = int(cnt[i])
        if nb <= 0:
            continue
        mine = list(range(int(start[i]), int(start[i]) + nb))
        if not all(kinds_[k] == KIND_SPHERE for k in mine):
            continue
        with np.errstate(all="ignore"):
            p = records[mine, M.ROW_P0_TYPE, :3]
            r = np.abs(records[mine, M.ROW_SIZE_MAT, 0])[:, None]
            l, h = (p - r).astype(f4).min(axis=0), (p + r).astype(f4).max(axis=0)
            if (M.lo(rows)[i] < l).any() or (M.hi(rows)[i] > h).any():
                found.append(i)
    return found


# ---- hand-made lists with leaves of spheres boxed larger than their spheres ----------------------------------------------
def light_cell(solr, view_distance=50000.0, lamps=1, extra=None):
    """M.panels with the lamp's leaf - the last node - boxed +-viewDistance as the reference's builder boxes the lamps' cell
    (GPUKernel.cpp:1189), the root grown to hold it; lamps == 2: a second lamp in the same leaf.  extra: [(name, [(p0,
    radius)], box or None)] more leaves of spheres, in front of the lamps' (box None: the builder's own p0 -+ r)."""
    scene = M.panels(solr)
    P, B = solr.PRIMITIVE_DTYPE, solr.BOX_DTYPE
    boxes, prims = list(scene.boxes[:-1]), list(scene.prims[:-1])
    names = dict(scene.names)
    for name, spheres, box in extra or []:
        members = [M._prim(P, M.ptSphere, p0, (radius, 0, 0), M.PLAIN) for p0, radius in spheres]
        l, h = M._box_of(members) if box is None else box
        b = np.zeros(1, B)[0]
        b["min"], b["max"], b["nbPrimitives"], b["startIndex"], b["indexForNextBox"] = l, h, len(members), len(prims), (1, 0)
        names[name] = len(boxes)
        boxes.append(b)
        for p in members:
            p["index"] = len(prims)
            prims.append(p)
    cell = [scene.prims[-1].copy()]
    if lamps == 2:
        cell.append(M._prim(P, M.ptSphere, (-3000.0, 7000.0, 1000.0), (25.0, 0, 0), M.LAMP))
    b = np.zeros(1, B)[0]
    b["min"], b["max"] = [-view_distance] * 3, [view_distance] * 3
    b["nbPrimitives"], b["startIndex"], b["indexForNextBox"] = len(cell), len(prims), (1, 0)
    names["lamp"] = len(boxes)
    boxes.append(b)
    first_lamp = len(prims)
    for p in cell:
        p["index"] = len(prims)
        prims.append(p)
    boxes = np.array(boxes, B)
    boxes["min"][0], boxes["max"][0] = [-view_distance] * 3, [view_distance] * 3
    boxes["indexForNextBox"][0] = (len(boxes), 0)
    return M.HandMade(boxes, np.array(prims, P), names, first_lamp)
