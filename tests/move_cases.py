"""Scenes and binary32 models for the tests of the rigid moves besides the rotation (tests/test_moves_host.py,
tests/test_moves_gpu.py): GPUKernel::translatePrimitives and a lamp's setPrimitiveCenter, on the host and on the resident
scene (solr_hip_translate_primitives, solr_hip_move_lamp).

  two_lamps          the sticks of tests/morph_cases.py (first key frame, one frame only) with a second lamp: slot 1 exists
  plane_lamp         spheres over a floor, lit by an emissive XZ plane alone: the lamps' leaf has a thin copy made from its p0
  translation_model  what translatePrimitives leaves of the flattened primitives
  refit_model        what the box updates behind it leave of the flattened boxes: updateBoundingBox and
                     updateOutterBoundingBox (GPUKernel.cpp:741-839 of the reference) restated over the flattened arrays,
                     every comparison as written there - the sign of a zero that ties depends on their order

The other scenes are morph_cases' (mesh, sticks, mix), imported unchanged."""
import importlib

import numpy as np

import morph_cases

solr = importlib.import_module("sol-r_amd")

f32 = np.float32
SECOND_LAMP = (6000.0, 4000.0, -9000.0)


def two_lamps(k):
    """the sticks with a second lamp, in kernel k, flattened; returns the primitive indices of the two lamps by slot"""
    k.initialize(width=morph_cases.WIDTH, height=morph_cases.HEIGHT, nbRayIterations=2)
    m = morph_cases._materials(k, "sticks")
    morph_cases._sticks(k, m, 0)
    morph_cases._lamp(k, m, SECOND_LAMP)
    k.compact_boxes(True)
    k.set_camera((0.0, 0.0, -14000.0))
    return k


def plane_lamp(k):
    """a ring of spheres and a floor under an emissive XZ plane, the only lamp, in kernel k, flattened"""
    k.initialize(width=morph_cases.WIDTH, height=morph_cases.HEIGHT, nbRayIterations=2)
    m = morph_cases._materials(k, "sticks")
    for a in range(12):
        k.add_primitive(solr.ptSphere, (3500.0 * np.cos(0.5 * a), -2500.0 + 300.0 * a, 3500.0 * np.sin(0.5 * a)),
                        size=(400.0 + 25.0 * (a % 5), 0, 0), material=m["walls"][a % 6])
    k.add_primitive(solr.ptXZPlane, (0.0, -4500.0, 0.0), size=(7000.0, 0.0, 7000.0), material=m["walls"][0])
    k.add_primitive(solr.ptXZPlane, (0.0, 7500.0, -2000.0), size=(1500.0, 0.0, 1500.0), material=m["lamp"])
    k.compact_boxes(True)
    k.set_camera((0.0, 0.0, -14000.0))
    return k


def build(k, name):
    if name == "plane_lamp":
        return plane_lamp(k)
    return two_lamps(k) if name == "two_lamps" else morph_cases.build(k, name)


def lamp_indices(k):
    """the primitive index of every lamp slot (SolR_GetLight)"""
    out = []
    while k.L.SolR_GetLight(len(out)) >= 0:
        out.append(k.L.SolR_GetLight(len(out)))
    return out


def moved_by_a_translation(flat, unmovable=()):
    """per flattened primitive: does GPUKernel::translatePrimitives move it - it sits in a level-0 box (the lamps, first in
    the flattened order, sit in the top level's first box), is movable (`unmovable`: the indices that are not) and is not
    the camera primitive"""
    p = flat.primitives
    return (np.arange(len(p)) >= flat.nb_lamps) & ~np.isin(p["index"], list(unmovable)) & (p["type"] != solr.ptCamera)


def translation_model(primitives, moved, t):
    """GPUKernel::translatePrimitives on flattened primitives: p0, p1 and p2 of the moved ones incremented by t, one
    binary32 addition a coordinate; nothing else changes"""
    t = np.asarray(t, f32)
    out = primitives.copy()
    for field in ("p0", "p1", "p2"):
        v = out[field].astype(f32)
        v[moved] = (v[moved] + t).astype(f32)
        out[field] = v
    return out


def _std_min(a, b):
    return b if b < a else a


def _std_max(a, b):
    return b if a < b else a


def _leaf_bounds(prims):
    """updateBoundingBox over the primitives of a level-0 box, in their order"""
    lo = [f32(1000000.0)] * 3
    hi = [f32(-1000000.0)] * 3
    for p in prims:
        kind = int(p["type"])
        p0, p1, p2, size = ([f32(c) for c in p[field]] for field in ("p0", "p1", "p2", "size"))
        if kind == solr.ptTriangle:
            c0 = [_std_min(_std_min(p0[a], p1[a]), p2[a]) for a in range(3)]
            c1 = [_std_max(_std_max(p0[a], p1[a]), p2[a]) for a in range(3)]
        elif kind == solr.ptCylinder:
            c0 = [_std_min(p0[a], p1[a]) for a in range(3)]
            c1 = [_std_max(p0[a], p1[a]) for a in range(3)]
        else:
            c0, c1 = list(p0), list(p0)
        a0 = [_std_min(c0[a], c1[a]) for a in range(3)]
        a1 = [c0[a] if c0[a] > c1[a] else c1[a] for a in range(3)]
        grow = [size[0]] * 3 if kind in (solr.ptCylinder, solr.ptSphere, solr.ptCone) else size
        for a in range(3):
            low, high = f32(a0[a] - grow[a]), f32(a1[a] + grow[a])
            if low < lo[a]:
                lo[a] = low
            if high > hi[a]:
                hi[a] = high
    return lo, hi


def refit_model(boxes, primitives, view_distance):
    """the flattened boxes after GPUKernel::refitBoxes on those primitives and a flattening: a node with primitives is a
    level-0 box (updateBoundingBox), one without is the union of its children (updateOutterBoundingBox, seeded with
    +-viewDistance), children first; node 0, the lamps' cell, is pinned to +-viewDistance by the flattening itself
    (GPUKernel.cpp:1183-1188)"""
    vd = f32(view_distance)
    out = boxes.copy()
    n = len(out)
    count, start, skip = out["nbPrimitives"], out["startIndex"], out["indexForNextBox"][:, 0]
    lo = np.zeros((n, 3), f32)
    hi = np.zeros((n, 3), f32)
    for i in range(n - 1, -1, -1):
        if i == 0:
            lo[i], hi[i] = [-vd] * 3, [vd] * 3
        elif count[i] > 0:
            lo[i], hi[i] = _leaf_bounds(primitives[start[i]:start[i] + count[i]])
        else:
            l, h = [vd] * 3, [-vd] * 3
            c = i + 1
            while c < i + skip[i]:
                for a in range(3):
                    if l[a] > lo[c][a]:
                        l[a] = lo[c][a]
                    if h[a] < hi[c][a]:
                        h[a] = hi[c][a]
                c += max(int(skip[c]), 1)
            lo[i], hi[i] = l, h
    out["min"], out["max"] = lo, hi
    return out
