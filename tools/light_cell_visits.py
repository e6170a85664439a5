#!/usr/bin/env python3
"""How many LEAVES does a wave of primary rays enter on the order-free lists, and what does the lamps' cell cost it?  The
visit model of tools/free_list_visits.py (imported, not changed: the same rays, tiles, slab test and cursor) with two
counts more - leaves a wave enters (any lane's slab test passes at a leaf) and leaf entries per lane - over host-built lists
(tests/free_list_topology_check.cpp --dump, no GPU) and their thin copy by tests/sphere_leaves_model.py, with the clause
for leaves of spheres (sol-r_amd/csrc/build_bounds.h) and without it (reach 0: solr_hip_set_variant(18)).  No distance
cut-off, as there: an upper bound, the same on both sides.

    python tools/light_cell_visits.py --host CHECKER [--scene cornell|room200] [--width 1920 --height 1080]

CHECKER: the program tests/free_list_topology_check.cpp compiles to (with list_builders.cpp; its header says how).
profiles/r16/light_cell.txt has the counts."""
import argparse
import importlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import free_list_visits as V  # noqa: E402

f4, i4 = np.float32, np.int32


def host_lists(solr, args):
    """the eight lists of the host builders, their start indices, the records and kinds the thin copies go by, the margin
    and the reach, the camera"""
    import list_copies_model as M
    import sphere_leaves_model as S
    k = solr.Kernel(engine="host-only")
    V.make_scene(solr, k, args.scene, args.width, args.height)
    flat = k.flat_scene()
    boxes, prims, materials = flat.boxes.copy(), flat.primitives.copy(), flat.materials.copy()
    si, pp, eye, target, ang = k.frame_parameters()
    view = float(si.viewDistance)
    k.finalize()
    rows = M.rows_of(boxes)
    kinds = S.kinds(prims, materials)
    records = M.records_of(prims, kinds)
    extent = M.extent(prims)
    with tempfile.TemporaryDirectory() as tmp:
        path, out = os.path.join(tmp, "scene.bin"), os.path.join(tmp, "lists.bin")
        with open(path, "wb") as f:
            np.array([len(boxes), len(prims)], i4).tofile(f)
            rows.tofile(f)
            np.ascontiguousarray(boxes["startIndex"], i4).tofile(f)
            by_type = records.copy()
            by_type[:, 0, 3] = (prims["type"].astype(i4) & 0xff).view(f4)
            by_type.tofile(f)
        run = subprocess.run([args.host, path, "--dump", out, "--share", "0.25"], capture_output=True, text=True)
        if run.returncode != 0:
            sys.stdout.write(run.stdout + run.stderr)
        raw = np.fromfile(out, i4)
    nb = int(raw[0])
    lists = raw[1:1 + 8 * nb * 8].view(f4).reshape(8 * nb, 2, 4)
    start = raw[1 + 8 * nb * 8:1 + 8 * nb * 9]
    return lists, start, nb, records, kinds, M.margin_of(extent), S.reach_of(extent, view), eye, target, float(ang[3])


def visits(thin, nb, origin, d, inside):
    """per tile: nodes visited, leaves the wave enters, leaf entries summed over its lanes (V.visits with two counts more)"""
    tiles = d.shape[0]
    first = inside.argmax(axis=1)
    d0 = d[np.arange(tiles), first]
    octant = (d0[:, 0] < 0).astype(i4) | ((d0[:, 1] < 0).astype(i4) << 1) | ((d0[:, 2] < 0).astype(i4) << 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (f4(1.0) / d).astype(f4)
    cursor = np.zeros(tiles, i4)
    visited, leaves, lanes = np.zeros(tiles, i4), np.zeros(tiles, i4), np.zeros(tiles, i4)
    lo = np.stack([thin[:, 0, 0], thin[:, 0, 1], thin[:, 0, 2]], axis=1).reshape(8, nb, 3)
    hi = np.stack([thin[:, 1, 0], thin[:, 1, 1], thin[:, 0, 3]], axis=1).reshape(8, nb, 3)
    count = thin[:, 1, 2].view(i4).reshape(8, nb)
    skip = np.maximum(thin[:, 1, 3].view(i4).reshape(8, nb), 1)
    o = np.asarray(origin, f4)
    for i in range(nb):
        here = np.nonzero(cursor == i)[0]
        if len(here) == 0:
            continue
        visited[here] += 1
        oc = octant[here]
        leaf = count[oc, i] > 0
        with np.errstate(invalid="ignore"):
            a = ((lo[oc, i][:, None, :] - o) * inv[here]).astype(f4)
            b = ((hi[oc, i][:, None, :] - o) * inv[here]).astype(f4)
        tnear = np.fmin(a, b).max(axis=2)
        tfar = np.fmax(a, b).min(axis=2)
        passes = (tnear <= tfar) & (tfar > 0) & inside[here]
        enters = passes.any(axis=1)
        leaves[here] += (leaf & enters).astype(i4)
        lanes[here] += np.where(leaf, passes.sum(axis=1), 0).astype(i4)
        cursor[here] = np.where(leaf | enters, i + 1, i + skip[oc, i])
    return visited, leaves, lanes


def main():
    import sphere_leaves_model as S
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="cornell")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--host", required=True, help="the compiled tests/free_list_topology_check.cpp")
    args = ap.parse_args()
    solr = importlib.import_module("sol-r_amd")
    lists, start, nb, records, kinds, margin, reach, eye, target, aw = host_lists(solr, args)
    origin, dirs = V.primary_rays((args.width, args.height), eye, target, aw)
    d, inside, shape = V.tiles_of(dirs)
    rays = int(inside.sum())
    print("%s %dx%d: 8 host-built lists of %d nodes; %d tiles, %d primary rays; margin %.2f, reach %.0f"
          % (args.scene, args.width, args.height, nb, d.shape[0], rays, margin, reach))
    kept = {}
    for label, r in (("sphere leaves as uploaded (variant 18)", 0.0), ("sphere leaves by their spheres", reach)):
        thin = S.thin_copy(lists, start, records, kinds, margin, r, list_length=nb)
        visited, leaves, lanes = visits(thin, nb, origin, d, inside)
        kept[label] = (visited, leaves, lanes)
        print("  %-40s nodes visited per walk %.3f, leaves entered per walk %.3f, leaf entries per ray %.3f  (totals %d, %d, %d)"
              % (label + ":", visited.mean(), leaves.mean(), lanes.sum() / rays, visited.sum(), leaves.sum(), lanes.sum()))
    (v0, l0, n0), (v1, l1, n1) = kept.values()
    print("  difference: %.3f leaves per walk, %.3f leaf entries per ray, %.3f nodes visited per walk; waves that enter as many "
          "leaves as before: %d of %d"
          % ((l0 - l1).mean(), (n0 - n1).sum() / rays, (v0 - v1).mean(), int((l0 == l1).sum()), len(l0)))


if __name__ == "__main__":
    main()
