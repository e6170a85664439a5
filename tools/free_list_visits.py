#!/usr/bin/env python3
"""How many nodes of the order-free lists does a wave of primary rays visit?  A numpy model of the wave-synchronous
walk (rt_device.h, the node loop): a node is visited when the wave's cursor reaches it, its children when ANY lane's
slab test passes - (b - o) * (1 / d) per axis in binary32, entered if tnear <= tfar and tfar > 0.  No distance
cut-off: an upper bound, the same for every list it is run on.  The rays are the primary rays of a frame as
renderer_kernel.h makes them from frame_parameters() (perspective camera, no rotation), in 8 x 8 tiles, each tile on
the list of its first lane's octant.

    python tools/free_list_visits.py --scene cornell --width 1920 --height 1080            the engine's lists (GPU)
    python tools/free_list_visits.py --scene cornell --host CHECKER [--share 0.25 | --fat]  host-built lists (no GPU)

--host: the program tests/free_list_topology_check.cpp compiles to (with list_builders.cpp); it builds the lists of the
host-only engine's scene on the CPU, the thin copy is tests/list_copies_model.py's.  --variant N: solr_hip_set_variant
before the scene is uploaded.  Scenes: cornell, panels, room200 (the Cornell room with 200 small spheres)."""
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
f4, i4 = np.float32, np.int32


def primary_rays(si_size, eye, target, aw):
    """origin (3,), directions (H, W, 3): renderer_kernel.h's perspective camera with angles (0, 0, 0, aw); the walks take
    target - origin"""
    w, h = si_size
    stepx = f4(f4(f4(w) / f4(h)) * f4(aw)) / f4(w)
    stepy = f4(aw) / f4(h)
    x = np.arange(w, dtype=i4) - i4(w // 2)
    y = np.arange(h, dtype=i4) - i4(h // 2)
    d = np.zeros((h, w, 3), f4)
    d[..., 0] = (f4(target[0]) - stepx * x.astype(f4))[None, :]
    d[..., 1] = (f4(target[1]) + stepy * y.astype(f4))[:, None]
    d[..., 2] = f4(target[2])
    return np.asarray(eye, f4), (d - np.asarray(eye, f4)).astype(f4)


def tiles_of(dirs):
    """(tiles, 64, 3) directions, (tiles, 64) which lanes lie in the frame; 8 x 8 tiles, ragged edges padded"""
    h, w, _ = dirs.shape
    th, tw = (h + 7) // 8, (w + 7) // 8
    padded = np.zeros((th * 8, tw * 8, 3), f4)
    inside = np.zeros((th * 8, tw * 8), bool)
    padded[:h, :w], inside[:h, :w] = dirs, True
    d = padded.reshape(th, 8, tw, 8, 3).transpose(0, 2, 1, 3, 4).reshape(th * tw, 64, 3)
    m = inside.reshape(th, 8, tw, 8).transpose(0, 2, 1, 3).reshape(th * tw, 64)
    return d, m, (th, tw)


def visits(thin, nb, origin, d, inside):
    """nodes visited per tile.  thin: (8 nb, 2, 4) rows of the eight lists' thin copies"""
    tiles = d.shape[0]
    first = inside.argmax(axis=1)
    d0 = d[np.arange(tiles), first]
    octant = (d0[:, 0] < 0).astype(i4) | ((d0[:, 1] < 0).astype(i4) << 1) | ((d0[:, 2] < 0).astype(i4) << 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (f4(1.0) / d).astype(f4)
    cursor = np.zeros(tiles, i4)
    visited = np.zeros(tiles, i4)
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
        enters = ((tnear <= tfar) & (tfar > 0) & inside[here]).any(axis=1)
        cursor[here] = np.where(leaf | enters, i + 1, i + skip[oc, i])
    return visited


def report(name, per_tile, shape):
    print("%s: %d tiles (%d x %d), nodes visited per primary walk: mean %.2f, min %d, max %d" %
          (name, per_tile.size, shape[1], shape[0], per_tile.mean(), per_tile.min(), per_tile.max()))
    top = int(per_tile.max())
    edges = sorted(set([0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 64, 96, 128, 256, top + 1]))
    edges = [e for e in edges if e <= top + 1]
    hist, _ = np.histogram(per_tile, bins=edges)
    print("  histogram over tiles: " + "  ".join("[%d,%d): %d" % (edges[k], edges[k + 1], hist[k]) for k in range(len(hist)) if hist[k]))
    print("  total node visits: %d" % int(per_tile.sum()))


def make_scene(solr, k, name, width, height):
    if name == "cornell":
        solr.scenes.cornell(k, width=width, height=height, iterations=3)
    elif name == "room200":
        solr.scenes.cornell(k, width=width, height=height, iterations=3, extra_spheres=200)
    else:
        raise SystemExit("unknown scene %s (panels: with --host only)" % name)


def host_lists(solr, args):
    """the lists of the host builders (tests/free_list_topology_check.cpp --dump) and their thin copy by the model"""
    import list_copies_model as M
    if args.scene == "panels":
        scene = M.panels(solr, opaque=True)
        boxes, prims = scene.boxes, scene.prims
        materials = M.hand_made_materials(solr.MATERIAL_DTYPE)
        eye, target, aw = np.array([0, 0, -15000], f4), np.zeros(3, f4), 6400.0
    else:
        k = solr.Kernel(engine="host-only")
        make_scene(solr, k, args.scene, args.width, args.height)
        flat = k.flat_scene()
        boxes, prims, materials = flat.boxes.copy(), flat.primitives.copy(), flat.materials.copy()
        si, pp, eye, target, ang = k.frame_parameters()
        aw = float(ang[3])
        k.finalize()
    rows = M.rows_of(boxes)
    kinds = M.plain_kinds(prims, materials)
    records = M.records_of(prims, kinds)
    margin = M.margin_of(M.extent(prims))
    with tempfile.TemporaryDirectory() as tmp:
        path, out = os.path.join(tmp, "scene.bin"), os.path.join(tmp, "lists.bin")
        with open(path, "wb") as f:
            np.array([len(boxes), len(prims)], i4).tofile(f)
            rows.tofile(f)
            np.ascontiguousarray(boxes["startIndex"], i4).tofile(f)
            records_plain = records.copy()
            records_plain[:, 0, 3] = (prims["type"].astype(i4) & 0xff).view(f4)
            records_plain.tofile(f)
        cmd = [args.host, path, "--dump", out] + (["--fat"] if args.fat else ["--share", str(args.share)])
        run = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write("  " + run.stdout.replace("\n", "\n  ").rstrip() + "\n")
        if run.returncode != 0:
            sys.stdout.write(run.stderr)
        raw = np.fromfile(out, i4)
    nb = int(raw[0])
    lists = raw[1:1 + 8 * nb * 8].view(f4).reshape(8 * nb, 2, 4)
    start = raw[1 + 8 * nb * 8:1 + 8 * nb * 9]
    thin = M.thin_copy(lists, start, records, kinds, margin, list_length=nb)
    return thin, nb, eye, target, aw


def engine_lists(solr, args):
    """the thin copy of the resident scene's order-free lists, read back from the engine"""
    import engine_probes as P
    hip = solr.hip_lib()
    P.declare(hip)
    if args.variant:
        hip.solr_hip_set_variant(args.variant)
    k = solr.Kernel(engine="hip")
    make_scene(solr, k, args.scene, args.width, args.height)
    for _ in range(3):      # (the lists are built once the scene has been rendered)
        k.render()
    thin = P.list_copy(hip, 2, 1)
    nb = len(thin) // 8
    si, pp, eye, target, ang = k.frame_parameters()
    k.finalize()
    return np.ascontiguousarray(thin, f4).reshape(8 * nb, 2, 4), nb, eye, target, float(ang[3])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="cornell")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--host", help="the compiled tests/free_list_topology_check.cpp: host-built lists, no GPU")
    ap.add_argument("--share", type=float, default=0.25)
    ap.add_argument("--fat", action="store_true", help="with --host: the lists built on the boxes as uploaded")
    ap.add_argument("--variant", type=int, default=0)
    args = ap.parse_args()
    solr = importlib.import_module("sol-r_amd")
    thin, nb, eye, target, aw = host_lists(solr, args) if args.host else engine_lists(solr, args)
    leaves = int((thin[:nb, 1, 2].view(i4) > 0).sum())
    print("%s %dx%d: 8 lists of %d nodes, %d leaves" % (args.scene, args.width, args.height, nb, leaves))
    origin, dirs = primary_rays((args.width, args.height), eye, target, aw)
    d, inside, shape = tiles_of(dirs)
    what = ("host-built, " + ("uploaded boxes" if args.fat else "build bounds, share %g" % args.share)) if args.host else \
        "engine" + (", variant %d" % args.variant if args.variant else "")
    report(what, visits(thin, nb, origin, d, inside), shape)


if __name__ == "__main__":
    main()
