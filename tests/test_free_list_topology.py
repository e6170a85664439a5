"""The order-free lists built on build bounds (sol-r_amd/csrc/build_bounds.h: a leaf of axis-plane rectangles by its thin
box, dominant leaves set apart) against the same lists built on the boxes as uploaded, on the CPU:
tests/free_list_topology_check.cpp links the host builders and nothing else and is run as a program of its own on
  - the Cornell room: six rectangles and 23 spheres;
  - `panels`, the hand-made list of tests/list_copies_model.py;
  - the Cornell spheres without a room: no axis-plane leaf;
  - a room two of whose walls share a leaf with a sphere.
It exits non-zero unless, with build bounds, every one of the eight lists has the leaves, start indices and origins it has
without, nested skip pointers, inner rows that are the unions of their leaves' uploaded boxes bit for bit, and - in the
two rooms, whose walls dominate; the small panels of `panels` stay in the hierarchy - every leaf of nothing but
rectangles at depth <= 1 (the conditions are spelled out in the program).  Here: without build bounds the
lists are the ones the builder made before build bounds existed (FNV-1a hashes recorded from that builder), a scene
without an axis-plane leaf gets those with build bounds as well, and in the Cornell room a fixed grid of beams visits
strictly fewer nodes than on the fat topology."""
import os
import subprocess

import numpy as np
import pytest

import list_copies_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "sol-r_amd", "csrc")
f4, i4 = np.float32, np.int32


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("free_list_topology") / "free_list_topology_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", exe,
                    os.path.join(HERE, "free_list_topology_check.cpp"), os.path.join(CSRC, "list_builders.cpp")], check=True)
    return exe


def _cornell(solr, room):
    k = solr.Kernel(engine="host-only")
    solr.scenes.cornell(k, width=64, height=48, iterations=1, room=room)
    flat = k.flat_scene()
    boxes, prims = flat.boxes.copy(), flat.primitives.copy()
    k.finalize()
    return boxes, prims


def _shared_leaf_room(solr):
    """the Cornell room's walls and 23 spheres under one root, a leaf each - but two walls share theirs with a sphere"""
    P, B = solr.PRIMITIVE_DTYPE, solr.BOX_DTYPE
    rng = np.random.default_rng(11)
    c, h = (0.0, 15000.0, 0.0), 20000.0
    walls = [M._prim(P, t, (c[0] + dx * h, c[1] + dy * h, c[2] + dz * h), (h, h, h), M.PLAIN)
             for t, dx, dy, dz in ((M.ptXYPlane, 0, 0, 1), (M.ptXYPlane, 0, 0, -1), (M.ptYZPlane, -1, 0, 0),
                                   (M.ptYZPlane, 1, 0, 0), (M.ptXZPlane, 0, 1, 0), (M.ptXZPlane, 0, -1, 0))]
    spheres = [M._prim(P, M.ptSphere, rng.uniform(-9000, 9000, 3).round(), (float(rng.integers(300, 2000)), 0, 0), M.PLAIN)
               for _ in range(23)]
    leaves = [[walls[0], spheres[0]], [spheres[1], walls[1]]] + [[w] for w in walls[2:]] + [[s] for s in spheres[2:]]
    rows, prims = [np.zeros(1, B)[0]], []
    for members in leaves:
        b = np.zeros(1, B)[0]
        b["min"], b["max"] = M._box_of(members)
        b["nbPrimitives"], b["startIndex"], b["indexForNextBox"] = len(members), len(prims), (1, 0)
        rows.append(b)
        for p in members:
            p["index"] = len(prims)
            prims.append(p)
    rows[0]["min"] = np.min([r["min"] for r in rows[1:]], axis=0)
    rows[0]["max"] = np.max([r["max"] for r in rows[1:]], axis=0)
    rows[0]["indexForNextBox"] = (len(rows), 0)
    return np.array(rows, B), np.array(prims, P)


def _panels(solr):
    scene = M.panels(solr)
    return scene.boxes, scene.prims


SCENES = {"cornell": lambda solr: _cornell(solr, True), "panels": _panels,
          "spheres-only": lambda solr: _cornell(solr, False), "shared-leaf": _shared_leaf_room}

ROOMS = ("cornell", "shared-leaf")

# what buildFreeOrderLists made of these scenes before build bounds existed (the checker's `fat` line, from that builder)
UNTOUCHED = {"cornell": "8d0ba647b0b0ffb6", "panels": "bc17b78d583e887e", "spheres-only": "4d1449572264a1be", "shared-leaf": "776c4aa87411f182"}


def _scene_file(boxes, prims, path):
    records = M.records_of(prims, np.zeros(len(prims), i4))     # (the type alone in the tag: materials come later)
    with open(path, "wb") as f:
        np.array([len(boxes), len(prims)], i4).tofile(f)
        M.rows_of(boxes).tofile(f)
        np.ascontiguousarray(boxes["startIndex"], i4).tofile(f)
        records.tofile(f)


@pytest.fixture(scope="module")
def verdicts(solr, checker, tmp_path_factory):
    """the checker's word on every scene, once"""
    out = {}
    tmp = tmp_path_factory.mktemp("free_list_scenes")
    for name, make in SCENES.items():
        path = str(tmp / (name + ".bin"))
        _scene_file(*make(solr), path)
        run = subprocess.run([checker, path] + (["--walls-at-top"] if name in ROOMS else []), capture_output=True, text=True)
        print(name, run.stdout, run.stderr)
        out[name] = (run, dict(line.split(None, 1) for line in run.stdout.splitlines() if " " in line))
    return out


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_lists_on_build_bounds_hold_the_same_leaves_under_unions_of_uploaded_boxes(verdicts, scene):
    run, said = verdicts[scene]
    assert run.returncode == 0, run.stdout + run.stderr
    if scene != "spheres-only":
        assert int(said["walls"]) > 0
    if scene in ROOMS:
        assert int(said["depth"]) <= 1


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_without_build_bounds_the_lists_are_the_untouched_builders(verdicts, scene):
    run, said = verdicts[scene]
    assert said["fat"] == UNTOUCHED[scene], said


def test_a_scene_without_axis_plane_leaves_gets_the_untouched_lists_with_build_bounds_too(verdicts):
    run, said = verdicts["spheres-only"]
    assert int(said["walls"]) == 0
    assert said["built"] == said["fat"] == UNTOUCHED["spheres-only"], said


def test_beams_through_the_room_visit_strictly_fewer_nodes_than_on_the_fat_topology(verdicts):
    run, said = verdicts["cornell"]
    fat, built = (int(v) for v in said["visits"].split())
    print("node visits over the grid of beams: %d on the fat topology, %d on build bounds" % (fat, built))
    assert built < fat
