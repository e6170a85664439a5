"""The host builders of the node lists (sol-r_amd/csrc/list_builders.cpp) on the CPU: tests/list_builders_check.cpp links
them and nothing else, is compiled under the address and undefined-behaviour sanitizers and run as a program of its own
on scenes from the host-only engine.  It builds the walk-order list, the eight order-free lists and the refit plan with
the default parameters and exits non-zero unless they are what the walks and the refit kernels rely on: nested skip
pointers, the reference's nodes in the reference's order and bit for bit, every leaf once, grouping nodes that are the
unions of their children, inner nodes of the order-free lists that enclose theirs, lists 0 and 7 in different orders,
refit levels with every node once and children first (the conditions are spelled out in the program).  The same program
runs the builders on the synthetic node lists of tests/list_builder_cases.py, written in its scene-file format: lists whose
leaves coincide, tie, lie on bin edges or a denormal apart are where a host builder reads past a range or converts what it
should not, and the sanitizers say so."""
import os
import subprocess

import numpy as np
import pytest

import list_builder_cases as K
import test_lists_gpu as G

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "sol-r_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("list_builders") / "list_builders_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", exe,
                    os.path.join(HERE, "list_builders_check.cpp"), os.path.join(CSRC, "list_builders.cpp")], check=True)
    return exe


def _twins(solr, k):
    G.k_solr = solr
    G._twins(k, triples=60)


SCENES = {"cornell": lambda solr, k: solr.scenes.cornell(k, width=64, height=48, iterations=1),
          "molecule-300": lambda solr, k: solr.scenes.molecule(k, atoms=300, width=64, height=48),
          "twins-60": _twins}


def _bits(a):
    return np.ascontiguousarray(a, np.int32).view(np.float32)


def _scene_file(flat, path):
    """the node rows, start indices and primitive rows h2d_scene makes of the flattened arrays (scene_layout.h)"""
    b, p = flat.boxes, flat.primitives
    rows = np.zeros((len(b), 2, 4), np.float32)
    rows[:, 0, :3] = b["min"]
    rows[:, 0, 3] = b["max"][:, 2]
    rows[:, 1, :2] = b["max"][:, :2]
    rows[:, 1, 2] = _bits(b["nbPrimitives"])
    rows[:, 1, 3] = _bits(b["indexForNextBox"][:, 0])
    prims = np.zeros((len(p), 8, 4), np.float32)
    for row, (field, word) in enumerate((("p0", p["type"] & 0xff), ("size", p["materialId"]), ("p1", p["index"]), ("p2", None))):
        prims[:, row, :3] = p[field]
        if word is not None:
            prims[:, row, 3] = _bits(word)
    with open(path, "wb") as f:
        np.array([len(b), len(p)], np.int32).tofile(f)
        rows.tofile(f)
        np.ascontiguousarray(b["startIndex"], np.int32).tofile(f)
        prims.tofile(f)


def _engine_scene(build):
    def write(solr, path):
        k = solr.Kernel(engine="host-only")
        build(solr, k)
        _scene_file(k.flat_scene(), path)
        k.finalize()
    return write


SCENES = {name: _engine_scene(build) for name, build in SCENES.items()}
# the synthetic node lists (tests/list_builder_cases.py), as scene files
SCENES.update({"case-" + name: (lambda solr, path, name=name: K.scene_file(name, path)) for name in K.FREE_CASES})


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_host_builders_make_lists_the_walks_can_rely_on(solr, checker, scene, tmp_path):
    path = str(tmp_path / "scene.bin")
    SCENES[scene](solr, path)
    run = subprocess.run([checker, path], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
