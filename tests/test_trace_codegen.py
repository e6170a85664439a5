"""What the compiler makes of the trace's early-outs and of the hit's records handed to the shader (rt_device.h
launchRayTracing, HitRecords; profiles/r12/trace_dead_trips.txt): the lean Cornell kernel keeps its four waves per SIMD
without scratch, and no instantiation with triangles - where neither change is compiled, their registers are gone - has
more scratch than the commit before had (profiles/r12/parent_resource_table.json).  No GPU needed: hipcc compiles the two
row files for gfx950 with the Makefile's own flags, and nothing but the kernels' resource metadata is read."""
import concurrent.futures
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ROWS = os.path.join(ROOT, "sol-r_amd", "csrc", "rows")
F_TRI = 16       # sol-r_amd/csrc/rt_device.h enum Feature
KEYS = ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")


def _makefile_flags():
    text = open(os.path.join(ROOT, "sol-r_amd", "Makefile")).read().replace("\\\n", " ")
    numeric = re.search(r"^NUMERIC\s*=\s*(.*)$", text, re.M).group(1)
    flags = re.search(r"^HIPFLAGS\s*=\s*(.*)$", text, re.M).group(1)
    return flags.replace("$(NUMERIC)", numeric).replace("$(ARCH)", "gfx950").split()


def _waves(vgprs):
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))


def _resources(row, tmp):
    """{(COUNT, FEAT): {key: int}} of the k_standardRenderer instantiations of a row file, from the metadata notes"""
    out = os.path.join(tmp, row + ".s")
    subprocess.run([HIPCC] + _makefile_flags() + ["--cuda-device-only", "-S", "-o", out, os.path.join(ROWS, row + ".hip")],
                   check=True, stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for block in re.split(r"\n  - \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+_Z18k_standardRendererILi(\d+)ELi(\d+)ELb0E", block)
        if name:
            found[(int(name.group(1)), int(name.group(2)))] = {
                k: int(v) for k, v in re.findall(r"\.(%s):\s+(\d+)" % "|".join(KEYS), block)}
    return found


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    tmp = str(tmp_path_factory.mktemp("isa"))
    rows = ("sphere_plane", "sphere_triangle")
    with concurrent.futures.ThreadPoolExecutor(len(rows)) as pool:          # (the two compilations side by side)
        return dict(zip(rows, pool.map(lambda row: _resources(row, tmp), rows)))


def test_the_lean_cornell_kernel_keeps_four_waves_without_scratch(resources):
    lean = resources["sphere_plane"][(0, 33)]
    print(lean)
    assert lean["private_segment_fixed_size"] == 0 and lean["vgpr_spill_count"] == 0
    assert lean["vgpr_count"] <= 128
    assert _waves(lean["vgpr_count"]) == 4


def test_no_instantiation_with_triangles_has_more_scratch_than_the_parent(resources):
    parent = json.load(open(os.path.join(ROOT, "profiles", "r12", "parent_resource_table.json")))["sphere_triangle.hip"]
    seen = 0
    for (count, feat), now in sorted(resources["sphere_triangle"].items()):
        assert feat & F_TRI
        before = parent["k_standardRenderer<%d, %d, false>" % (count, feat)]
        print((count, feat), "scratch %d B, the parent %d B" % (now["private_segment_fixed_size"], before["private_segment_fixed_size"]))
        assert now["private_segment_fixed_size"] <= before["private_segment_fixed_size"], (count, feat)
        seen += 1
    assert seen == 10
    assert not any(feat & F_TRI for _, feat in resources["sphere_plane"])
