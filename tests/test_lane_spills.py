"""Where the renderer's kernel arguments live (sol-r_amd/csrc/rt_device.h again(), renderer.h RendererArgs): every phase of
k_standardRenderer reads the fields it uses from the kernel-argument segment, with scalar loads, instead of carrying
what was loaded at entry across the walks in lanes of spill registers.  This is the fence behind that change, not its
measure (the device's instruction counter is: profiles/r8/kernel_argument_reloads.txt): the lean rows are compiled with
the Makefile's flags (tools/lane_spills.py) and

  * no instantiation of a lean row has more scalar spill slots than it had before the change (the figures below are a
    compile of that commit; profiles/r7/shadow_lamp_cutoff.txt has the Cornell kernel's 184),
  * the lean Cornell kernel fits 128 vector registers without scratch,
  * the kernel-argument pointer never reaches the vector side: every read of the segment is a scalar load,
  * k_walkBound, which has nothing to spill, is as it was.

No GPU needed: hipcc only compiles."""
import importlib.util
import os
import re
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("lane_spills", os.path.join(ROOT, "tools", "lane_spills.py"))
lane_spills = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lane_spills)

# .sgpr_spill_count of every k_standardRenderer<COUNT, FEAT> the lean row files hold, compiled from the commit before the
# arguments were re-read per phase: {row file: {(COUNT, FEAT): slots}}
BEFORE = {
    "sphere_plane": {(0, 1825): 211, (0, 1569): 190, (0, 1313): 204, (0, 1057): 189, (0, 801): 206, (0, 545): 185,
                     (0, 289): 199, (0, 33): 184, (2, 289): 223, (2, 33): 196},
    "sphere_triangle": {(0, 1809): 251, (0, 1553): 215, (0, 1297): 246, (0, 1041): 211, (0, 785): 246, (0, 529): 210,
                        (0, 273): 241, (0, 17): 206, (2, 273): 278, (2, 17): 230},
    "sphere_cylinder": {(0, 1797): 187, (0, 1541): 164, (0, 1285): 182, (0, 1029): 159, (0, 773): 182, (0, 517): 159,
                        (0, 261): 177, (0, 5): 154, (2, 261): 195, (2, 5): 184},
    "untextured_mix": {(0, 1845): 343, (0, 1333): 338, (0, 821): 343, (0, 309): 338, (2, 309): 359},
}
CORNELL = ("sphere_plane", (0, 33))  # k_standardRenderer<0, F_SPHERE | F_PLANE>: the frame bench.py measures


def _instantiation(name):
    m = re.match(r"_Z18k_standardRendererILi(\d+)ELi(\d+)ELb0E", name)
    return (int(m.group(1)), int(m.group(2))) if m else None


@pytest.fixture(scope="module")
def rows():
    """{row file: {(COUNT, FEAT) or the k_walkBound name: (metadata, counts)}}, the four row files compiled side by side"""
    if not os.path.exists(lane_spills.HIPCC):
        pytest.skip("no hipcc")
    path = lambda row: os.path.join(ROOT, "sol-r_amd", "csrc", "rows", row + ".hip")  # noqa: E731
    with ThreadPoolExecutor(len(BEFORE)) as pool:
        reports = list(pool.map(lambda row: lane_spills.report(path(row)), BEFORE))
    return {row: {_instantiation(name) or name: (meta, counts) for name, meta, counts in report}
            for row, report in zip(BEFORE, reports)}


def test_every_lean_instantiation_is_there(rows):
    for row, before in BEFORE.items():
        assert set(before) <= set(rows[row]), (row, sorted(set(before) - set(rows[row]), key=str))


def test_the_cornell_kernel(rows):
    meta, counts = rows[CORNELL[0]][CORNELL[1]]
    print(meta, counts)
    assert meta["sgpr_spill_count"] <= BEFORE[CORNELL[0]][CORNELL[1]] == 184
    assert meta["vgpr_count"] <= 128
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0
    assert meta["kernarg_segment_size"] <= 512
    assert counts["kernarg_vector_loads"] == 0
    # the lane traffic is what the spill slots cost: a write per slot, and no more reads than before (348)
    assert counts["writelane"] <= 184 and counts["readlane"] <= 348


def test_no_lean_row_spills_more_scalars_than_before(rows):
    worse = {}
    for row, before in BEFORE.items():
        for which, slots in before.items():
            meta, counts = rows[row][which]
            print(row, which, "spill slots", slots, "->", meta["sgpr_spill_count"], "vgprs", meta["vgpr_count"],
                  "scratch", meta["private_segment_fixed_size"])
            if meta["sgpr_spill_count"] > slots:
                worse[(row, which)] = (slots, meta["sgpr_spill_count"])
    assert not worse, worse


def test_every_read_of_the_arguments_is_a_scalar_load(rows):
    for row in BEFORE:
        for which, (meta, counts) in rows[row].items():
            assert counts["kernarg_vector_loads"] == 0, (row, which)
            assert meta["kernarg_segment_size"] <= 512, (row, which)


def test_the_walk_replay_has_nothing_to_spill(rows):
    replays = [(row, which, meta) for row in BEFORE for which, (meta, _) in rows[row].items() if isinstance(which, str)]
    assert len(replays) >= 4
    for row, which, meta in replays:
        assert "k_walkBound" in which
        assert meta["sgpr_spill_count"] == 0 and meta["vgpr_spill_count"] == 0, (row, which, meta)
        assert meta["vgpr_count"] == 64 and meta["private_segment_fixed_size"] == 0, (row, which, meta)
