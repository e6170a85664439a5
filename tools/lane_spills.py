#!/usr/bin/env python3
"""Development aid: what a row file's kernels pay for scalars parked in vector lanes.

    python tools/lane_spills.py [sol-r_amd/csrc/rows/sphere_plane.hip] [--kernel ILi0ELi33E] [--keep row.s]

Compiles the row file for the device with the Makefile's own flags (assembly only, nothing is linked) and prints, per
k_standardRenderer / k_walkBound instantiation: the spill slots the register allocator gave to scalars
(.sgpr_spill_count), the vector registers, scratch, the kernel-argument bytes, vector / scalar / scalar-memory
instruction counts, the lane writes and reads that serve those spills (v_writelane_b32 / v_readlane_b32) with the
hazard nops, and how the lane traffic spreads over the loop nests: depth 0 is straight-line code (prologue, epilogue),
depth 1 the per-trip loop of the trace, deeper the lamp loop, the walks and their leaf loops.  A loop is what a backward
branch spans, the hand-written node loops included.  Vector instructions that read the kernel-argument pointer or an address made
from it are counted too: there should be none, every read of the segment a scalar load.

Static counts say what the compiler did, not what a frame executes: the device's instruction counter is the measure
(tools/profile_round.sh)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNEL = re.compile(r"^(_Z(?:18k_standardRenderer|11k_walkBound)\w+):\s*;", re.M)


def makefile_flags():
    text = open(os.path.join(ROOT, "sol-r_amd", "Makefile")).read().replace("\\\n", " ")
    numeric = re.search(r"^NUMERIC\s*=\s*(.*)$", text, re.M).group(1)
    flags = re.search(r"^HIPFLAGS\s*=\s*(.*)$", text, re.M).group(1)
    # (EXTRA_HIPFLAGS: as the Makefile takes it, for experiments)
    return flags.replace("$(NUMERIC)", numeric).replace("$(ARCH)", "gfx950").split() + os.environ.get("EXTRA_HIPFLAGS", "").split()


def assembly(row, keep=None):
    """the device assembly of a row file"""
    with tempfile.TemporaryDirectory() as tmp:
        out = keep or os.path.join(tmp, "row.s")
        done = subprocess.run([HIPCC] + makefile_flags() + ["--cuda-device-only", "-S", "-o", out, row],
                              stderr=subprocess.PIPE, text=True)
        if done.returncode:
            sys.exit(done.stderr)
        return open(out).read()


def metadata(text):
    """{kernel: {key: int}} from the notes at the end of the file"""
    out = {}
    for block in re.split(r"\n  - \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name:
            continue
        out[name.group(1)] = {k: int(v) for k, v in re.findall(
            r"\.(sgpr_spill_count|vgpr_spill_count|sgpr_count|vgpr_count|private_segment_fixed_size|kernarg_segment_size):\s+(\d+)",
            block)}
    return out


def bodies(text):
    """{kernel: [instruction or label lines]}"""
    out = {}
    for m in KERNEL.finditer(text):
        end = text.index(".Lfunc_end", m.end())
        lines = []
        for line in text[m.end():end].split("\n"):
            line = line.split(";")[0].split("//")[0].strip()
            if line and not (line.startswith(".") and not line.endswith(":")):
                lines.append(line)
        out[m.group(1)] = lines
    return out


def loop_depths(lines):
    """for every line, in how many loops it lies: a loop is the span of a backward branch"""
    where = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    delta = [0] * (len(lines) + 1)
    for i, l in enumerate(lines):
        m = re.match(r"s_c?branch\w*\s+(\S+)", l)
        if m and m.group(1) in where and where[m.group(1)] <= i:
            delta[where[m.group(1)]] += 1
            delta[i + 1] -= 1
    depth, d = [], 0
    for i in range(len(lines)):
        d += delta[i]
        depth.append(d)
    return depth


def _sgprs(operand):
    """the scalar registers an operand names: s5 -> {5}, s[10:11] -> {10, 11}"""
    m = re.fullmatch(r"s\[(\d+):(\d+)\]", operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"s(\d+)", operand)
    return {int(m.group(1))} if m else set()


def kernarg_vector_loads(lines):
    """vector instructions that read the kernel-argument pointer or an address made from it.  s[0:1] holds it at entry;
    scalar moves and arithmetic pass it on (followed in program order), a spill to a lane and back keeps it, a scalar
    load from it yields data, not an address.  While it stays on the scalar side no vector-memory load - global, flat
    or buffer - can address the segment."""
    held = {0, 1}
    slots = set()  # (vector register, lane) of a spilled half
    found = 0
    for l in lines:
        parts = l.split(None, 1)
        if l.endswith(":") or len(parts) < 2:
            continue
        operands = [o.strip().split()[0] for o in parts[1].split(",") if o.strip()]
        read = set().union(*[_sgprs(o) for o in operands[1:]]) if len(operands) > 1 else set()
        if l.startswith("v_writelane_b32"):
            if read & held:
                slots.add((operands[0], operands[2]))
            else:
                slots.discard((operands[0], operands[2]))
        elif l.startswith("v_readlane_b32"):
            held -= _sgprs(operands[0])
            if (operands[1], operands[2]) in slots:
                held |= _sgprs(operands[0])
        elif l.startswith("s_"):
            passes_on = re.match(r"s_(mov_b32|mov_b64|add_u32|addc_u32)\b", l) and (read & held)
            if not re.match(r"s_(cmp|bitcmp|c?branch|waitcnt|nop|store|setprio|sleep)", l):
                held -= _sgprs(operands[0])
                if passes_on:
                    held |= _sgprs(operands[0])
        else:
            # (a vector instruction's own scalar results: the carry of an addition, the flag of v_div_scale, a comparison)
            carries = re.match(r"v_(div_scale|add_co|sub_co|subrev_co|addc_co|subb_co|subbrev_co|mad_u64_u32|mad_i64_i32)", l)
            written = _sgprs(operands[0]) | (_sgprs(operands[1]) if carries and len(operands) > 1 else set())
            reads = set().union(*[_sgprs(o) for o in operands[(2 if carries else 1):]]) if len(operands) > 1 else set()
            # what could carry the pointer to the vector side: a move or 64-bit address arithmetic, or a load based on it
            if (reads & held) and re.match(r"(global_|flat_|buffer_|v_mov_b32|v_mov_b64|v_add_co_u32|v_addc_co_u32|v_lshl_add_u64)", l):
                found += 1
            held -= written
    return found


def measure(lines):
    depth = loop_depths(lines)
    code = [(l, d) for l, d in zip(lines, depth) if not l.endswith(":")]
    count = lambda pattern: sum(1 for l, _ in code if re.match(pattern, l))
    by_depth = {}
    for l, d in code:
        kind = "w" if l.startswith("v_writelane_b32") else "r" if l.startswith("v_readlane_b32") else None
        if kind:
            by_depth.setdefault(d, {"w": 0, "r": 0})[kind] += 1
    return {
        "instructions": len(code),
        "vector": count(r"(v_|ds_|global_|flat_|buffer_|scratch_)"),
        "valu": count(r"v_"),
        "scalar": count(r"s_(?!load|buffer_load|nop|waitcnt)"),
        "s_load": count(r"s_(buffer_)?load"),
        "s_nop": count(r"s_nop"),
        "writelane": count(r"v_writelane_b32"),
        "readlane": count(r"v_readlane_b32"),
        "by_depth": by_depth,
        "kernarg_vector_loads": kernarg_vector_loads(lines),
    }


def report(row, only=None, keep=None):
    """[(kernel, metadata, counts)] of a row file's kernels"""
    text = assembly(row, keep)
    meta = metadata(text)
    return [(name, meta.get(name, {}), measure(lines)) for name, lines in bodies(text).items()
            if only is None or only in name]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("row", nargs="?", default=os.path.join(ROOT, "sol-r_amd", "csrc", "rows", "sphere_plane.hip"))
    ap.add_argument("--kernel", help="only the instantiations whose mangled name contains this (ILi0ELi33E: the lean Cornell kernel)")
    ap.add_argument("--keep", help="leave the assembly in this file")
    a = ap.parse_args()
    for name, meta, c in report(a.row, a.kernel, a.keep):
        print(name)
        print("  sgpr spill slots %d  vgprs %d  scratch %d B  kernarg %d B" % (
            meta.get("sgpr_spill_count", -1), meta.get("vgpr_count", -1), meta.get("private_segment_fixed_size", -1),
            meta.get("kernarg_segment_size", -1)))
        print("  instructions %d  vector %d (valu %d)  scalar %d  s_load %d  s_nop %d" % (
            c["instructions"], c["vector"], c["valu"], c["scalar"], c["s_load"], c["s_nop"]))
        print("  v_writelane_b32 %d  v_readlane_b32 %d  (%.1f %% of valu)  vector reads of the kernel-argument pointer %d" % (
            c["writelane"], c["readlane"], 100.0 * (c["writelane"] + c["readlane"]) / max(c["valu"], 1),
            c["kernarg_vector_loads"]))
        for d in sorted(c["by_depth"]):
            print("    loop depth %d: %3d lane writes %3d lane reads" % (d, c["by_depth"][d]["w"], c["by_depth"][d]["r"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
