#!/usr/bin/env python3
"""Development aid: the resource notes of every kernel of the renderer's row files and of the probes, this tree against
another tree (a worktree of the parent commit), as profiles/r11/walk_refactor_codegen.txt shows them.

    python tools/codegen_table.py ab/wt/<commit> [--json parent_table.json]

Compiles csrc/rows/*.hip and csrc/solr_probes.hip of both trees for the device with the Makefile's flags (assembly only,
as tools/lane_spills.py does) and reads the metadata: .vgpr_count, .sgpr_count, .sgpr_spill_count, .vgpr_spill_count,
.private_segment_fixed_size.  waves/SIMD = min(8, 512 / vgpr rounded up to the allocation block of 8).  --json writes
the other tree's figures, per row file and demangled kernel, for tests/test_trace_codegen.py."""
import argparse
import concurrent.futures
import glob
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lane_spills  # noqa: E402

KEYS = ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")


def waves(vgprs):
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))


def demangle(names):
    out = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True).stdout.split("\n")
    short = {}
    for name, d in zip(names, out):
        m = re.match(r"void (\w+(?:<[^>]*>)?)", d)
        short[name] = m.group(1) if m else d.split("(")[0]
    return short


def table(root):
    """{row file: {kernel: {key: int}}}"""
    csrc = os.path.join(root, "sol-r_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "rows", "*.hip"))) + [os.path.join(csrc, "solr_probes.hip")]
    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        texts = list(pool.map(lane_spills.assembly, files))
    out = {}
    for f, text in zip(files, texts):
        meta = lane_spills.metadata(text)
        short = demangle(list(meta))
        out[os.path.basename(f)] = {short[k]: {key: v.get(key, 0) for key in KEYS} for k, v in meta.items()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("other", help="the tree to compare with (a worktree of the parent commit)")
    ap.add_argument("--json", help="write the other tree's table here")
    a = ap.parse_args()
    here = table(lane_spills.ROOT)
    there = table(a.other)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(there, f, indent=1, sort_keys=True)
            f.write("\n")
    worse = 0
    for row in sorted(here):
        print(row)
        print("  %-42s %-7s %5s %5s %10s %10s %8s  waves/SIMD  verdict" % ("kernel", "side", "vgpr", "sgpr", "sgpr_spill",
                                                                            "vgpr_spill", "scratch"))
        for kernel in sorted(here[row]):
            h, p = here[row][kernel], there.get(row, {}).get(kernel)
            line = lambda side, r: "%-7s %5d %5d %10d %10d %8d  %d" % ((side,) + tuple(r[k] for k in KEYS) + (waves(r["vgpr_count"]),))  # noqa: E731
            if p is None:
                print("  %-42s %s           new" % (kernel, line("change", h)))
                continue
            print("  %-42s %s" % (kernel, line("parent", p)))
            if h == p:
                verdict = "identical"
            elif waves(h["vgpr_count"]) < waves(p["vgpr_count"]) or h["private_segment_fixed_size"] > p["private_segment_fixed_size"]:
                verdict = "WORSE (waves lost or scratch gained)"
                worse += 1
            else:
                verdict = "pass (same waves, scratch not above the parent's)"
            print("  %-42s %s           %s" % ("", line("change", h), verdict))
    print("kernels that lost waves per SIMD or gained scratch: %d" % worse)
    return 0


if __name__ == "__main__":
    sys.exit(main())
