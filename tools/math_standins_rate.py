"""How often do pow_f's lean path, pow_general and the host's stand-in disagree?  (profiles/r23/math_standins.txt)

Bases in [0.3, 1) and exponents in [1, 300] - the Blinn term's neighbourhood - in blocks of 2^20 seeded inputs, each block
through solr_hip_probe_math as pow_f (pure lean waves) and as pow_general, and through numpy's binary64 pow rounded once
(what the oracle's rounded mode computes).  Prints the three disagreement counts, how many inputs the 2^-41 rule of
tests/math_cases.py excludes, and the inputs on which anything differed, in hex.

    python tools/math_standins_rate.py [blocks, default 32]
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import engine_probes as E  # noqa: E402
import math_cases as M  # noqa: E402


def main():
    blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    hip = importlib.import_module("sol-r_amd").hip_lib()
    n = 1 << 20
    total = dict(inputs=0, excluded=0, lean_host=0, general_host=0, lean_general=0, outside=0)
    examples = []
    for block in range(blocks):
        rng = np.random.default_rng(9000 + block)
        a, b = M.narrow(rng.uniform(0.3, 1.0, n)), M.narrow(rng.uniform(1.0, 300.0, n))
        assert M.lean_domain(a, b).all()
        h = M.host64(M.POW, a, b)
        host = M.narrow(h)
        lean, general = E.probe_math(hip, M.POW, a, b), E.probe_math(hip, M.POW_GENERAL, a, b)
        excluded = M.sweep_excluded(h, 2.0 ** -41, 0)
        d1, d2, d3 = ~M.same_bits(lean, host), ~M.same_bits(general, host), ~M.same_bits(lean, general)
        total["inputs"] += n
        total["excluded"] += int(excluded.sum())
        total["lean_host"] += int(d1.sum())
        total["general_host"] += int(d2.sum())
        total["lean_general"] += int(d3.sum())
        total["outside"] += int(((d1 | d3) & ~excluded).sum())
        for i in np.flatnonzero(d1 | d2 | d3):
            examples.append("  a %s b %s: lean %s general %s host %s" % (
                float(a[i]).hex(), float(b[i]).hex(), float(lean[i]).hex(), float(general[i]).hex(), float(host[i]).hex()))
    print("pow, a in [0.3, 1), b in [1, 300]: %(inputs)d inputs, %(excluded)d within 2^-41 (+ 2 binary64 ULPs) of a rounding "
          "boundary; pow_f lean != host stand-in on %(lean_host)d, pow_general != host stand-in on %(general_host)d, "
          "pow_f lean != pow_general on %(lean_general)d; %(outside)d of the disagreements outside the excluded inputs" % total)
    print("\n".join(examples))


if __name__ == "__main__":
    main()
