"""Writes tests/golden/math_standins.npz: the inputs of tests/math_cases.py for the transcendental stand-ins of
sol-r_amd/csrc/rt_device.h (pow_f / pow_general, sin_f, cos_f, atan2_f, asin_f) with, per input and from mpmath at 256 bits,

  <op>_bits    the correctly rounded binary32 result;
  <op>_margin  floor(log2(the relative distance from the exact value to the nearest binary32 rounding boundary)), clipped
               into an int8.  A rounding boundary is a midpoint of adjacent binary32 values - subnormal spacing below
               2^-126, 2^128 - 2^103 above FLT_MAX.  -128: an exact tie; 127: an exact zero;
  <op>_side    the sign of exact - rounded (0: the result is exact): the other float that brackets the exact value lies
               one step from the rounded one on that side.

The GPU tests read the file with numpy alone; tests/test_math_fixture.py regenerates a subsample when mpmath imports.

    python tests/golden/make_math_fixtures.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import math_cases as M  # noqa: E402

PRECISION = 256
FIXTURE = os.path.join(HERE, "math_standins.npz")


def exact(mp, op, a, b):
    """the exact value of the op at binary32 inputs given as binary64 floats: an mpf at PRECISION bits"""
    a, b = mp.mpf(float(a)), mp.mpf(float(b))
    if op == M.POW:
        return mp.mpf(0) if a == 0 else mp.power(a, b)
    if op == M.SIN:
        return mp.sin(a)
    if op == M.COS:
        return mp.cos(a)
    if op == M.ASIN:
        return mp.asin(a)
    if op == M.ATAN2:
        return mp.atan2(a, b)
    raise KeyError(op)


def rounded(mp, y, negative_zero=False):
    """(bits, margin, side) of an exact value"""
    if y == 0:
        return (0x80000000 if negative_zero else 0), 127, 0
    sign = 0x80000000 if y < 0 else 0
    y = abs(y)
    top = mp.mpf(2) ** 128 - mp.mpf(2) ** 103
    if y >= mp.mpf(2) ** 128:
        distance = (y - top) / y
        result, side = 0x7F800000, -1
    else:
        e = max(int(mp.floor(mp.log(y, 2))), -126)
        while e > -126 and mp.ldexp(mp.mpf(1), e) > y:
            e -= 1
        while mp.ldexp(mp.mpf(1), e + 1) <= y:
            e += 1
        q = mp.ldexp(y, 23 - e)                      # in units of the binary32 spacing at y
        k = int(mp.floor(q))
        frac = q - k
        half = mp.mpf(0.5)
        up = frac > half or (frac == half and (k & 1))
        kr = k + 1 if up else k
        side = 0 if frac == 0 else (-1 if up else 1)
        d = abs(frac - half)
        if e > -126:                                 # just above a power of two the boundary below is a quarter step away
            d = min(d, q - (mp.mpf(2) ** 23 - mp.mpf(0.25)))
        distance = d / q
        result = ((e + 126) << 23) + kr
        if result >= 0x7F800000:
            result = 0x7F800000
    margin = -128 if distance == 0 else max(-128, min(127, int(mp.floor(mp.log(distance, 2)))))
    return sign | result, margin, (-side if sign else side)


def reference(mp, op, a, b=None):
    """arrays (bits uint32, margin int8, side int8) for binary32 input arrays"""
    mp.mp.prec = PRECISION
    a = M.widen(a)
    b = np.zeros(len(a)) if b is None else M.widen(b)
    out = [rounded(mp, exact(mp, op, x, y), negative_zero=bool(np.signbit(x)) and op in (M.SIN, M.ASIN, M.ATAN2))
           for x, y in zip(a, b)]
    return (np.array([o[0] for o in out], np.uint32), np.array([o[1] for o in out], np.int8),
            np.array([o[2] for o in out], np.int8))


def exact64(mp, op, a, b=None):
    """the exact values rounded to binary64 (for the accuracy of the host's routines)"""
    mp.mp.prec = PRECISION
    a = M.widen(a)
    b = np.zeros(len(a)) if b is None else M.widen(b)
    out = np.zeros(len(a))
    for i, (x, y) in enumerate(zip(a, b)):
        v = exact(mp, op, x, y)
        out[i] = float(v) if abs(v) < mp.mpf(2) ** 1023 else (np.inf if v > 0 else -np.inf)
    return out


def inputs():
    """{op name: (op, a, b or None, group)} from the seeded generators"""
    pa, pb, pg = M.pow_cases()
    ta, tg = M.trig_cases()
    sa, sg = M.asin_cases()
    aa, ab, ag = M.atan2_cases()
    return {"pow": (M.POW, pa, pb, pg), "sin": (M.SIN, ta, None, tg), "cos": (M.COS, ta, None, tg),
            "asin": (M.ASIN, sa, None, sg), "atan2": (M.ATAN2, aa, ab, ag)}


def main():
    import mpmath
    arrays = {}
    for name, (op, a, b, group) in inputs().items():
        stem = "trig" if name in ("sin", "cos") else name
        arrays[stem + "_a"], arrays[stem + "_group"] = a, group
        if b is not None:
            arrays[stem + "_b"] = b
        arrays[name + "_bits"], arrays[name + "_margin"], arrays[name + "_side"] = reference(mpmath, op, a, b)
        print("%-6s %5d inputs, %d with a margin at or under 2^-41" % (name, len(a), int((arrays[name + "_margin"] <= -41).sum())))
    np.savez_compressed(FIXTURE, **arrays)
    print("%s: %d bytes" % (FIXTURE, os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    main()
