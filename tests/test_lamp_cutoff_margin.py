"""The lamp's cut-off of the shadow walks (sol-r_amd/csrc/rt_device.h shadowWalk, `lampCut`): a shadow walk leaves out
every box whose entry parameter reaches farFree = 1.0002 + 1e-4 sum|o| / |L - o|.  That is exact only if a box that
holds a hit the walk would accept - a point nearer to the origin than the lamp - is never left out, rounding included.
Here the claim is put to random rays in numpy's binary32 with the node loop's own operations, (bound - o) * (1 / d) per
axis, then min / max: origins up to 35 000 units from zero, lamps anywhere in that range, points strictly before the
lamp, boxes from 1 to 20 000 units around the point (the reference's leaves) and boxes a margin thick with the point
anywhere inside, their faces included (the thin copies: margin = 2^-10 of a 40 000-unit extent).  No GPU."""
import os
import re

import numpy as np

F = np.float32
SAMPLES = 12_000_000
CHUNK = 1_000_000
MARGIN = F(40000.0 / 1024.0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _entry_parameter(lo, hi, o, d):
    """the node loop: v_pk_add (bound - o), v_pk_mul by the reciprocal, min per axis, max3; a zero component has the
    reciprocal 1 (makeWalkRay)"""
    with np.errstate(divide="ignore"):
        inv = np.where(d != 0, F(1) / d, F(1)).astype(F)
    a = ((lo - o).astype(F) * inv).astype(F)
    b = ((hi - o).astype(F) * inv).astype(F)
    return np.minimum(a, b).max(axis=1)


def _far_free(o, length):
    s = (np.abs(o[:, 0]) + np.abs(o[:, 1])).astype(F)
    s = (s + np.abs(o[:, 2])).astype(F)
    return (F(1.0002) + ((F(1.0e-4) * s).astype(F) / length).astype(F)).astype(F)


def _length(v):
    x = (v[:, 0] * v[:, 0]).astype(F)
    x = (x + (v[:, 1] * v[:, 1]).astype(F)).astype(F)
    x = (x + (v[:, 2] * v[:, 2]).astype(F)).astype(F)
    return np.sqrt(x).astype(F)


def _chunk(rng, n):
    # origins and lamps: log-uniform magnitudes up to 35 000 per axis, either sign; one ray in eight has a lamp that
    # shares a coordinate with the origin (a zero direction component), one in eight a lamp only a few units away
    def coordinates():
        magnitude = np.exp(rng.uniform(np.log(1.0e-2), np.log(35000.0), (n, 3)))
        return (magnitude * rng.choice([-1.0, 1.0], (n, 3))).astype(F)
    o = coordinates()
    lamp = coordinates()
    near = rng.random(n) < 0.125
    lamp[near] = (o[near] + rng.uniform(-8.0, 8.0, (int(near.sum()), 3))).astype(F)
    flat = rng.random(n) < 0.125
    axis = rng.integers(0, 3, n)
    lamp[flat, axis[flat]] = o[flat, axis[flat]]
    d = (lamp - o).astype(F)
    length = _length(d)
    # a point the walk would accept: before the lamp by the walk's own measure, l = |p - o| < |d| in binary32
    s = rng.random(n) ** 0.25          # most of them close to the lamp, where the margin is needed ...
    edge = rng.random(n) < 0.25        # ... and a quarter within rounding of it, on either side: `keep` decides as the walk does
    s[edge] = 1.0 + rng.uniform(-4.0e-7, 4.0e-7, int(edge.sum()))
    p = (o.astype(np.float64) + s[:, None] * d.astype(np.float64)).astype(F)
    keep = (_length((p - o).astype(F)) < length) & (length >= F(2)) & ((d * d).sum(axis=1) <= 1.0e24)
    # the boxes around it
    below = np.exp(rng.uniform(0.0, np.log(20000.0), (n, 3))) * rng.random((n, 3))
    above = np.exp(rng.uniform(0.0, np.log(20000.0), (n, 3))) * rng.random((n, 3))
    thin = rng.random(n) < 0.5
    thin_axis = rng.integers(0, 3, n)
    rows = np.nonzero(thin)[0]
    below[rows, thin_axis[rows]] = float(MARGIN) * rng.random(rows.size) * rng.integers(0, 2, rows.size)
    above[rows, thin_axis[rows]] = float(MARGIN) * rng.random(rows.size) * rng.integers(0, 2, rows.size)
    lo = np.minimum((p - below.astype(F)).astype(F), p)   # (rounded towards the point at worst: the box holds it)
    hi = np.maximum((p + above.astype(F)).astype(F), p)
    return o[keep], d[keep], length[keep], lo[keep], hi[keep]


def test_the_source_has_the_formula_tested_here():
    text = open(os.path.join(ROOT, "sol-r_amd", "csrc", "rt_device.h")).read()
    assert re.search(r"farFree = 1\.0002f \+ 1\.0e-4f \* \(fabsf\(r\.o\.x\) \+ fabsf\(r\.o\.y\) \+ fabsf\(r\.o\.z\)\) / lengthOL;",
                     text)
    assert "fminf(minDistance, farFree)" in text


def test_a_box_that_holds_a_point_before_the_lamp_begins_before_the_cut_off():
    rng = np.random.default_rng(20260117)
    tested = violations = 0
    used = 0.0       # the largest (tmin - 1) / (farFree - 1): the share of the margin a sample used up
    while tested < SAMPLES:
        o, d, length, lo, hi = _chunk(rng, CHUNK)
        tmin = _entry_parameter(lo, hi, o, d)
        far = _far_free(o, length)
        violations += int((~(tmin < far)).sum())
        share = (tmin.astype(np.float64) - 1.0) / (far.astype(np.float64) - 1.0)
        used = max(used, float(share.max()))
        tested += o.shape[0]
    print("lamp cut-off margin: %d samples, %d violations, largest share of the margin used %.5f" % (tested, violations, used))
    assert tested >= 10_000_000
    assert violations == 0
