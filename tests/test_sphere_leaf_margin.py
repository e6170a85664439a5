"""The thin box of a sphere (sol-r_amd/csrc/build_bounds.h sphereBuildExtent): every ray that the sphere test's own arithmetic
(rt_device.h sphereHit: normalised direction, a = 2 n.n, b = 2 (o - p).n, c = |o - p|^2 - r^2, d = b b - 2 a c, the roots,
the epsilon) calls a hit has to pass the slab test of the box p -+ extent with the node loop's own operations ((bound - o) *
(1 / d) per axis, min / max), and enter it before the hit.  Put to random rays in numpy's binary32, in the manner of
tests/test_lamp_cutoff_margin.py: spheres of radius 10 ... 2000 inside a scene of extent 55 000 (the Cornell scene's), origins
up to viewDistance from zero on every axis - 50 000, the Cornell frame's, and 200 000, beyond the extent: the reach follows
it - aimed at the sphere's rim: a hair inside, on it, outside it by up to a few hundred units, and straight at it; long
directions and short ones (the bounce rays), origins inside the sphere and a few units outside it.  No GPU.

Why the box is not p -+ (r + margin): d is a difference of two numbers of the size 4 s^2 (s = |o - p|), and its sign decides.
A ray that misses a sphere of radius 10 by tens of units from 100 000 units away is called a hit - the reference, which
gives the lamps' cell the box +-viewDistance, finds such hits, and so must a walk of the thin copy.  The test prints how
many of its computed hits the box without the allowance for that would have lost."""
import os
import re

import numpy as np

import list_copies_model as M
import sphere_leaves_model as S

F = np.float32
EXTENT = F(55000.0)
MARGIN = M.margin_of(EXTENT)
EPSILON = F(0.001)      # sceneInfo.geometryEpsilon's default
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAYS = 240_000          # per radius band and viewDistance


def _dot(a, b):
    # rt_device.h dot: (a.x b.x + a.y b.y) + a.z b.z, every product and sum rounded
    p = ((a[:, 0] * b[:, 0]).astype(F) + (a[:, 1] * b[:, 1]).astype(F)).astype(F)
    return (p + (a[:, 2] * b[:, 2]).astype(F)).astype(F)


def _sphere_hit(o, d, p0, radius):
    """sphereHit: (hit, t) - t the parameter along the normalised direction"""
    with np.errstate(all="ignore"):
        inv_len = (F(1) / np.sqrt(_dot(d, d)).astype(F)).astype(F)
        n = (d * inv_len[:, None]).astype(F)
        oc = (o - p0).astype(F)
        a = (F(2) * _dot(n, n)).astype(F)
        b = (F(2) * _dot(oc, n)).astype(F)
        c = (_dot(oc, oc) - (radius * radius).astype(F)).astype(F)
        disc = ((b * b).astype(F) - ((F(2) * a).astype(F) * c).astype(F)).astype(F)
        ok = ~((disc <= 0) | (a == 0))
        root = np.sqrt(np.where(ok, disc, F(1))).astype(F)
        t1 = ((-b - root).astype(F) / a).astype(F)
        t2 = ((-b + root).astype(F) / a).astype(F)
        b1, b2 = t1 <= EPSILON, t2 <= EPSILON
        ok &= ~(b1 & b2)
        t = np.where(b1, t2, np.where(b2, t1, np.where(t1 < t2, t1, t2)))
        ok &= ~(t < EPSILON)
    return ok, t


def _slab(lo, hi, o, d):
    """the node loop: (bound - o) * (1 / d) per axis (a zero component has the reciprocal 1), min per axis, max3; max, min3"""
    with np.errstate(divide="ignore"):
        inv = np.where(d != 0, F(1) / d, F(1)).astype(F)
    a = ((lo - o).astype(F) * inv).astype(F)
    b = ((hi - o).astype(F) * inv).astype(F)
    return np.minimum(a, b).max(axis=1), np.maximum(a, b).min(axis=1)


def _extents(p0, radius, reach):
    """S.sphere_extent for arrays, the same operations"""
    far = (F(reach) + np.abs(p0).max(axis=1).astype(F)).astype(F)
    slack = (((F(3) * far).astype(F) * F(2.0 ** -21)).astype(F) / (radius / far).astype(F)).astype(F)
    return (((radius + MARGIN).astype(F) + slack).astype(F) + (far * F(2.0 ** -9)).astype(F)).astype(F)


def _rays(rng, n, r_lo, r_hi, view):
    radius = np.exp(rng.uniform(np.log(r_lo), np.log(r_hi), n)).astype(F)
    room = float(EXTENT) - radius.astype(np.float64)
    p0 = (rng.uniform(-1, 1, (n, 3)) * room[:, None]).astype(F)
    # origins: log-uniform distances from zero up to viewDistance per axis, a quarter at +-viewDistance on some axis, an
    # eighth inside the sphere or within a few units of it
    mag = np.exp(rng.uniform(np.log(1.0), np.log(view), (n, 3)))
    o = (mag * rng.choice([-1.0, 1.0], (n, 3))).astype(F)
    edge = rng.random(n) < 0.25
    axis = rng.integers(0, 3, n)
    o[edge, axis[edge]] = (view * rng.choice([-1.0, 1.0], int(edge.sum()))).astype(F)
    near = rng.random(n) < 0.125
    step = rng.normal(size=(int(near.sum()), 3))
    step *= (radius[near] * rng.uniform(0.0, 1.3, int(near.sum())) / np.linalg.norm(step, axis=1))[:, None]
    o[near] = np.clip(p0[near] + step, -view, view).astype(F)
    # targets: the point of the sphere's rim as seen from the origin, moved off the rim by `off`
    to = p0.astype(np.float64) - o.astype(np.float64)
    u = rng.normal(size=(n, 3))
    u -= (u * to).sum(axis=1)[:, None] * to / np.maximum((to * to).sum(axis=1), 1e-30)[:, None]
    u /= np.maximum(np.linalg.norm(u, axis=1), 1e-30)[:, None]
    scale = rng.choice([0.0, 1.0e-4, 1.0e-2, 1.0, 30.0, 300.0], n)
    off = radius * np.where(rng.random(n) < 0.2, rng.random(n), 1.0) + rng.uniform(-1, 1, n) * scale
    target = p0.astype(np.float64) + u * off[:, None]
    d = target - o.astype(np.float64)
    length = np.exp(rng.uniform(np.log(0.5), np.log(1.0e5), n))
    d = (d * (length / np.maximum(np.linalg.norm(d, axis=1), 1e-30))[:, None]).astype(F)
    keep = (d != 0).all(axis=1) & np.isfinite(d).all(axis=1)
    return o[keep], d[keep], p0[keep], radius[keep]


def test_the_source_has_the_formula_tested_here():
    text = open(os.path.join(ROOT, "sol-r_amd", "csrc", "build_bounds.h")).read()
    assert re.search(r"const float far = reach \+ fmaxf\(fmaxf\(fabsf\(p\.x\), fabsf\(p\.y\)\), fabsf\(p\.z\)\);", text)
    assert "return ((r + margin) + (3.f * far * 0x1p-21f) / (r / far)) + far * 0x1p-9f;" in text
    device = open(os.path.join(ROOT, "sol-r_amd", "csrc", "rt_device.h")).read()
    assert "const float d = b * b - 2.f * a * c;" in device and "const float b = 2.f * dot(O_C, dir);" in device
    # the array form above is the model's
    rng = np.random.default_rng(3)
    p0 = rng.uniform(-50000, 50000, (64, 3)).astype(F)
    radius = rng.uniform(10, 2000, 64).astype(F)
    mine = _extents(p0, radius, 61000.0)
    assert all(mine[i].view(np.int32) == S.sphere_extent(p0[i], radius[i], MARGIN, 61000.0).view(np.int32) for i in range(64))


def test_a_ray_the_sphere_test_calls_a_hit_enters_the_thin_box_before_it():
    rng = np.random.default_rng(20261020)
    for view in (50000.0, 200000.0):
        reach = S.reach_of(EXTENT, view)
        for r_lo, r_hi in ((10.0, 12.0), (12.0, 200.0), (200.0, 2000.0)):
            o, d, p0, radius = _rays(rng, RAYS, r_lo, r_hi, view)
            hit, t = _sphere_hit(o, d, p0, radius)
            o, d, p0, radius, t = o[hit], d[hit], p0[hit], radius[hit], t[hit]
            e = _extents(p0, radius, reach)
            assert np.isfinite(e).all()
            tmin, tmax = _slab((p0 - e[:, None]).astype(F), (p0 + e[:, None]).astype(F), o, d)
            length = np.linalg.norm(d.astype(np.float64), axis=1)
            passes = (tmin <= tmax) & (tmax > 0) & (tmin.astype(np.float64) * length < t)
            # how far outside the sphere the line of a computed hit passes, against the allowance made for it
            w = p0.astype(np.float64) - o.astype(np.float64)
            miss = np.linalg.norm(np.cross(w, d.astype(np.float64)), axis=1) / length - radius
            allowed = (e - radius - MARGIN).astype(np.float64)
            plain = (radius + MARGIN).astype(F)
            pmin, pmax = _slab((p0 - plain[:, None]).astype(F), (p0 + plain[:, None]).astype(F), o, d)
            lost = int((~((pmin <= pmax) & (pmax > 0))).sum())
            print("viewDistance %6.0f, radius %4.0f ... %4.0f: %6d computed hits, %d outside the thin box; the line of one passes "
                  "the sphere at up to %8.2f (largest share of the allowance used %.3f); p -+ (r + margin) would lose %d"
                  % (view, r_lo, r_hi, len(t), int((~passes).sum()), miss.max(), (miss / allowed).max(), lost))
            assert len(t) >= RAYS // 8
            assert passes.all()
