"""(CPU) The references of tests/test_math_standins_gpu.py, held on their own before any device is: the fixture
tests/golden/math_standins.npz against its generators and (when mpmath imports) against mpmath again, the numpy models of
tests/math_cases.py against exact arithmetic, numpy's binary64 routines - the stand-in of the oracle's rounded mode and the
reference of the dense sweeps - against the fixture, the share of inputs the rules exclude, and the binary64 emulation of
pow_f's lean path in tools/gen_pow_table.py, with the degrees the device evaluates, against the same fixture by the same
rule as the device.  Three deliberately wrong variants (a table entry one unit of its last place off, a degree-8 exp2, a
contracted dot product) show that the rules can fail."""
import importlib.util
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import math_cases as M  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def maker():
    return _load("make_math_fixtures", os.path.join(HERE, "golden", "make_math_fixtures.py"))


@pytest.fixture(scope="module")
def fixture(maker):
    return dict(np.load(maker.FIXTURE))


@pytest.fixture(scope="module")
def generator():
    return _load("gen_pow_table", os.path.join(ROOT, "tools", "gen_pow_table.py"))


def _stem(name):
    return "trig" if name in ("sin", "cos") else name


def _case(fixture, name):
    stem = _stem(name)
    return fixture[stem + "_a"], fixture.get(stem + "_b"), fixture[stem + "_group"]


OPS = {"pow": M.POW, "sin": M.SIN, "cos": M.COS, "asin": M.ASIN, "atan2": M.ATAN2}


# ---- the fixture -----------------------------------------------------------------------------------------------------
def test_fixture_holds_the_generators_inputs(maker, fixture):
    assert os.path.getsize(maker.FIXTURE) <= 248053            # the JPEG fixtures next to it
    for name, (op, a, b, group) in maker.inputs().items():
        fa, fb, fg = _case(fixture, name)
        assert np.array_equal(M.bits(fa), M.bits(a)) and np.array_equal(fg, group), name
        assert (b is None and fb is None) or np.array_equal(M.bits(fb), M.bits(b)), name
        assert len(fixture[name + "_bits"]) == len(a) and fixture[name + "_margin"].dtype == np.int8


def test_a_subsample_regenerates_bit_for_bit(maker, fixture):
    mpmath = pytest.importorskip("mpmath")
    for name, op in OPS.items():
        a, b, _ = _case(fixture, name)
        pick = np.sort(np.random.default_rng(77 + op).choice(len(a), len(a) // 12, replace=False))
        got = maker.reference(mpmath, op, a[pick], None if b is None else b[pick])
        for key, g in zip(("_bits", "_margin", "_side"), got):
            assert np.array_equal(g, fixture[name + key][pick]), (name, key)


def test_the_hard_cases_are_in_the_fixture(fixture):
    a, b, group = _case(fixture, "pow")
    res, margin, side = fixture["pow_bits"], fixture["pow_margin"], fixture["pow_side"]
    g = {name: group == i for i, name in enumerate(M.POW_GROUPS)}
    assert all(m.any() for m in g.values())
    # every table-interval edge at five exponents: both floats of every edge
    ba = M.bits(a[g["table_edges"]]).astype(np.int64)
    for e in (-1, 0, 1, -100, 60):
        at = ba[((ba >> 23) - 127) == e]
        assert set(((at >> 16) & 0x7F)[(at & 0xFFFF) == 0]) == set(range(128)), e          # 1 + i/128 itself
        assert set(((at >> 16) & 0x7F)[(at & 0xFFFF) == 0xFFFF]) >= set(range(127)), e     # the float below the next edge
    assert (((ba >> 23) - 127) == -2).any() and (((ba >> 23) - 127) == 59).any()           # the float below i = 0
    near = g["near_one"]
    assert set(M.bits(a[near]).tolist()) == {0x3F800000, 0x3F7FFFFF, 0x3F800001} and near.sum() == 9
    assert set(b[near].tolist()) == {2.0 ** -20, 1.0, 4096.0}
    assert np.array_equal(res[g["b_is_one"]], M.bits(a[g["b_is_one"]]))                     # pow(a, 1) is a
    assert (side[g["exact"]] == 0).all() and (margin[g["exact"]] >= -26).all()
    assert (margin[g["ties"]] == -128).all() and (side[g["ties"]] != 0).all() and (res[g["ties"]] & 1 == 0).all()
    exps = ((res[g["result_edges"]].astype(np.int64) >> 23) & 0xFF)
    assert (exps == 0).sum() > 60 and (res[g["result_edges"]] == 0).any() and (res[g["result_edges"]] == 0x7F800000).any()
    assert ((exps >= 1) & (exps <= 2)).any() and (exps == 254).any()
    edge = a[g["domain_edges"]], b[g["domain_edges"]]
    for value in (M.FLT_MIN, M._next(M.FLT_MIN, -1), M.MIN_SUBNORMAL, M._next(M.LEAN_A_LIMIT, -1), M.LEAN_A_LIMIT, M.FLT_MAX, 0.0):
        assert (M.bits(edge[0]) == M.bits(value)).any(), value
    for value in (M.MIN_SUBNORMAL, 4096.0, M._next(M.LEAN_B_LIMIT, 1)):
        assert (M.bits(edge[1]) == M.bits(value)).any(), value
    lean = M.lean_domain(*edge)
    assert lean.any() and (~lean).any()
    assert set(M.blinn_powers().tolist()) <= set(b[g["blinn"]].tolist()) and len(M.blinn_powers()) == 259
    assert (a[g["blinn"]] > 0).all() and (a[g["blinn"]] <= 1).all()
    assert [(float(x).hex(), float(y).hex()) for x, y in zip(a[g["candidates"]], b[g["candidates"]])] == \
        [(float.fromhex(x).hex(), float.fromhex(y).hex()) for x, y in M.POW_CANDIDATES]
    # what the issue says of the candidates: 2^-42.7 to 2^-44 from a midpoint
    assert ((margin[g["candidates"]] >= -45) & (margin[g["candidates"]] <= -43)).all(), margin[g["candidates"]]
    ta, _, tg = _case(fixture, "sin")
    assert (np.abs(ta) >= 2.0 ** 127).any() and (M.bits(np.abs(ta)) < 0x00800000).any() and (np.abs(ta) > 2.0 ** 30).sum() > 100
    sa = _case(fixture, "asin")[0]
    assert {0x3F800000, 0xBF800000, 0x3F7FFFFF, 0xBF7FFFFF} <= set(M.bits(sa).tolist()) and (M.bits(np.abs(sa)) < 0x00800000).any()
    sub = (fixture["atan2_bits"] & 0x7F800000) == 0
    assert sub.sum() > 50                                                                   # subnormal results


# ---- the models --------------------------------------------------------------------------------------------------------
def _exact_f32(x):
    """a Fraction rounded to binary32 (nearest even, subnormals, overflow): the bits"""
    if x == 0:
        return 0
    sign = 0x80000000 if x < 0 else 0
    x = abs(x)
    e = max(x.numerator.bit_length() - x.denominator.bit_length(), -126)
    while e > -126 and Fraction(2) ** e > x:
        e -= 1
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    q = x / Fraction(2) ** (e - 23)
    k = q.numerator // q.denominator
    frac = q - k
    if frac > Fraction(1, 2) or (frac == Fraction(1, 2) and k & 1):
        k += 1
    return sign | min(((e + 126) << 23) + k, 0x7F800000)


def test_models_equal_exact_arithmetic():
    rng = np.random.default_rng(5)
    every = np.concatenate([rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32),
                            np.arange(0, 40, dtype=np.uint32), np.arange(0x007FFFF0, 0x00800010, dtype=np.uint32)])
    x = M.from_bits(every)
    finite = np.isfinite(x)
    assert np.array_equal(M.bits(M.narrow(M.widen(x)))[finite], every[finite])              # through binary64 and back
    assert all(Fraction(float(w)) == Fraction(int(b & 0x7FFFFF) + (0 if (b >> 23) & 0xFF == 0 else 1 << 23)) *
               Fraction(2) ** (max(int((b >> 23) & 0xFF), 1) - 150) * (-1 if b >> 31 else 1)
               for w, b in zip(M.widen(x[finite][:3000]), every[finite][:3000]))
    n = 600
    a = np.concatenate([M._log_uniform(rng, n, -8, 8, True), M._log_uniform(rng, n, -126, -100, True), M._log_uniform(rng, n, -75, -60, True)])
    b = np.concatenate([M._log_uniform(rng, n, -8, 8, True), M._log_uniform(rng, n, 10, 40, True), M._log_uniform(rng, n, -75, -60, True)])
    c = np.concatenate([M._log_uniform(rng, n, -8, 8, True), M._log_uniform(rng, n, -149, -120, True), M._log_uniform(rng, n, -149, -120, True)])
    c[:n:2] = M.narrow(-(M.widen(a[:n:2]) * M.widen(b[:n:2])))                            # cancellation: the fused result differs
    fa, fb, fc = ([Fraction(float(v)) for v in M.widen(z)] for z in (a, b, c))
    for got, want in ((M.mul(a, b), [p * q for p, q in zip(fa, fb)]), (M.add(a, c), [p + q for p, q in zip(fa, fc)]),
                      (M.div(a, b), [p / q for p, q in zip(fa, fb)]), (M.fma(a, b, c), [p * q + r for p, q, r in zip(fa, fb, fc)])):
        assert M.bits(got).tolist() == [_exact_f32(w) for w in want]
    assert (M.bits(M.fma(a, b, c)) != M.bits(M.add(M.mul(a, b), c))).sum() > n // 2
    # sqrt: the rounded root is the nearest float to the exact one - its neighbours' midpoints bracket the argument
    s = np.concatenate([M._log_uniform(rng, 2000, -126, 128), M.from_bits(rng.integers(1, 1 << 23, 500).astype(np.uint32))])
    r = M.sqrt(s)
    lo = [(Fraction(float(p)) + Fraction(float(q))) / 2 for p, q in zip(M.widen(M._next(r, -1)), M.widen(r))]
    hi = [(Fraction(float(p)) + Fraction(float(q))) / 2 for p, q in zip(M.widen(M._next(r, 1)), M.widen(r))]
    assert all(l * l <= Fraction(float(v)) <= h * h for l, h, v in zip(lo, hi, M.widen(s)))
    cast = M.f2i(np.array([np.nan, 2147483648.0, -2147483648.0, 3e38, -3e38, np.inf, -np.inf, 2147483520.0, -2.9, 2.9, -0.0, 1e-45], M.f32))
    assert cast.tolist() == [0, 2147483647, -2147483648, 2147483647, -2147483648, 2147483647, -2147483648, 2147483520, -2, 2, 0, 0]


def test_a_contracted_product_differs_on_the_vector_inputs():
    u, v, s, searched = M.exact_vector_inputs()
    assert searched >= 1024
    u, v = u[:searched], v[:searched]
    for variant in (0, 1):
        for plain, fused in ((M.dot(u, v), M.dot_contracted(u, v, variant)),
                             (M.cross(u, v), M.cross_contracted(u, v, variant)),
                             (M.project(u, v), M.project_contracted(u, v, variant))):
            differ = ~M.same_bits(plain, fused)
            differ = differ if differ.ndim == 1 else differ.any(axis=1)
            assert differ.mean() >= 0.5, (variant, differ.mean())
    # the exact-ops rule - bit for bit - rejects a contracted dot on the whole set of vector inputs
    u, v, s, _ = M.exact_vector_inputs()
    assert not M.same_bits(M.dot_contracted(u, v), M.dot(u, v)).all()


# ---- numpy's binary64 routines, the reference of the dense sweeps ----------------------------------------------------
@pytest.mark.parametrize("name", sorted(OPS))
def test_host_float_is_the_correctly_rounded_value(fixture, name):
    a, b, _ = _case(fixture, name)
    host = M.narrow(M.host64(OPS[name], a, b))
    held = fixture[name + "_margin"] > M.HOST_LOG2
    assert held.mean() > 0.95
    wrong = held & ~M.same_bits(host, M.from_bits(fixture[name + "_bits"]))
    assert not wrong.any(), [(float(x).hex(), None if b is None else float(b[i]).hex()) for i, x in enumerate(a) if wrong[i]][:5]
    # and elsewhere it is one of the two floats that bracket the exact value
    rule = M.fixture_rule(host, fixture[name + "_bits"], fixture[name + "_margin"], fixture[name + "_side"], M.HOST_LOG2)
    assert rule.all()


@pytest.mark.parametrize("name", sorted(OPS))
def test_host_binary64_is_within_two_ulps_of_mpmath(maker, fixture, name):
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.prec = maker.PRECISION
    a, b, _ = _case(fixture, name)
    host = M.host64(OPS[name], a, b)
    wa, wb = M.widen(a), np.zeros(len(a)) if b is None else M.widen(b)
    worst = 0.0
    for h, x, y in zip(host, wa, wb):
        exact = maker.exact(mpmath, OPS[name], x, y)
        if abs(exact) >= mpmath.mpf(2) ** 1024:             # outside binary64's normal range: infinite, or tiny
            assert np.isinf(h) and (h > 0) == (exact > 0), (x, y)
            continue
        if abs(exact) < mpmath.mpf(2) ** -1022:
            assert abs(h) <= 2.0 ** -1022, (x, y)
            continue
        assert np.isfinite(h), (x, y)
        worst = max(worst, float(abs(mpmath.mpf(float(h)) - exact) / mpmath.mpf(float(np.spacing(abs(h))))))
    print("%s: numpy binary64 at most %.3f ULP from mpmath on %d inputs" % (name, worst, len(a)))
    assert worst <= M.HOST_ULPS


def test_host_meets_the_special_value_table():
    """the hand-written C99 Annex F table against an implementation that is not under test"""
    broken = M.check_special_values(lambda op, a, b: M.narrow(M.host64(op, a, b)),
                                    ops=(M.POW_GENERAL, M.SIN, M.COS, M.ASIN, M.ATAN2))
    assert not broken, broken


# ---- the exclusion cap, on the references alone ------------------------------------------------------------------------
def test_exclusion_cap_on_the_fixture(fixture):
    for name, op in OPS.items():
        _, _, group = _case(fixture, name)
        # (the hard cases are not counted: cos(2^-12) = 1 - 2^-25 + 2^-50 / 6 sits 2^-52.6 from a midpoint by nature)
        counted = np.isin(group, [M.POW_GROUPS.index(g) for g in M.COUNTED_GROUPS]) if name == "pow" else group == 0
        assert counted.sum() >= 1200
        for which in ((M.POW, M.POW_GENERAL) if name == "pow" else (op,)):
            share = M.excluded_by_margin(fixture[name + "_margin"], M.BOUND_LOG2[which])[counted].mean()
            assert share <= M.EXCLUSION_CAP, (name, which, share)
    margin, group = fixture["pow_margin"], fixture["pow_group"]
    for apart in ("ties", "candidates"):                    # they exist to exercise the "either neighbour" rule
        assert M.excluded_by_margin(margin[group == M.POW_GROUPS.index(apart)], M.BOUND_LOG2[M.POW]).all()


@pytest.mark.parametrize("op", [M.POW, M.POW_GENERAL, M.SIN, M.COS, M.ATAN2, M.ASIN])
def test_exclusion_cap_on_the_sweep(op):
    a, b = M.sweep_inputs(op)
    assert len(a) == 1 << 20
    h = M.host64(op, a, b)
    excluded = M.sweep_excluded(h, 2.0 ** -41, 0) if op == M.POW else M.sweep_excluded(h, 0.0, M.BOUND_ULPS[op])
    print("op %d: %d of %d excluded" % (op, excluded.sum(), len(a)))
    assert excluded.mean() <= M.EXCLUSION_CAP
    if op == M.POW:
        assert M.lean_domain(a, b).all()                    # the sweep of pow_f stays on the lean path
        assert excluded.sum() > 0                           # (2^-41 of 2^-24: some thirty of 2^20)
    inside = np.isfinite(h) & (h != 0) & (np.abs(h) > 2.0 ** -126) & (np.abs(h) < 2.0 ** 127)
    assert inside.mean() > 0.5                              # most results are ordinary numbers


def test_boundary_distance():
    h = np.array([1.0, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 2.0 ** -150, 2.0 ** -149, 1.5 * 2.0 ** -149, 2.0 ** 128,
                  2.0 ** 128 - 2.0 ** 103, 3.0 * 2.0 ** -127, 3.5 * 2.0 ** -149 * 2.0])
    d, spacing = M.boundary_distance(h)
    assert d.tolist() == [2.0 ** -24, 0.0, 2.0 ** -50, 0.0, 2.0 ** -150, 0.0, 2.0 ** 103, 0.0, 2.0 ** -150, 2.0 ** -150]
    assert spacing[:3].tolist() == [2.0 ** -23] * 3 and spacing[3] == 2.0 ** -149


# ---- the emulation of pow_f's lean path, by the device's rule ----------------------------------------------------------
def _emulated(generator, a, b, **how):
    def one(x, y):
        if x == 0:
            return 0.0
        try:
            return generator.lean_pow(x, y, **how)
        except OverflowError:                               # math.ldexp raises where the device's ldexp returns infinity
            return np.inf
    return M.narrow(np.array([one(float(x), float(y)) for x, y in zip(M.widen(a), M.widen(b))]))


@pytest.fixture(scope="module")
def lean_inputs(fixture):
    a, b, group = _case(fixture, "pow")
    lean = M.lean_domain(a, b)
    assert lean.sum() > 7000
    keys = ("pow_bits", "pow_margin", "pow_side")
    return (a[lean], b[lean]) + tuple(fixture[k][lean] for k in keys)


def test_emulation_uses_the_degrees_of_the_device(generator):
    source = open(os.path.join(ROOT, "sol-r_amd", "csrc", "rt_device.h")).read()
    assert "hornerDown<6, POW_LOG_COEFFS>(scalarConstant<__builtin_bit_cast(unsigned long long, POW_LOG_COEFFS[7])>" in source
    assert "hornerDown<9, POW_EXP_COEFFS>(scalarConstant<__builtin_bit_cast(unsigned long long, POW_EXP_COEFFS[10])>" in source
    assert (generator.LOG_TERMS, generator.EXP_DEGREE) == (8, 10) and len(generator.LOG_C) == 8


def test_emulation_is_held_to_the_fixture(generator, lean_inputs):
    a, b, res, margin, side = lean_inputs
    got = _emulated(generator, a, b)
    ok = M.fixture_rule(got, res, margin, side, M.BOUND_LOG2[M.POW])
    assert ok.all(), [(float(x).hex(), float(y).hex()) for x, y in zip(a[~ok], b[~ok])][:8]
    differ = ~M.same_bits(got, M.from_bits(res))
    print("the emulation takes the other neighbour on %d of %d inputs" % (differ.sum(), len(a)))


def test_the_rule_rejects_a_table_entry_off_by_one(generator, lean_inputs):
    a, b, res, margin, side = lean_inputs
    table = list(generator.rows)
    invc, log2c = table[77]
    table[77] = (invc + 2.0 ** -28 * 2.0 ** np.floor(np.log2(invc)), log2c)       # one unit of invc's 28-bit last place
    got = _emulated(generator, a, b, table=table)
    bad = ~M.fixture_rule(got, res, margin, side, M.BOUND_LOG2[M.POW])
    idx = (M.bits(a).astype(np.int64) >> 16) & 0x7F
    assert bad.any() and (idx[bad] == 77).all()


def test_the_rule_rejects_a_shorter_exp2(generator, lean_inputs):
    a, b, res, margin, side = lean_inputs
    got = _emulated(generator, a, b, exp_degree=8)
    assert not M.fixture_rule(got, res, margin, side, M.BOUND_LOG2[M.POW]).all()


def test_the_table_is_reproducible(tmp_path):
    out = tmp_path / "pow_table.h"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_pow_table.py"), str(out)], check=True, capture_output=True)
    assert out.read_bytes() == open(os.path.join(ROOT, "sol-r_amd", "csrc", "pow_table.h"), "rb").read()
