"""The device math stand-ins at the top of sol-r_amd/csrc/rt_device.h, per element, against references that do not come
from the code under test.

Every parity claim of the project rests on pow_f (with its lean table path) and pow_general, sin_f, cos_f, atan2_f, asin_f,
sqrt_ieee, the correctly rounded divide, normalize / length, the v3 operators built without contraction and the plain (int)
casts of the texture mappers: the oracle's exact mode evaluates the same calls in binary64 on the host, rounds once, and the
frames are compared exactly.  Here the functions themselves run on the device over arrays of inputs, through
solr_hip_probe_math / solr_hip_probe_vector_math (include/solr_hip_probes.h; element e is lane e % 64 of wave e // 64).

BOUNDS: the relative error of an op before its one rounding to binary32 (tests/math_cases.py BOUND_LOG2 / BOUND_ULPS).
  * the lean path of pow_f: 2^-41, the figure of the comment above pow_f;
  * the binary64 library routines behind pow_general, sin_f, cos_f, asin_f, atan2_f: the OpenCL full-profile table for
    double - pow 16 ULP, sin / cos / asin 4, atan2 6 (binary64 ULPs).  The ROCm installation this was written against
    documents no figures of its own for its device library, so that table is the source.
None of them was tuned to what the device returns.

THE FIXTURE (tests/golden/math_standins.npz: mpmath at 256 bits, tests/golden/make_math_fixtures.py): the device's bits equal
the correctly rounded bits wherever the exact value is farther from a binary32 rounding boundary than the op's bound;
elsewhere the result is one of the two floats that bracket the exact value.
THE DENSE SWEEP: 2^20 seeded inputs per op against numpy's binary64 routine rounded once - what the oracle's rounded mode
computes; tests/test_math_fixture.py holds numpy to 2 binary64 ULPs of mpmath.  An input is excluded when the host's
binary64 value lies within (op bound + 2) binary64 ULPs of a rounding boundary; no other input may differ, and at most
1e-4 of the inputs may be excluded.
WAVE COMPOSITION: pow_f sends a whole wave to pow_general when one lane is outside the lean domain.
THE EXACT OPS equal the numpy models of tests/math_cases.py bit for bit (NaN compared as NaN).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_probes as E  # noqa: E402
import math_cases as M  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "math_standins.npz")
NAMES = {M.POW: "pow_f", M.POW_GENERAL: "pow_general", M.SIN: "sin_f", M.COS: "cos_f", M.ATAN2: "atan2_f", M.ASIN: "asin_f"}
STEM = {M.POW: "pow", M.POW_GENERAL: "pow", M.SIN: "sin", M.COS: "cos", M.ATAN2: "atan2", M.ASIN: "asin"}
TRANSCENDENTAL = sorted(NAMES)


@pytest.fixture(scope="module")
def hip(solr):
    lib = solr.hip_lib()
    lib.solr_hip_clear_error()
    return lib


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(FIXTURE))


def _hex(a, b, where, limit=4):
    return ["(%s, %s)" % (float(a[i]).hex(), float(b[i]).hex()) for i in np.flatnonzero(where)[:limit]]


@pytest.mark.parametrize("op", TRANSCENDENTAL)
def test_fixture(hip, fixture, op):
    stem = STEM[op]
    a = fixture[("trig" if stem in ("sin", "cos") else stem) + "_a"]
    b = fixture.get(stem + "_b", np.zeros(len(a), M.f32))
    want, margin, side = (fixture[stem + k] for k in ("_bits", "_margin", "_side"))
    if op == M.POW:
        # waves of nothing but lean inputs, held to the lean bound; the rest goes to the library routine whatever its wave
        lean = M.lean_domain(a, b)
        got, bound = np.zeros(len(a), M.f32), np.where(lean, M.BOUND_LOG2[M.POW], M.BOUND_LOG2[M.POW_GENERAL])
        got[lean] = E.probe_math(hip, op, a[lean], b[lean])
        got[~lean] = E.probe_math(hip, op, a[~lean], b[~lean])
        assert lean.sum() > 7000 and (~lean).sum() > 20
    else:
        got, bound = E.probe_math(hip, op, a, b), np.full(len(a), M.BOUND_LOG2[op])
    ok = M.fixture_rule(got, want, margin, side, bound)
    loose = M.excluded_by_margin(margin, bound)
    other = ~M.same_bits(got, M.from_bits(want))
    print("math_standins: %-11s fixture: %5d inputs, %3d within the bound of a boundary (either neighbour), %3d not the "
          "correctly rounded value, %d outside the rule" % (NAMES[op], len(a), loose.sum(), other.sum(), (~ok).sum()))
    assert ok.all(), _hex(a, b, ~ok, 8)


@pytest.mark.parametrize("op", TRANSCENDENTAL)
def test_dense_sweep(hip, op):
    a, b = M.sweep_inputs(op)
    h = M.host64(op, a, b)
    want = M.narrow(h)
    got = E.probe_math(hip, op, a, b)
    excluded = M.sweep_excluded(h, 2.0 ** -41, 0) if op == M.POW else M.sweep_excluded(h, 0.0, M.BOUND_ULPS[op])
    differ = ~M.same_bits(got, want)
    print("math_standins: %-11s sweep: %d inputs, %d excluded, %d differ from the host stand-in %s" % (
        NAMES[op], len(a), excluded.sum(), differ.sum(), " ".join(_hex(a, b, differ))))
    assert not (differ & ~excluded).any(), _hex(a, b, differ & ~excluded, 8)
    assert excluded.mean() <= M.EXCLUSION_CAP
    # an excluded input is still one of the two neighbours
    assert (np.abs(M.ordered(M.bits(got)) - M.ordered(M.bits(want)))[differ] <= 1).all()


def _out_of_domain(a, b):
    """lane j(w) of every wave w replaced by an input outside the lean domain: b = 0, b = 8192, a subnormal, a negative,
    a NaN in turn, j moving through the wave"""
    a, b = a.copy(), b.copy()
    waves = len(a) // 64
    lane = (np.arange(waves) * 7 + 3) % 64
    at = np.arange(waves) * 64 + lane
    kind = np.arange(waves) % 5
    b[at[kind == 0]] = 0.0
    b[at[kind == 1]] = 8192.0
    a[at[kind == 2]] = M.from_bits(np.uint32(0x00400001))
    a[at[kind == 3]] = -a[at[kind == 3]]
    a[at[kind == 4]] = np.nan
    assert len(set(lane.tolist())) == 64 and not M.lean_domain(a[at], b[at]).any()
    touched = np.zeros(len(a), bool)
    touched[at] = True
    return a, b, touched


def test_wave_composition(hip):
    n = 64 * 1280
    a, b = (x[:n].copy() for x in M.sweep_inputs(M.POW))
    assert M.lean_domain(a, b).all()
    lean = E.probe_math(hip, M.POW, a, b)                          # A: pure lean waves
    a2, b2, touched = _out_of_domain(a, b)
    mixed = E.probe_math(hip, M.POW, a2, b2)                       # B: one lane of every wave out of the domain
    general = E.probe_math(hip, M.POW_GENERAL, a, b)               # C: the library routine on the original inputs
    general2 = E.probe_math(hip, M.POW_GENERAL, a2, b2)
    # the ballot reroutes the whole wave and nothing else changes
    assert M.same_bits(mixed, general)[~touched].all()
    assert M.same_bits(mixed, general2).all()
    # lean and general agree outside the inputs where their two bounds let them differ
    h = M.host64(M.POW, a, b)
    excluded = M.sweep_excluded(h, 2.0 ** -41, M.BOUND_ULPS[M.POW_GENERAL])
    differ = ~M.same_bits(lean, general)
    print("math_standins: pow_f lean against pow_general: %d inputs, %d excluded, %d lanes differ %s" % (
        n, excluded.sum(), differ.sum(), " ".join(_hex(a, b, differ))))
    assert not (differ & ~excluded).any(), _hex(a, b, differ & ~excluded, 8)
    assert (np.abs(M.ordered(M.bits(lean)) - M.ordered(M.bits(general)))[differ] <= 1).all()
    # inactive lanes take no part in the ballot: a partial last wave gives the bits the full waves gave
    for count in (1, 63, 65, 127):
        assert M.same_bits(E.probe_math(hip, M.POW, a[:count], b[:count]), lean[:count]).all(), count
        part = E.probe_math(hip, M.POW, a2[:count], b2[:count])
        # a wave keeps to the library routine only while its out-of-domain lane is among the active ones
        whole = np.zeros(count, bool)
        for w in range(0, count, 64):
            whole[w:w + 64] = touched[w:min(w + 64, count)].any()
        assert M.same_bits(part, np.where(whole, general2[:count], lean[:count])).all(), count


def test_special_values(hip):
    broken = M.check_special_values(lambda op, a, b: E.probe_math(hip, op, a, b))
    print("math_standins: special values: %d rows, %d broken" % (len(M.special_values()), len(broken)))
    assert not broken, broken
    # the same rows of pow_f one to a wave, 63 lean lanes around each: the wave goes to the library routine or, where the
    # row is in the lean domain itself (pow(1, 3), pow(+0, 3)), stays
    rows = [r for r in M.special_values() if r[0] == M.POW]
    a = np.full((len(rows), 64), 0.75, M.f32)
    b = np.full((len(rows), 64), 100.0, M.f32)
    lane = (np.arange(len(rows)) * 5 + 1) % 64
    a[np.arange(len(rows)), lane] = [r[1] for r in rows]
    b[np.arange(len(rows)), lane] = [r[2] for r in rows]
    got = M.bits(E.probe_math(hip, M.POW, a.ravel(), b.ravel())).reshape(-1, 64)[np.arange(len(rows)), lane]
    for r, g in zip(rows, got):
        assert M.is_nan_bits(g) if r[3] is None else int(g) == int(M.bits(M.f32(r[3]))), (r, hex(int(g)))


@pytest.mark.parametrize("op", [M.SQRT, M.DIVIDE, M.RECIPROCAL, M.TO_INT])
def test_exact_scalar_ops(hip, op):
    a, b = M.exact_scalar_inputs(op)
    got, want = E.probe_math(hip, op, a, b), M.scalar_model(op, a, b)
    same = M.same_bits(got, want)
    subnormal = ((M.bits(want) & 0x7F800000) == 0) & ((M.bits(want) & 0x7FFFFF) != 0)
    print("math_standins: exact scalar op %d: %d inputs (%d subnormal results), %d differ" % (op, len(a), subnormal.sum(), (~same).sum()))
    assert op == M.TO_INT or subnormal.sum() >= (0 if op == M.SQRT else 200)
    assert same.all(), ["%s %s -> %s, model %s" % (float(a[i]).hex(), float(b[i]).hex(), hex(int(M.bits(got)[i])),
                                                   hex(int(M.bits(want)[i]))) for i in np.flatnonzero(~same)[:8]]


@pytest.mark.parametrize("op", range(10))
def test_exact_vector_ops(hip, op):
    u, v, s, _ = M.exact_vector_inputs()
    got, want = E.probe_vector_math(hip, op, u, v, s), M.vector_model(op, u, v, s)
    same = M.same_bits(got, want).all(axis=1)
    print("math_standins: exact vector op %d: %d inputs, %d differ" % (op, len(s), (~same).sum()))
    assert same.all(), [(u[i].tolist(), v[i].tolist(), float(s[i]), got[i].tolist(), want[i].tolist()) for i in np.flatnonzero(~same)[:4]]


def test_an_unknown_op_is_an_error(hip):
    one = np.ones(3, M.f32)
    out = np.zeros(3, M.f32)
    buf = C.create_string_buffer(256)
    for call in (lambda: hip.solr_hip_probe_math(10, 1, E._p(one), E._p(one), E._p(out)),
                 lambda: hip.solr_hip_probe_math(-1, 1, E._p(one), E._p(one), E._p(out)),
                 lambda: hip.solr_hip_probe_vector_math(10, 1, E._p(one), E._p(one), E._p(one), E._p(out))):
        E.declare(hip)
        hip.solr_hip_clear_error()
        assert call() == -1
        assert hip.solr_hip_last_error(buf, 256) != 0 and b"op" in buf.value
        hip.solr_hip_clear_error()
    assert (out == 0).all()
