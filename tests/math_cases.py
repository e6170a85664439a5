"""Inputs and CPU models for the device math stand-ins at the top of sol-r_amd/csrc/rt_device.h (test infrastructure).

Three things live here, none of which needs a GPU or anything but numpy:

* the numpy MODELS of the exact operations: binary32 in source order.  Every operation is the binary64 operation on
  the widened operands, rounded once to binary32: exact for + - x / sqrt because 53 >= 2 x 24 + 2 (double rounding is
  then innocuous).  Binary32 values enter and leave binary64 THROUGH THEIR BITS wherever they are subnormal
  (`widen`, `narrow`), so that a flush-to-zero or denormals-are-zero state of the host changes nothing;
* deterministic, seeded GENERATORS of inputs for the transcendental stand-ins (the hard cases and a few thousand random
  inputs per op - tests/golden/make_math_fixtures.py adds mpmath's answers and writes tests/golden/math_standins.npz),
  for the dense sweeps, for the exact ops, and the C99 Annex F table of special values;
* the RULES a result is held to: `fixture_rule` (the correctly rounded bits wherever the exact value is farther from a
  binary32 rounding boundary than the op's error bound, else either float that brackets it) and `sweep_excluded`
  (the same against numpy's binary64 value rounded once, which is what the oracle's rounded mode computes).
"""
import numpy as np

f32, f64, u32, i32, i64 = np.float32, np.float64, np.uint32, np.int32, np.int64

# ops of include/solr_hip_probes.h
POW, POW_GENERAL, SIN, COS, ATAN2, ASIN, SQRT, DIVIDE, RECIPROCAL, TO_INT = range(10)
V_ADD, V_SUB, V_SCALE, V_DOT, V_CROSS, V_LENGTH, V_NORMALIZE, V_DIVIDE, V_PROJECT, V_REFLECTION = range(10)

FLT_MIN, FLT_MAX = f32(1.17549435e-38), f32(3.40282347e38)
LEAN_A_LIMIT, LEAN_B_LIMIT = f32(3.0e38), f32(4096.0)
MIN_SUBNORMAL = np.array([1], np.uint32).view(np.float32)[0]

# Error bounds of the ops BEFORE their one rounding to binary32, as log2 of a relative error.  The lean path: the comment
# above pow_f.  The library routines: the OpenCL full-profile table for double (pow 16 ULP, sin / cos / asin 4, atan2 6),
# one binary64 ULP being at most 2^-52 relative: 16 -> 2^-48, 4 -> 2^-50, 6 (< 8) -> 2^-49.
BOUND_ULPS = {POW_GENERAL: 16, SIN: 4, COS: 4, ATAN2: 6, ASIN: 4}
BOUND_LOG2 = {POW: -41, POW_GENERAL: -48, SIN: -50, COS: -50, ATAN2: -49, ASIN: -50}
HOST_ULPS = 2             # what numpy's binary64 routines are held to (tests/test_math_fixture.py)
HOST_LOG2 = -51
EXCLUSION_CAP = 1e-4


# ---- binary32 <-> binary64 through the bits -------------------------------------------------------------------------
def bits(a):
    a = np.asarray(a, f32)
    return np.ascontiguousarray(a).view(u32).reshape(a.shape)


def from_bits(b):
    b = np.asarray(b, u32)
    return np.ascontiguousarray(b).view(f32).reshape(b.shape)


def widen(a):
    """binary32 -> binary64, exact; subnormals through their bits"""
    a = np.asarray(a, f32)
    b = bits(a).astype(i64)
    mantissa = (b & 0x7FFFFF).astype(f64)
    subnormal = ((b >> 23) & 0xFF) == 0
    sign = np.where((b >> 31) != 0, -1.0, 1.0)
    with np.errstate(all="ignore"):
        return np.where(subnormal, sign * (mantissa * 2.0 ** -149), a.astype(f64))


def narrow(d):
    """binary64 -> binary32, round to nearest even; subnormal results by integer rounding of the scaled value"""
    d = np.asarray(d, f64)
    with np.errstate(all="ignore"):
        r = d.astype(f32)
        small = np.abs(d) < 2.0 ** -126
        k = np.rint(np.where(small, np.abs(d), 0.0) * 2.0 ** 149).astype(i64)      # <= 2^23: FLT_MIN when it rounds up
    sub = from_bits((k | np.where(np.signbit(d), i64(1) << 31, i64(0))).astype(u32))
    return np.where(small, sub, r).astype(f32)


def ordered(b):
    """binary32 bits -> integers in the order of the values (-0 and +0 both 0)"""
    b = np.asarray(b, u32).astype(i64)
    return np.where(b >> 31 != 0, -(b & 0x7FFFFFFF), b)


def is_nan_bits(b):
    b = np.asarray(b, u32)
    return (b & u32(0x7FFFFFFF)) > u32(0x7F800000)


def same_bits(got, want):
    """bit for bit, NaN compared as NaN"""
    got, want = bits(got), bits(want)
    return (got == want) | (is_nan_bits(got) & is_nan_bits(want))


# ---- models of the exact ops ----------------------------------------------------------------------------------------
def _op(fn, *a):
    with np.errstate(all="ignore"):
        return narrow(fn(*[widen(x) for x in a]))


def add(a, b):
    return _op(np.add, a, b)


def sub(a, b):
    return _op(np.subtract, a, b)


def mul(a, b):
    return _op(np.multiply, a, b)


def div(a, b):
    return _op(np.divide, a, b)


def sqrt(a):
    return _op(np.sqrt, a)


def reciprocal(a):
    return div(np.ones_like(np.asarray(a, f32)), a)


def f2i(a):
    """the (int) cast as the oracle's f2i states it: truncate, saturate, NaN -> 0"""
    d = widen(a)
    with np.errstate(all="ignore"):
        t = np.trunc(np.where(np.isnan(d), 0.0, d))
    return np.clip(t, -2147483648.0, 2147483647.0).astype(i64).astype(i32)


def fma(a, b, c):
    """the fused a * b + c of binary32, correctly rounded: the product is exact in binary64, the sum is rounded TO ODD
    (TwoSum gives its error exactly), and 53 >= 24 + 2 bits make the second rounding the only one"""
    with np.errstate(all="ignore"):
        p, cc = widen(a) * widen(b), widen(c)
        s = p + cc
        t = s - p
        err = (p - (s - t)) + (cc - t)
        ok = np.isfinite(s) & np.isfinite(err) & (err != 0)
        sb = s.view(i64).copy()
        toward_zero = ok & (np.signbit(err) != np.signbit(s))       # the exact sum is nearer to zero than s
        sb = np.where(toward_zero, sb - 1, sb)
        sb = np.where(ok, sb | 1, sb)
        return narrow(sb.view(f64))


def _xyz(v):
    v = np.ascontiguousarray(v, f32)
    return v[:, 0], v[:, 1], v[:, 2]


def _vec(x, y, z):
    return np.stack([x, y, z], axis=1).astype(f32)


def v_add(u, v):
    return _vec(*[add(a, b) for a, b in zip(_xyz(u), _xyz(v))])


def v_sub(u, v):
    return _vec(*[sub(a, b) for a, b in zip(_xyz(u), _xyz(v))])


def v_scale(u, s):
    return _vec(*[mul(a, s) for a in _xyz(u)])


def v_divide(u, s):
    return _vec(*[div(a, s) for a in _xyz(u)])


def dot(u, v):
    (ax, ay, az), (bx, by, bz) = _xyz(u), _xyz(v)
    return add(add(mul(ax, bx), mul(ay, by)), mul(az, bz))


def cross(u, v):
    (bx, by, bz), (cx, cy, cz) = _xyz(u), _xyz(v)
    return _vec(sub(mul(by, cz), mul(bz, cy)), sub(mul(bz, cx), mul(bx, cz)), sub(mul(bx, cy), mul(by, cx)))


def length(u):
    return sqrt(dot(u, u))


def normalize(u):
    return v_scale(u, reciprocal(sqrt(dot(u, u))))


def project(a, b):
    return v_scale(b, div(dot(a, b), dot(b, b)))


def reflection(i, n):
    k = mul(np.full(len(i), 2.0, f32), dot(i, n))
    return v_sub(i, v_scale(n, k))


def _scalar_result(x):
    return _vec(x, np.zeros_like(x), np.zeros_like(x))


def vector_model(op, u, v, s):
    """what solr_hip_probe_vector_math must return: (n, 3) binary32"""
    return {V_ADD: lambda: v_add(u, v), V_SUB: lambda: v_sub(u, v), V_SCALE: lambda: v_scale(u, s),
            V_DOT: lambda: _scalar_result(dot(u, v)), V_CROSS: lambda: cross(u, v),
            V_LENGTH: lambda: _scalar_result(length(u)), V_NORMALIZE: lambda: normalize(u),
            V_DIVIDE: lambda: v_divide(u, s), V_PROJECT: lambda: project(u, v),
            V_REFLECTION: lambda: reflection(u, v)}[op]()


def scalar_model(op, a, b):
    """what solr_hip_probe_math must return for the exact ops: binary32 (the int's bits for TO_INT)"""
    return {SQRT: lambda: sqrt(a), DIVIDE: lambda: div(a, b), RECIPROCAL: lambda: reciprocal(a),
            TO_INT: lambda: f2i(a).view(f32)}[op]()


# what a compiler that contracts products into fused multiply-adds would compute instead (both ways round)
def dot_contracted(u, v, variant=0):
    (ax, ay, az), (bx, by, bz) = _xyz(u), _xyz(v)
    first = fma(ay, by, mul(ax, bx)) if variant == 0 else fma(ax, bx, mul(ay, by))
    return fma(az, bz, first)


def cross_contracted(u, v, variant=0):
    (bx, by, bz), (cx, cy, cz) = _xyz(u), _xyz(v)

    def one(p, q, r, s):                       # p * q - r * s
        if variant == 0:
            return fma(p, q, -mul(r, s))
        return fma(-r, s, mul(p, q))
    return _vec(one(by, cz, bz, cy), one(bz, cx, bx, cz), one(bx, cy, by, cx))


def project_contracted(a, b, variant=0):
    return v_scale(b, div(dot_contracted(a, b, variant), dot_contracted(b, b, variant)))


# ---- seeded inputs --------------------------------------------------------------------------------------------------
def _log_uniform(rng, n, lo_exp, hi_exp, signed=False):
    """binary32 values with exponent uniform in [lo_exp, hi_exp) and random significand bits"""
    e = rng.integers(lo_exp, hi_exp, n)
    m = rng.integers(0, 1 << 23, n)
    v = widen(from_bits((m | (127 << 23)).astype(u32))) * np.exp2(e.astype(f64))
    if signed:
        v = v * rng.choice([-1.0, 1.0], n)
    return narrow(v)


def _next(a, steps=1):
    """the binary32 value `steps` floats above (below for negative steps) in the order of the values; a > 0"""
    return from_bits((bits(a).astype(i64) + steps).astype(u32))


SPECULAR_POWERS = (80.0, 100.0, 200.0, 234.0)          # every specPower of sol-r_amd/scenes.py


def blinn_powers():
    """the exponents the Blinn term meets: the scenes' specular powers and fetchTexel's 1000.f * g / 256.f"""
    g = np.arange(1, 256).astype(f32)
    return np.concatenate([np.array(SPECULAR_POWERS, f32), div(mul(np.full(255, 1000.0, f32), g), np.full(255, 256.0, f32))])


# (a, b) in hex that a numpy emulation of the lean path rounded differently from (float)pow((double)a, (double)b)
POW_CANDIDATES = (("0x1.48a02ap-2", "0x1.237578p+6"), ("0x1.40bb52p-2", "0x1.4002b4p+4"), ("0x1.f14b66p-1", "0x1.1d04e2p+5"))

POW_GROUPS = ("random", "blinn", "table_edges", "near_one", "b_is_one", "exact", "ties", "result_edges", "domain_edges",
              "candidates")
COUNTED_GROUPS = ("random", "blinn")                   # the groups the exclusion cap is counted over


def pow_cases(seed=2301):
    """(a, b, group) - group indexes POW_GROUPS"""
    rng = np.random.default_rng(seed)
    out = []

    def put(name, a, b):
        a, b = np.asarray(a, f32).ravel(), np.asarray(b, f32).ravel()
        a, b = np.broadcast_arrays(a, b)
        out.append((a.astype(f32), b.astype(f32), np.full(len(a), POW_GROUPS.index(name), np.uint8)))

    # random: moderate bases with small exponents, bases around one with exponents up to 4096
    put("random", _log_uniform(rng, 1000, -20, 20), _log_uniform(rng, 1000, -8, 4))
    put("random", _log_uniform(rng, 1000, -1, 1), _log_uniform(rng, 1000, 0, 12))
    # the Blinn domain: a in (0, 1], thick near one where the term is visible
    u = rng.random(3000)
    a = np.where(np.arange(3000) % 3 == 0, 1.0 - u, 1.0 - 0.25 * u ** 3)
    powers = blinn_powers()
    put("blinn", narrow(a), powers[rng.integers(0, len(powers), 3000)])
    # every edge of the 128 table intervals, where |r| is largest: 1 + i/128 and the float just below it
    edge = narrow(1.0 + np.arange(128) / 128.0)
    for e, bs in ((-1, (234.0, 3.90625)), (0, (100.0, 0.3)), (1, (80.0, 7.8125)), (-100, (1.1,)), (60, (0.3,))):
        at = narrow(widen(edge) * 2.0 ** e)
        for b in bs:
            put("table_edges", np.concatenate([at, _next(at, -1)]), f32(b))
    one = f32(1.0)
    near = np.array([one, _next(one, -1), _next(one, 1)], f32)
    put("near_one", np.repeat(near, 3), np.tile(np.array([2.0 ** -20, 1.0, 4096.0], f32), 3))
    put("b_is_one", _log_uniform(rng, 200, -126, 127), one)
    # exact results: squares of <= 12-bit significands, square roots of perfect squares
    put("exact", narrow(rng.integers(1, 4096, 100) * np.exp2(rng.integers(-40, 40, 100).astype(f64))), f32(2.0))
    k = rng.integers(1, 4096, 100).astype(f64)
    put("exact", narrow(k * k * 4.0 ** rng.integers(-20, 20, 100)), f32(0.5))
    # exact ties: an odd 13-bit significand below sqrt(2) x 2^12 squares to an odd 25-bit one
    m = 2 * rng.integers(2049, 2896, 100) - 1
    put("ties", narrow(m * np.exp2(rng.integers(-30, 30, 100).astype(f64))), f32(2.0))
    # results around 2^-126, 2^-149 (and the underflow threshold 2^-150) and 2^128
    for target, lo, hi in ((-126.0, 0.3, 0.95), (-149.0, 0.3, 0.95), (-150.0, 0.3, 0.95), (128.0, 1.05, 3.0)):
        a = narrow(rng.uniform(lo, hi, 60))
        put("result_edges", a, narrow((target + rng.uniform(-0.7, 0.7, 60)) / np.log2(widen(a))))
    # the edges of the lean domain (each side of them)
    just_below = _next(LEAN_A_LIMIT, -1)
    aa = np.array([FLT_MIN, _next(FLT_MIN, -1), MIN_SUBNORMAL, just_below, LEAN_A_LIMIT, FLT_MAX, 0.0, 0.75, 1.5,
                   _next(one, -1), 2.0], f32)
    bb = np.array([MIN_SUBNORMAL, 2.0 ** -20, 0.5, 1.0, 2.0, 100.0, 4096.0, _next(LEAN_B_LIMIT, 1), 8192.0], f32)
    put("domain_edges", np.repeat(aa, len(bb)), np.tile(bb, len(aa)))
    put("candidates", [float.fromhex(c[0]) for c in POW_CANDIDATES], [float.fromhex(c[1]) for c in POW_CANDIDATES])
    return tuple(np.concatenate(x) for x in zip(*out))


TRIG_GROUPS = ("random", "near_half_pi", "powers_of_two", "tiny", "timestamps")


def trig_cases(seed=2302):
    """(a, group) for sin_f and cos_f"""
    rng = np.random.default_rng(seed)
    out = []

    def put(name, a):
        a = np.asarray(a, f32).ravel()
        out.append((a, np.full(len(a), TRIG_GROUPS.index(name), np.uint8)))

    put("random", _log_uniform(rng, 1200, -20, 20, signed=True))
    k = np.concatenate([np.arange(1, 201), rng.integers(201, 1000001, 600)]).astype(f64)
    put("near_half_pi", narrow(k * (np.pi / 2) * rng.choice([-1.0, 1.0], len(k))))
    put("powers_of_two", narrow(np.exp2(np.arange(-149, 128).astype(f64))))
    put("tiny", np.concatenate([from_bits(rng.integers(1, 1 << 23, 60).astype(u32)), -from_bits(rng.integers(1, 1 << 23, 20).astype(u32)),
                                _log_uniform(rng, 60, -126, -30, signed=True)]))
    # juliaSet: timestamp / 1500.f, timestamp / 2000.f; the procedural spheres add a coordinate to the time stamp
    t = np.concatenate([rng.integers(0, 1 << 31, 100), (2.0 ** rng.uniform(0, 31, 100)).astype(i64),
                        [0, 1, 1499, 1500, 2000, (1 << 31) - 1]]).astype(i32)
    tf = t.astype(f32)                                     # (int -> float, correctly rounded)
    put("timestamps", np.concatenate([div(tf, np.full(len(tf), 1500.0, f32)), div(tf, np.full(len(tf), 2000.0, f32)),
                                      add(tf[:100], narrow(rng.uniform(-500, 500, 100)))]))
    return tuple(np.concatenate(x) for x in zip(*out))


ASIN_GROUPS = ("random", "at_one", "tiny", "near_one")


def asin_cases(seed=2303):
    rng = np.random.default_rng(seed)
    one = f32(1.0)
    at_one = np.array([one, -one, _next(one, -1), -_next(one, -1), _next(one, -2), -_next(one, -2), 0.5, -0.5], f32)
    tiny = np.concatenate([narrow(np.exp2(np.arange(-149, 0).astype(f64))), _log_uniform(rng, 100, -140, -10, signed=True),
                           -from_bits(rng.integers(1, 1 << 23, 20).astype(u32))])
    near = narrow((1.0 - np.exp2(-rng.uniform(1, 24, 300))) * rng.choice([-1.0, 1.0], 300))
    parts = (narrow(rng.uniform(-1, 1, 1500)), at_one, tiny, near)
    return (np.concatenate(parts).astype(f32),
            np.concatenate([np.full(len(p), i, np.uint8) for i, p in enumerate(parts)]))


ATAN2_GROUPS = ("random", "a_much_smaller", "a_much_larger", "subnormal")


def atan2_cases(seed=2304):
    """(a, b, group) for atan2_f(a, b): a is the ordinate"""
    rng = np.random.default_rng(seed)
    parts = [(_log_uniform(rng, 1500, -30, 30, True), _log_uniform(rng, 1500, -30, 30, True)),
             (_log_uniform(rng, 300, -126, -100, True), _log_uniform(rng, 300, 0, 40, True)),      # results down to subnormal
             (_log_uniform(rng, 300, 0, 100, True), _log_uniform(rng, 300, -126, -20, True)),
             (from_bits(rng.integers(1, 1 << 23, 100).astype(u32)) * rng.choice([-1, 1], 100).astype(f32),
              np.concatenate([from_bits(rng.integers(1, 1 << 23, 50).astype(u32)), _log_uniform(rng, 50, -10, 10, True)]))]
    return (np.concatenate([p[0] for p in parts]).astype(f32), np.concatenate([p[1] for p in parts]).astype(f32),
            np.concatenate([np.full(len(p[0]), i, np.uint8) for i, p in enumerate(parts)]))


def sweep_inputs(op, n=1 << 20, seed=2310):
    """the dense sweep's inputs for one op: (a, b)"""
    rng = np.random.default_rng(seed + op)
    zero = np.zeros(n, f32)
    if op in (POW, POW_GENERAL):
        # half in the Blinn domain (bases in [0.3, 1), powers in [1, 300] or one of the scenes' / a texture's), half wider
        h = n // 2
        powers = blinn_powers()
        b1 = np.where(rng.random(h) < 0.5, narrow(rng.uniform(1.0, 300.0, h)), powers[rng.integers(0, len(powers), h)])
        a = np.concatenate([narrow(rng.uniform(0.3, 1.0, h)), _log_uniform(rng, n - h, -4, 4)])
        b = np.concatenate([b1.astype(f32), _log_uniform(rng, n - h, -6, 5)])
        return a, b
    if op in (SIN, COS):
        return _log_uniform(rng, n, -12, 22, signed=True), zero
    if op == ASIN:
        return narrow(rng.uniform(-1.0, 1.0, n)), zero
    if op == ATAN2:
        return _log_uniform(rng, n, -20, 20, True), _log_uniform(rng, n, -20, 20, True)
    raise KeyError(op)


def host64(op, a, b=None):
    """numpy's binary64 routine on the widened inputs: what the oracle's rounded mode evaluates before it rounds once"""
    x = widen(a)
    with np.errstate(all="ignore"):
        if op in (POW, POW_GENERAL):
            return np.power(x, widen(b))
        if op == ATAN2:
            return np.arctan2(x, widen(b))
        return {SIN: np.sin, COS: np.cos, ASIN: np.arcsin}[op](x)


def lean_domain(a, b):
    """the inputs pow_f keeps on its lean path (a wave of nothing else), +0 bases included"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    with np.errstate(all="ignore"):
        ok_b = (widen(b) > 0) & (b <= LEAN_B_LIMIT)
        return (((widen(a) >= widen(FLT_MIN)) & (a < LEAN_A_LIMIT)) | (bits(a) == 0)) & ok_b


# ---- exact ops: inputs ---------------------------------------------------------------------------------------------
SPECIALS32 = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 3.0e38, -3.0e38, 1.0e-38, 1.4e-45, -1.4e-45], f32)


def exact_scalar_inputs(op, seed=2320):
    """(a, b) for SQRT, DIVIDE, RECIPROCAL and TO_INT: subnormal inputs and results, perfect squares +- 1 ulp, quotients
    that land in the subnormal range (ties included), +-0, inf, NaN, casts out of range"""
    rng = np.random.default_rng(seed + op)
    sub = from_bits(rng.integers(1, 1 << 23, 200).astype(u32))
    if op == SQRT:
        k = rng.integers(1, 4096, 200).astype(f64)
        sq = narrow(k * k * 4.0 ** rng.integers(-60, 50, 200))         # (finite: at most 2^24 x 4^49)
        a = np.concatenate([_log_uniform(rng, 2000, -126, 128), sub, sq, _next(sq, 1), _next(sq, -1),
                            narrow(np.exp2(np.arange(-149, 128).astype(f64))), SPECIALS32, [-4.0, -1e-40]])
        return a.astype(f32), np.zeros(len(a), f32)
    if op == RECIPROCAL:
        a = np.concatenate([_log_uniform(rng, 2000, -126, 128, True), sub, -sub,
                            _log_uniform(rng, 400, 126, 128, True),            # reciprocals in the subnormal range
                            narrow(np.exp2(np.arange(-149, 128).astype(f64))), SPECIALS32])
        return a.astype(f32), np.zeros(len(a), f32)
    if op == DIVIDE:
        a1, b1 = _log_uniform(rng, 2000, -126, 128, True), _log_uniform(rng, 2000, -126, 128, True)
        a2, b2 = _log_uniform(rng, 800, -126, -100, True), _log_uniform(rng, 800, 10, 40, True)      # subnormal quotients
        # ties in the subnormal range: (2 k + 1) x 2^-149 x 2^(j - 1) over 2^j is half way between two subnormals
        kk = (2 * rng.integers(0, 1 << 20, 200) + 1).astype(f64)
        j = rng.integers(1, 40, 200).astype(f64)
        a3, b3 = narrow(kk * 2.0 ** -149 * np.exp2(j - 1)), narrow(np.exp2(j))
        a4, b4 = np.repeat(SPECIALS32, len(SPECIALS32)), np.tile(SPECIALS32, len(SPECIALS32))
        return (np.concatenate([a1, a2, a3, sub, a4]).astype(f32),
                np.concatenate([b1, b2, b3, _log_uniform(rng, 200, -3, 3, True), b4]).astype(f32))
    if op == TO_INT:
        edge = f32(2147483648.0)
        a = np.concatenate([narrow(rng.uniform(-5000, 5000, 1500)), _log_uniform(rng, 600, -10, 40, True), sub,
                            [edge, -edge, _next(edge, -1), -_next(edge, -1), _next(edge, 1), -_next(edge, 1), 4294967296.0,
                             -4294967296.0, 0.99999994, -0.99999994, 1e10, -1e10, 3e38, -3e38, 0.5, -0.5, 2.5, -2.5],
                            SPECIALS32])
        return a.astype(f32), np.zeros(len(a), f32)
    raise KeyError(op)


def contraction_vectors(n=1024, seed=2330):
    """(u, v, s): n vectors on EVERY one of which the source-order dot(u, v), cross(u, v) and project(u, v) each differ from
    both fused evaluations - found by search, so a contracted build cannot hide - and the special vectors behind them"""
    rng = np.random.default_rng(seed)
    us, vs, have = [], [], 0
    while have < n:
        u = narrow(rng.uniform(-4, 4, (4 * n, 3)) * np.exp2(rng.integers(-3, 4, (4 * n, 1)).astype(f64)))
        v = narrow(rng.uniform(-4, 4, (4 * n, 3)) * np.exp2(rng.integers(-3, 4, (4 * n, 1)).astype(f64)))
        keep = np.ones(len(u), bool)
        for variant in (0, 1):
            keep &= bits(dot(u, v)) != bits(dot_contracted(u, v, variant))
            keep &= (bits(cross(u, v)) != bits(cross_contracted(u, v, variant))).any(axis=1)
            keep &= (bits(project(u, v)) != bits(project_contracted(u, v, variant))).any(axis=1)
        us.append(u[keep])
        vs.append(v[keep])
        have += int(keep.sum())
    u, v = np.concatenate(us)[:n], np.concatenate(vs)[:n]
    return u, v, _log_uniform(rng, n, -4, 4, True)


def exact_vector_inputs(seed=2331):
    """(u, v, s, nb_contraction): the searched vectors first, then random ones over the whole range, subnormal components
    and results, and the special values"""
    rng = np.random.default_rng(seed)
    u0, v0, s0 = contraction_vectors()
    n = 1500
    u1, v1 = _log_uniform(rng, 3 * n, -40, 40, True).reshape(n, 3), _log_uniform(rng, 3 * n, -40, 40, True).reshape(n, 3)
    s1 = _log_uniform(rng, n, -40, 40, True)
    m = 400                                                 # products, sums and quotients in the subnormal range
    u2, v2 = _log_uniform(rng, 3 * m, -100, -60, True).reshape(m, 3), _log_uniform(rng, 3 * m, -75, -55, True).reshape(m, 3)
    s2 = _log_uniform(rng, m, -60, 60, True)
    u3 = (from_bits(rng.integers(1, 1 << 23, 3 * m).astype(u32)) * rng.choice([-1, 1], 3 * m).astype(f32)).reshape(m, 3)
    v3 = _log_uniform(rng, 3 * m, -2, 2, True).reshape(m, 3)
    s3 = _log_uniform(rng, m, -2, 2, True)
    k = len(SPECIALS32)
    u4 = np.stack([np.repeat(SPECIALS32, k), np.tile(SPECIALS32, k), np.full(k * k, 1.5, f32)], axis=1)
    v4 = np.stack([np.tile(SPECIALS32, k), np.full(k * k, -2.0, f32), np.repeat(SPECIALS32, k)], axis=1)
    s4 = np.tile(SPECIALS32, k)
    return (np.concatenate([u0, u1, u2, u3, u4]).astype(f32), np.concatenate([v0, v1, v2, v3, v4]).astype(f32),
            np.concatenate([s0, s1, s2, s3, s4]).astype(f32), len(u0))


# ---- C99 Annex F: special values -------------------------------------------------------------------------------------
def special_values():
    """[(op, a, b, expected)]: expected is a binary32 value held bit for bit (its sign included), or None for a NaN"""
    inf, nan = np.inf, np.nan
    pi = float(narrow(np.pi))                      # what (float) makes of the binary64 constant
    pi2, pi4, pi34 = float(narrow(np.pi / 2)), float(narrow(np.pi / 4)), float(narrow(3 * np.pi / 4))
    T = []
    for op in (POW, POW_GENERAL):
        for x in (2.0, -3.0, 0.0, -0.0, inf, -inf, nan, 1e-40):          # F.10.4.4: pow(x, +-0) is 1, even for a NaN
            T += [(op, x, 0.0, 1.0), (op, x, -0.0, 1.0)]
        for y in (3.0, -2.5, 0.0, inf, -inf, nan, 1e-40):                # pow(+1, y) is 1, even for a NaN
            T.append((op, 1.0, y, 1.0))
        T += [(op, nan, 1.0, None), (op, nan, -2.0, None), (op, 2.0, nan, None), (op, -2.0, nan, None), (op, nan, nan, None)]
        T += [(op, -2.0, 2.0, 4.0), (op, -2.0, 3.0, -8.0), (op, -2.0, -2.0, 0.25), (op, -2.0, -3.0, -0.125),
              (op, -2.0, 0.5, None), (op, -8.0, 1.0 / 3.0, None), (op, -0.5, 2.5, None), (op, -1e-40, 0.5, None)]
        T += [(op, 0.0, -3.0, inf), (op, -0.0, -3.0, -inf), (op, 0.0, -2.0, inf), (op, -0.0, -2.0, inf),
              (op, 0.0, -2.5, inf), (op, -0.0, -2.5, inf), (op, 0.0, 3.0, 0.0), (op, -0.0, 3.0, -0.0),
              (op, 0.0, 2.0, 0.0), (op, -0.0, 2.0, 0.0), (op, 0.0, 2.5, 0.0), (op, -0.0, 2.5, 0.0),
              (op, 0.0, -inf, inf), (op, -0.0, -inf, inf), (op, 0.0, inf, 0.0), (op, -0.0, inf, 0.0)]
        T += [(op, -1.0, inf, 1.0), (op, -1.0, -inf, 1.0),
              (op, 0.5, -inf, inf), (op, -0.5, -inf, inf), (op, 2.0, -inf, 0.0), (op, -2.0, -inf, 0.0),
              (op, 0.5, inf, 0.0), (op, -0.5, inf, 0.0), (op, 2.0, inf, inf), (op, -2.0, inf, inf)]
        T += [(op, -inf, -3.0, -0.0), (op, -inf, -2.0, 0.0), (op, -inf, -2.5, 0.0), (op, -inf, 3.0, -inf),
              (op, -inf, 2.0, inf), (op, -inf, 2.5, inf), (op, inf, -3.0, 0.0), (op, inf, -0.5, 0.0), (op, inf, 3.0, inf),
              (op, inf, 0.5, inf), (op, inf, inf, inf), (op, inf, -inf, 0.0), (op, -inf, inf, inf), (op, -inf, -inf, 0.0)]
    T += [(SIN, inf, 0, None), (SIN, -inf, 0, None), (SIN, nan, 0, None), (SIN, -0.0, 0, -0.0), (SIN, 0.0, 0, 0.0),
          (COS, inf, 0, None), (COS, -inf, 0, None), (COS, nan, 0, None), (COS, -0.0, 0, 1.0), (COS, 0.0, 0, 1.0)]
    T += [(ASIN, 1.5, 0, None), (ASIN, -1.0000001, 0, None), (ASIN, inf, 0, None), (ASIN, -inf, 0, None), (ASIN, nan, 0, None),
          (ASIN, -0.0, 0, -0.0), (ASIN, 0.0, 0, 0.0), (ASIN, 1.0, 0, pi2), (ASIN, -1.0, 0, -pi2)]
    T += [(ATAN2, 0.0, -0.0, pi), (ATAN2, -0.0, -0.0, -pi), (ATAN2, 0.0, 0.0, 0.0), (ATAN2, -0.0, 0.0, -0.0),
          (ATAN2, 0.0, -2.0, pi), (ATAN2, -0.0, -2.0, -pi), (ATAN2, 0.0, 2.0, 0.0), (ATAN2, -0.0, 2.0, -0.0),
          (ATAN2, -3.0, 0.0, -pi2), (ATAN2, -3.0, -0.0, -pi2), (ATAN2, 3.0, 0.0, pi2), (ATAN2, 3.0, -0.0, pi2),
          (ATAN2, 3.0, -inf, pi), (ATAN2, -3.0, -inf, -pi), (ATAN2, 3.0, inf, 0.0), (ATAN2, -3.0, inf, -0.0),
          (ATAN2, 0.0, -inf, pi), (ATAN2, -0.0, -inf, -pi), (ATAN2, 0.0, inf, 0.0), (ATAN2, -0.0, inf, -0.0),
          (ATAN2, inf, 3.0, pi2), (ATAN2, -inf, 3.0, -pi2), (ATAN2, inf, -3.0, pi2), (ATAN2, -inf, -3.0, -pi2),
          (ATAN2, inf, 0.0, pi2), (ATAN2, -inf, -0.0, -pi2),
          (ATAN2, inf, -inf, pi34), (ATAN2, -inf, -inf, -pi34), (ATAN2, inf, inf, pi4), (ATAN2, -inf, inf, -pi4),
          (ATAN2, nan, 1.0, None), (ATAN2, 1.0, nan, None), (ATAN2, nan, nan, None), (ATAN2, nan, inf, None), (ATAN2, 0.0, nan, None)]
    return T


def check_special_values(evaluate, ops=None):
    """evaluate(op, a, b) -> binary32 array; returns the rows of the table that are broken"""
    table = [row for row in special_values() if ops is None or row[0] in ops]
    broken = []
    for op in sorted({row[0] for row in table}):
        rows = [row for row in table if row[0] == op]
        got = bits(evaluate(op, np.array([r[1] for r in rows], f32), np.array([r[2] for r in rows], f32)))
        for row, g in zip(rows, got):
            want = row[3]
            ok = bool(is_nan_bits(g)) if want is None else int(g) == int(bits(f32(want))[()])
            if not ok:
                broken.append((row, hex(int(g))))
    return broken


# ---- the rules -------------------------------------------------------------------------------------------------------
def neighbour(correct_bits, side):
    """the other float that brackets the exact value: one step from the correctly rounded one towards it (side = the
    sign of exact - rounded; 0 where the result is exact, and then the result itself)"""
    b = np.asarray(correct_bits, u32).astype(i64)
    magnitude, sign = b & 0x7FFFFFFF, b & 0x80000000
    away = np.where(sign != 0, -np.asarray(side, i64), np.asarray(side, i64))      # +1: away from zero
    return (sign | np.clip(magnitude + away, 0, 0x7F800000)).astype(u32)


def fixture_rule(got, correct_bits, margin, side, bound_log2):
    """boolean array: the result passes.  The correctly rounded bits wherever the stored margin exceeds the bound (the
    margin is floor(log2(relative distance to the nearest rounding boundary))), else either bracketing float"""
    got = bits(got)
    correct_bits = np.asarray(correct_bits, u32)
    exactly = (got == correct_bits) | (is_nan_bits(got) & is_nan_bits(correct_bits))
    loose = np.asarray(margin, np.int16) <= bound_log2
    return exactly | (loose & (got == neighbour(correct_bits, side)))


def excluded_by_margin(margin, bound_log2):
    return np.asarray(margin, np.int16) <= bound_log2


def boundary_distance(h):
    """|h| as a binary64 array -> (distance from |h| to the nearest midpoint of adjacent binary32 values, the spacing of
    binary32 there), both exact in binary64.  Subnormal spacing below 2^-126; above FLT_MAX the one boundary is
    2^128 - 2^103."""
    h = np.abs(np.asarray(h, f64))
    with np.errstate(all="ignore"):
        e = np.clip(np.floor(np.log2(np.where((h > 0) & np.isfinite(h), h, 1.0))), -126, 127)
        e = np.where(np.exp2(e) > h, e - 1, e)                       # (log2 rounded up across a power of two)
        e = np.where(np.exp2(e + 1) <= h, e + 1, e)
        e = np.clip(e, -126, 127)
        spacing = np.exp2(e - 23)
        q = h / spacing                                              # exact: a power of two
        frac = q - np.floor(q)
        d = np.abs(frac - 0.5) * spacing
        top = 2.0 ** 128 - 2.0 ** 103
        d = np.where(h >= 2.0 ** 128, h - top, d)
    return d, spacing


def sweep_excluded(h, rel_bound=0.0, ulps=0):
    """the dense sweep's exclusion: the host's binary64 value h lies within (the op's bound + HOST_ULPS binary64 ULPs) of
    a binary32 rounding boundary.  The op's bound is rel_bound x |h| or `ulps` binary64 ULPs."""
    h = np.asarray(h, f64)
    d, _ = boundary_distance(h)
    with np.errstate(all="ignore"):
        ulp = np.spacing(np.abs(h))
        reach = rel_bound * np.abs(h) + (ulps + HOST_ULPS) * ulp
        return np.isfinite(h) & (h != 0) & (d <= reach)
