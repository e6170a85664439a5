"""A model of the texture tier written from the reference's text alone (test infrastructure, plain Python + numpy + mpmath).

What it restates, statement by statement and in source order: TextureMapping.cuh:30-456 ("TM": the six secondary maps, the
two fractals, the triangle, sphere and cube mappers, wireFrameMapping), GeometryShaders.cuh:36-124 ("GS": intersectionShader
with its dispatch by primitive type and the untextured checkerboard), GeometryIntersections.cuh:87-151 ("GI": skyboxMapping)
and GI:430-561 (planeIntersection with the wireframe, the emissive YZ pattern, the textured plane's colour key and
shadowIntensity = color.w).  It shares no code with the engine's device functions or with the C oracle, and reads neither.

Arithmetic.  Every float is a binary32 `np.float32` SCALAR and every operation one numpy scalar operation, in the order the
text writes them (no contraction); the one binary64 expression is the Mandelbrot set's imaginary pitch (TM:172-175).
Integers are Python ints wrapped to 32 bits after every operation (`wrap`).  `%` is C's truncating remainder (`crem`).
Float -> int is the DEVICE's conversion (`Model.to_int`): truncate, saturate at both ends, NaN gives 0.

Transcendentals.  atan2 / asin (sphere and skybox mappers) and sin / cos (Julia's constant) are mpmath's at 256 bits rounded
ONCE to binary32.  Where the exact value lies within the op's error bound (math_cases.BOUND_ULPS binary64 ULPs) of a
binary32 rounding boundary the element is AMBIGUOUS: the model evaluates it with either neighbour and returns both results
(`alternatives`), and a comparison accepts either.

Two places where the text is undefined and the project has defined a behaviour (both only choose between "material colour"
and a read far outside the atlas, and are stated here as the project states them):
  * `x % 0` in the triangle mapper (TM:224-225 has no guard): whatever the remainder is, `u >= 0 && u < 0` is false, so
    the material's colour results; the model leaves the dividend unchanged.
  * a skybox material WITHOUT a diffuse texture (GI:87-151 fetches whatever the material): the host gives such a material
    the 40000 x 40000 "computed texture" mapping; the sky shows the material's colour.

Before anything is handed to a device `World.check_tables` holds every table to the engine's rule (offset + W * H * depth
+ 2 <= atlas bytes) and every byte index the model computes is asserted to lie inside the atlas (`Model._byte`).

`Model(variant=...)` restates ONE statement wrongly (VARIANTS): the cases must tell each of them from the right model.
"""
import math

import mpmath
import numpy as np

import math_cases as M

F = np.float32
INT_MIN, INT_MAX = -2147483648, 2147483647
TEXTURE_NONE, TEXTURE_MANDELBROT, TEXTURE_JULIA = -1, -2, -3
NB_MAX_ITERATIONS = 10
PI = F(3.14159265358979323846)
(ptSphere, ptCylinder, ptTriangle, ptCheckboard, ptCamera, ptXYPlane, ptYZPlane, ptXZPlane, ptMagicCarpet, ptEnvironment,
 ptEllipsoid, ptQuad, ptCone) = range(13)
SPHERE_LIKE = (ptCone, ptCylinder, ptEnvironment, ptSphere, ptEllipsoid)
CUBE_LIKE = (ptXYPlane, ptYZPlane, ptXZPlane, ptCamera)

VARIANTS = ("cube_v_lt_h", "floor", "py_mod", "nan_int_min", "no_saturation", "f32_pitch", "julia_counts_escape",
            "mandelbrot_new_z", "checker_minus", "secondary_own_size", "bump_scales_opacity", "scroll_always")


def wrap(i):
    """a Python int as the 32-bit two's complement int it would be in C"""
    i &= 0xFFFFFFFF
    return i - (1 << 32) if i & 0x80000000 else i


def crem(a, b):
    """C's truncating remainder: the sign of the dividend"""
    r = abs(a) % abs(b)
    return -r if a < 0 else r


def nearest32(x, ulps):
    """an mpmath value -> (the nearest binary32, the other bracketing binary32 when x lies within `ulps` binary64 ULPs of
    the rounding boundary between them, else None)"""
    if x == 0:
        return F(0.0), None
    f = F(float(x))                                       # (rounded twice: the right one is this or a neighbour)
    around = [np.nextafter(f, F(-np.inf)), f, np.nextafter(f, F(np.inf))]
    best = min(around, key=lambda c: abs(x - mpmath.mpf(float(c))))
    lo, hi = np.nextafter(best, F(-np.inf)), np.nextafter(best, F(np.inf))
    b = mpmath.mpf(float(best))
    d_lo, d_hi = abs(x - (b + mpmath.mpf(float(lo))) / 2), abs(x - (b + mpmath.mpf(float(hi))) / 2)
    reach = ulps * mpmath.mpf(math.ulp(abs(float(x))))
    if min(d_lo, d_hi) <= reach:
        return best, (lo if d_lo < d_hi else hi)
    return best, None


_CACHE = {}


def _transcendental(op, a, b=None):
    """(binary32 result, alternative or None) of atan2(a, b), asin(a), sin(a), cos(a): binary32 in, exact in between"""
    key = (op, F(a).tobytes(), None if b is None else F(b).tobytes())
    if key in _CACHE:
        return _CACHE[key]
    a = F(a)
    ulps = M.BOUND_ULPS[op]
    with mpmath.workprec(256):
        if op == M.ATAN2:
            b = F(b)
            assert not (np.isinf(a) or np.isinf(b)), "non-finite hit points are out of scope"
            if a != a or b != b:
                out = (F(np.nan), None)
            elif a == 0:                                   # C99 F.10.1.4: +-0 for b > 0 or +0, +-pi for b < 0 or -0
                if b > 0 or (b == 0 and not np.signbit(b)):
                    out = (a, None)
                else:
                    r, alt = nearest32(mpmath.pi, ulps)
                    out = (-r, None if alt is None else -alt) if np.signbit(a) else (r, alt)
            else:
                out = nearest32(mpmath.atan2(mpmath.mpf(float(a)), mpmath.mpf(float(b))), ulps)
        elif op == M.ASIN:
            if a != a or abs(a) > 1:
                out = (F(np.nan), None)
            elif a == 0:
                out = (a, None)
            else:
                out = nearest32(mpmath.asin(mpmath.mpf(float(a))), ulps)
        else:
            assert np.isfinite(a)
            if op == M.SIN and a == 0:
                out = (a, None)
            else:
                out = nearest32((mpmath.sin if op == M.SIN else mpmath.cos)(mpmath.mpf(float(a))), ulps)
    _CACHE[key] = out
    return out


class World:
    """a texture atlas and a material table; `materials` is a numpy array of the package's MATERIAL_DTYPE"""

    def __init__(self, materials, textures, own_texels=None):
        self.materials = materials
        self.textures = np.ascontiguousarray(textures, np.uint8)
        # per material, the size in bytes of each of its seven maps' OWN textures (only the secondary_own_size variant reads it)
        self.own_texels = own_texels if own_texels is not None else {}
        self._mat = {}

    def material(self, i):
        if i not in self._mat:
            m = self.materials[i]
            ids = [int(x) for x in m["textureIds"]] + [int(x) for x in m["advancedTextureIds"][:3]]
            off = [int(x) for x in m["textureOffset"]] + [int(x) for x in m["advancedTextureOffset"][:3]]
            self._mat[i] = dict(id=i, color=[F(x) for x in m["color"]], W=int(m["textureMapping"][0]),
                                H=int(m["textureMapping"][1]), depth=int(m["textureMapping"][3]), ids=ids, off=off,
                                mo=[F(x) for x in m["mappingOffset"]], attributes=[int(x) for x in m["attributes"]],
                                inner=F(m["innerIllumination"][0]), specular=[F(x) for x in m["specular"][:3]])
        return self._mat[i]

    def check_tables(self, used):
        """the rule of the engine's checkTextureTables for every material in `used`: a textured material (a diffuse id >= 0
        and a mapping with columns) has rows and a depth, and each map it names lies, AT THE DIFFUSE TEXTURE'S SIZE, inside
        the atlas with the two bytes a depth-1 fetch reads beyond its texel"""
        nbytes = len(self.textures)
        for i in sorted(set(int(x) for x in used)):
            m = self.material(i)
            assert not (m["ids"][0] >= 0 and m["W"] == 40000 and m["H"] == 40000 and m["off"][0] == 0), \
                "material %d carries the computed-texture mapping next to a texture id: the engine makes it untextured" % i
            if m["ids"][0] < 0 or m["W"] <= 0:
                continue
            texels = m["W"] * m["H"] * m["depth"]
            assert m["H"] > 0 and m["depth"] > 0 and texels < 2 ** 31, i
            for t in range(7):
                if t == 0 or m["ids"][t] != TEXTURE_NONE:
                    assert 0 <= m["off"][t] and m["off"][t] + texels + 2 <= nbytes, \
                        "material %d, map %d: offset %d + %d texels + 2 > %d atlas bytes" % (i, t, m["off"][t], texels, nbytes)


class Model:
    def __init__(self, world, variant=None):
        assert variant is None or variant in VARIANTS, variant
        self.world, self.variant = world, variant
        self.tex = world.textures
        self._forced, self._ambiguous, self._ops = (), [], 0
        self.note = {}

    # ---- the conversions ------------------------------------------------------------------------------------------
    def to_int(self, v):
        """float -> int as the device converts: truncate, saturate, NaN -> 0"""
        v = F(v)
        if v != v:
            self._flag("nan")
            return INT_MIN if self.variant == "nan_int_min" else 0
        if v >= F(2147483648.0) or v < F(-2147483648.0):
            self._flag("saturated")
            if self.variant == "no_saturation":          # what an x86 cast or a wrapping conversion would leave
                return INT_MIN if np.isinf(v) else wrap(int(float(v)))
            return INT_MAX if v > 0 else INT_MIN
        if self.variant == "floor":
            return int(math.floor(float(v)))
        return int(float(v))

    def mod(self, a, b):
        if self.variant == "py_mod":
            return a % b
        return crem(a, b)

    def _flag(self, what):
        self.note[what] = self.note.get(what, 0) + 1

    def _fn(self, op, a, b=None):
        k = self._ops
        self._ops += 1
        value, alt = _transcendental(op, a, b)
        if alt is not None:
            self._ambiguous.append(k)
            if k in self._forced:
                return alt
        return value

    def _byte(self, i):
        assert 0 <= i < len(self.tex), "byte index %d outside the atlas of %d bytes" % (i, len(self.tex))
        return int(self.tex[i])

    # ---- TM:30-116 and the fetch every mapper repeats (TM:238-279, 311-343, 410-440) --------------------------------
    def fetch(self, m, u, v, out):
        W, H, depth = m["W"], m["H"], m["depth"]
        A = wrap(wrap(wrap(v * W) + u) * depth)
        B = wrap(wrap(W * H) * depth)
        index = self.mod(A, B)

        def rgb(t):
            idx = index
            if t and self.variant == "secondary_own_size":
                idx = self.mod(A, self.world.own_texels[m["id"]][t])
            i = m["off"][t] + idx
            return self._byte(i), self._byte(i + 1), self._byte(i + 2)
        r, g, b = rgb(0)
        out["index"] = index
        result = [F(r) / F(256.0), F(g) / F(256.0), F(b) / F(256.0)]
        strength = F(3.0)
        ids = m["ids"]
        if ids[2] != TEXTURE_NONE:                                        # bumpMap, TM:45-57
            r, g, b = rgb(2)
            strength = F(10.0) * F(r + g + b) / F(768.0)
            if self.variant == "bump_scales_opacity":
                out["attributes"][3] = out["attributes"][3] * (F(r + g + b) / F(768.0))
        if ids[1] != TEXTURE_NONE:                                        # normalMap, TM:30-40
            r, g, _ = rgb(1)
            n = out["normal"]
            n[0] = n[0] - strength * (F(r) / F(256.0) - F(0.5))
            n[1] = n[1] - strength * (F(g) / F(256.0) - F(0.5))
            n[2] = F(0.0)
        if ids[3] != TEXTURE_NONE:                                        # specularMap, TM:62-73
            r, g, b = rgb(3)
            out["specular"][0] = F(r) / F(256.0)
            out["specular"][1] = F(1000.0) * F(g) / F(256.0)
            out["specular"][2] = F(b) / F(256.0)
        if ids[4] != TEXTURE_NONE:                                        # reflectionMap, TM:78-87
            r, g, b = rgb(4)
            out["attributes"][0] = out["attributes"][0] * (F(r + g + b) / F(768.0))
        if ids[5] != TEXTURE_NONE:                                        # transparencyMap, TM:92-102
            r, g, b = rgb(5)
            out["attributes"][1] = out["attributes"][1] * (F(r + g + b) / F(768.0))
        if ids[6] != TEXTURE_NONE:                                        # ambientOcclusionMap, TM:107-116
            r, g, b = rgb(6)
            out["advanced"][0] = F(r + g + b) / F(768.0)
        return result

    # ---- TM:118-197 ---------------------------------------------------------------------------------------------------
    def _shade(self, color, n, limit, out):
        share = F(n) / limit
        out["steps"] = n
        return [F(1.0) - color[0] * share, F(1.0) - color[1] * share, F(1.0) - color[2] * share, F(1.0) - share]

    def julia(self, m, si, x, y, color, out):
        W, H = F(m["W"]), F(m["H"])
        cRe = F(-0.7) + F(0.4) * self._fn(M.SIN, F(si.timestamp) / F(1500.0))
        cIm = F(0.27015) + F(0.4) * self._fn(M.COS, F(si.timestamp) / F(2000.0))
        newRe = F(1.5) * (x - W / F(2.0)) / (F(0.5) * W)
        newIm = (y - H / F(2.0)) / (F(0.5) * H)
        limit = F(40.0) + F(si.pathTracingIteration)
        n = 0
        while F(n) < limit:
            oldRe, oldIm = newRe, newIm
            newRe = oldRe * oldRe - oldIm * oldIm + cRe
            newIm = F(2.0) * oldRe * oldIm + cIm
            if (newRe * newRe + newIm * newIm) > F(4.0):
                if self.variant == "julia_counts_escape":
                    n += 1
                break
            n += 1
        if newRe != newRe or newIm != newIm:
            self._flag("fractal_nan")
        return self._shade(color, n, limit, out)

    def mandelbrot(self, m, si, x, y, color, out):
        W, H = F(m["W"]), F(m["H"])
        MinRe, MaxRe, MinIm = F(-2.0), F(1.0), F(-1.2)
        MaxIm = MinIm + (MaxRe - MinRe) * H / W
        Re_factor = (MaxRe - MinRe) / (W - F(1.0))
        Im_factor = np.float64((MaxIm - MinIm) / (H - F(1.0)))            # a binary32 quotient, widened
        limit = F(NB_MAX_ITERATIONS + si.pathTracingIteration)
        if self.variant == "f32_pitch":
            c_im = MaxIm - y * F(Im_factor)
        else:
            c_im = F(np.float64(MaxIm) - np.float64(y) * Im_factor)
        c_re = MinRe + x * Re_factor
        Z_re, Z_im = c_re, c_im
        if c_re != c_re or c_im != c_im:
            self._flag("fractal_nan")
        inside, n = True, 0
        while inside and F(n) < limit:
            Z_re2, Z_im2 = Z_re * Z_re, Z_im * Z_im
            if self.variant != "mandelbrot_new_z" and Z_re2 + Z_im2 > F(4.0):
                inside = False
            Z_im = F(2.0) * Z_re * Z_im + c_im
            Z_re = Z_re2 - Z_im2 + c_re
            if self.variant == "mandelbrot_new_z" and Z_re * Z_re + Z_im * Z_im > F(4.0):
                inside = False
            n += 1
        return self._shade(color, n, limit, out)

    def _texel(self, m, si, u, v, result, out, fractals=True):
        out["fetched"] = True
        if fractals and m["ids"][0] == TEXTURE_MANDELBROT:
            out["fractal"] = "mandelbrot"
            return self.mandelbrot(m, si, F(u), F(v), result, out)
        if fractals and m["ids"][0] == TEXTURE_JULIA:
            out["fractal"] = "julia"
            return self.julia(m, si, F(u), F(v), result, out)
        return self.fetch(m, u, v, out) + [result[3]]

    # ---- TM:205-283 ---------------------------------------------------------------------------------------------------
    def triangle_mapping(self, si, p, m, areas, out):
        out["mapper"] = "triangle"
        result = list(m["color"])
        a = [F(x) for x in areas]
        vt0, vt1, vt2 = ([F(x) for x in p[k]] for k in ("vt0", "vt1", "vt2"))
        total = a[0] + a[1] + a[2]
        T = [(vt0[c] * a[0] + vt1[c] * a[1] + vt2[c] * a[2]) / total for c in (0, 1)]
        offset = [F(0.0), F(0.0)]
        if m["attributes"][1] == 1 or self.variant == "scroll_always":
            offset = [m["mo"][0] * F(si.timestamp), m["mo"][1] * F(si.timestamp)]
            if m["attributes"][1] == 1 and (offset[0] != 0 or offset[1] != 0):
                self._flag("scrolled")
        W, H = m["W"], m["H"]
        x, y = T[0] * F(W) + offset[0], T[1] * F(H) + offset[1]
        out["uv_float"] = (x, y)
        u, v = self.to_int(x), self.to_int(y)
        if W != 0:
            u = self.mod(u, W)
        else:
            self._flag("zero_width")                       # (undefined in the text; see the module's docstring)
        if H != 0:
            v = self.mod(v, H)
        out["u"], out["v"] = u, v
        if 0 <= u < W and 0 <= v < H:
            result = self._texel(m, si, u, v, result, out)
        return result

    # ---- TM:291-346 ---------------------------------------------------------------------------------------------------
    def normalize(self, v):
        inv = F(1.0) / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        return [v[0] * inv, v[1] * inv, v[2] * inv]

    def sphere_mapping(self, p, m, intersection, out):
        out["mapper"] = "sphere"
        result = list(m["color"])
        I = self.normalize([intersection[c] - F(p["p0"][c]) for c in range(3)])
        U = ((self._fn(M.ATAN2, I[0], I[2]) / PI) + F(1.0)) * F(0.5)
        V = (self._fn(M.ASIN, I[1]) / PI) + F(0.5)
        W, H = m["W"], m["H"]
        u = self.to_int(F(W) * (U * F(p["vt1"][0])))
        v = self.to_int(F(H) * (V * F(p["vt1"][1])))
        if W != 0:
            u = self.mod(u, W)
        if H != 0:
            v = self.mod(v, H)
        out["u"], out["v"], out["I"] = u, v, I
        if 0 <= u < W and 0 <= v < H:
            result = self._texel(m, None, u, v, result, out, fractals=False)
        return result

    # ---- TM:354-447 (no Kinect) -----------------------------------------------------------------------------------------
    def cube_mapping(self, si, p, m, intersection, out):
        out["mapper"] = "cube"
        result = list(m["color"])
        t = int(p["type"])
        p0, size = [F(x) for x in p["p0"]], [F(x) for x in p["size"]]
        I = intersection
        if t in (ptCheckboard, ptXZPlane, ptXYPlane):
            x = I[0] - p0[0] + size[0]
        else:
            x = I[2] - p0[2] + size[2]
        if t in (ptCheckboard, ptXZPlane):
            y = (I[2] - p0[2] if self.variant == "checker_minus" else I[2] + p0[2]) + size[2]   # plus: TM:390
        else:
            y = I[1] - p0[1] + size[1]
        out["uv_float"] = (x, y)
        u, v = self.to_int(x), self.to_int(y)
        W, H = m["W"], m["H"]
        if W != 0:
            u = self.mod(u, W)
        if H != 0:
            v = self.mod(v, H)
        out["u"], out["v"] = u, v
        limit = H if self.variant == "cube_v_lt_h" else W                 # sic, TM:398
        if 0 <= u < W and 0 <= v < limit:
            result = self._texel(m, si, u, v, result, out)
        elif 0 <= u < W and 0 <= v < H:
            self._flag("blanked_row")                      # a row of a tall texture that TM:398 leaves to the material
        return result

    # ---- GS:36-124 -----------------------------------------------------------------------------------------------------
    def intersection_shader(self, si, p, intersection, areas, attributes):
        """-> dict(color [4], bump [3], specular [3], advanced [1], attributes [4]) and the element's trace"""
        m = self.world.material(int(p["materialId"]))
        out = dict(normal=[F(0.0)] * 3, specular=list(m["specular"]), attributes=[F(x) for x in attributes],
                   advanced=[F(0.0)], mapper="none", fetched=False)
        color = list(m["color"][:3]) + [F(0.0)]
        I = [F(x) for x in intersection]
        t = int(p["type"])
        textured = m["ids"][0] != TEXTURE_NONE
        if si.extendedGeometry:
            if t in SPHERE_LIKE:
                if textured:
                    color = self.sphere_mapping(p, m, I, out)
            elif t == ptCheckboard:
                if textured:
                    color = self.cube_mapping(si, p, m, I, out)
                else:
                    out["mapper"] = "checker"
                    p0, sx = [F(x) for x in p["p0"]], F(p["size"][0])
                    qx, qz = F(si.viewDistance) + ((I[0] - p0[0]) / sx), F(si.viewDistance) + ((I[2] - p0[2]) / sx)
                    x, z = self.to_int(qx), self.to_int(qz)
                    out["u"], out["v"] = x, z
                    if (self.mod(x, 2) == 0) == (self.mod(z, 2) == 0):
                        out["inverted"] = True
                        color = [F(1.0) - color[0], F(1.0) - color[1], F(1.0) - color[2], color[3]]
            elif t in CUBE_LIKE:
                if textured:
                    color = self.cube_mapping(si, p, m, I, out)
            elif t == ptTriangle:
                if textured:
                    color = self.triangle_mapping(si, p, m, areas, out)
        elif textured:
            color = self.triangle_mapping(si, p, m, areas, out)
        res = dict(color=color, bump=out["normal"], specular=out["specular"], advanced=out["advanced"],
                   attributes=out["attributes"])
        return res, out

    # ---- GI:87-151 -------------------------------------------------------------------------------------------------------
    def skybox(self, si, origin, target):
        m = self.world.material(int(si.skyboxMaterialId))
        out = dict(mapper="skybox", fetched=False, where="sky")
        result = list(m["color"][:3])
        o = [F(x) for x in origin]
        d = self.normalize([F(target[c]) - o[c] for c in range(3)])
        dot = lambda p, q: p[0] * q[0] + p[1] * q[1] + p[2] * q[2]      # noqa: E731
        a = F(2.0) * dot(d, d)
        b = F(2.0) * dot(o, d)
        c = dot(o, o) - F(wrap(si.skyboxRadius * si.skyboxRadius))
        disc = b * b - F(2.0) * a * c
        eps = F(si.geometryEpsilon)
        if disc <= 0 or a == 0:
            out["where"] = "no root"
            return dict(color=result), out
        r = np.sqrt(disc)
        t1, t2 = (-b - r) / a, (-b + r) / a
        if t1 <= eps and t2 <= eps:
            out["where"] = "behind"
            return dict(color=result), out
        if t1 <= eps:
            t = t2
        elif t2 <= eps:
            t = t1
        else:
            t = t1 if t1 < t2 else t2
        if t < eps:
            out["where"] = "too close"
            return dict(color=result), out
        if m["ids"][0] < 0:                                 # (the project's rule; see the module's docstring)
            out["where"] = "untextured"
            return dict(color=result), out
        I = self.normalize([o[k] + t * d[k] for k in range(3)])
        U = ((self._fn(M.ATAN2, I[0], I[2]) / PI) + F(1.0)) * F(0.5)
        V = (self._fn(M.ASIN, I[1]) / PI) + F(0.5)
        W, H = m["W"], m["H"]
        u, v = self.to_int(F(W) * U), self.to_int(F(H) * V)
        if W != 0:
            u = self.mod(u, W)
        if H != 0:
            v = self.mod(v, H)
        out["u"], out["v"], out["I"] = u, v, I
        if 0 <= u < W and 0 <= v < H:
            out["fetched"] = True
            A = wrap(wrap(wrap(v * W) + u) * m["depth"])
            index = self.mod(A, wrap(wrap(W * H) * m["depth"]))
            i = m["off"][0] + index
            result = [F(self._byte(i + k)) / F(256.0) for k in range(3)]
        return dict(color=result), out

    # ---- TM:449-456 and GI:430-561 -----------------------------------------------------------------------------------------
    def wire_frame(self, x, y, width):
        X, Y = self.to_int(abs(F(x))), self.to_int(abs(F(y)))
        return self.mod(X, 100) <= width or self.mod(Y, 100) <= width

    def plane(self, si, p, origin, direction, shadows, initial):
        """-> dict(hit, intersection [3], normal [3], shadow) as the per-primitive test leaves them.  The shadow walk's
        dispatch (GI:833-870) differs from the closest-hit walk's for these types only in skipping ptCamera."""
        m = self.world.material(int(p["materialId"]))
        out = dict(mapper="plane", fetched=False)
        I = [F(x) for x in initial[0]]                      # (the caller's locals; the normal is set on entry, GI:431)
        t = int(p["type"])
        assert t in (ptCheckboard, ptMagicCarpet, ptXZPlane, ptYZPlane, ptXYPlane), t
        o, d = [F(x) for x in origin], [F(x) for x in direction]
        p0, size = [F(x) for x in p["p0"]], [F(x) for x in p["size"]]
        collision = False
        N = [F(x) for x in p["n0"]]
        wire, width = m["attributes"][2] == 2, m["attributes"][3]
        # (axis, the two in-plane axes in the order the text names them)
        axis, (c1, c2) = {ptCheckboard: (1, (0, 2)), ptMagicCarpet: (1, (0, 2)), ptXZPlane: (1, (0, 2)),
                          ptYZPlane: (0, (1, 2)), ptXYPlane: (2, (0, 1))}[t]
        dist = o[axis] - p0[axis]

        def place():
            I[axis] = p0[axis]
            I[c1] = o[c1] + dist * d[c1] / -d[axis]
            I[c2] = o[c2] + dist * d[c2] / -d[axis]
            hit = bool(abs(I[c1] - p0[c1]) < size[c1] and abs(I[c2] - p0[c2]) < size[c2])
            if t == ptYZPlane and m["inner"] != 0:         # "chessboard like lights", GI:486-490 (z first, then y)
                lit = self.mod(self.to_int(abs(I[2])), 4000) < 2000 and self.mod(self.to_int(abs(I[1])), 4000) < 2000
                if hit and not lit:
                    out["dark_square"] = True
                hit = hit and lit
            if wire and t not in (ptCheckboard, ptMagicCarpet):
                on_wire = self.wire_frame(I[c1], I[c2], width)
                if hit and not on_wire:
                    out["between_wires"] = True
                hit = hit and on_wire
            return hit
        if t in (ptCheckboard, ptMagicCarpet):
            I[1] = p0[1]
        if d[axis] < 0 and o[axis] > p0[axis]:
            collision = place()
        if t not in (ptCheckboard, ptMagicCarpet) and not collision and d[axis] > 0 and o[axis] < p0[axis]:
            N = [-x for x in N]
            out["back"] = True
            collision = place()
        shadow = F(0.0)
        if collision:
            shadow = F(1.0)
            color = list(m["color"])
            if m["ids"][0] != TEXTURE_NONE:
                acc = dict(normal=N, specular=[F(0.0)] * 3, attributes=[F(0.0)] * 4, advanced=[F(0.0)], fetched=False)
                color = self.cube_mapping(si, p, m, I, acc)
                out.update({k: acc[k] for k in ("u", "v", "fetched", "fractal", "steps") if k in acc})
                shadow = color[3]
            if (color[0] + color[1] + color[2]) / F(3.0) >= F(si.transparentColor):
                out["keyed_out"] = True
                collision = False
        return dict(hit=int(collision), intersection=I, normal=N, shadow=shadow), out

    # ---- an element with its alternatives --------------------------------------------------------------------------------
    def element(self, fn, *args):
        """-> (result, trace, [alternative results]) of one element; the alternatives are the results with an ambiguous
        transcendental rounded the other way (every combination)"""
        self._forced, self._ambiguous, self._ops, self.note = (), [], 0, {}
        with np.errstate(all="ignore"):
            res, trace = fn(*args)
            trace["notes"] = dict(self.note)
            ambiguous = list(self._ambiguous)
            trace["ambiguous"] = len(ambiguous)
            alternatives = []
            for mask in range(1, 1 << len(ambiguous)):
                self._forced = tuple(k for j, k in enumerate(ambiguous) if mask >> j & 1)
                self._ambiguous, self._ops = [], 0
                alternatives.append(fn(*args)[0])
        self._forced = ()
        return res, trace, alternatives


def _stack(rows, keys):
    return {k: np.array([[x for x in np.atleast_1d(r[k])] for r in rows], F if k != "hit" else np.int32) for k in keys}


def run(case, world, variant=None):
    """a case of texture_mapper_cases through the model: (outputs keyed like oracle.probes.oracle_outputs, the traces,
    {element: [alternative outputs, one row each]})"""
    model = Model(world, variant)
    name, si = case["name"], case["si"]
    rows, traces, alts = [], [], {}
    if name == "intersection_shader":
        world.check_tables(case["prims"]["materialId"])
        keys = ("color", "bump", "specular", "advanced", "attributes")
        for e in range(len(case["inter"])):
            r, t, a = model.element(model.intersection_shader, si, case["prims"][e], case["inter"][e], case["areas"][e],
                                    case["attributes"][e])
            rows.append(r), traces.append(t)
            if a:
                alts[e] = a
    elif name == "skybox":
        world.check_tables([si.skyboxMaterialId])
        keys = ("color",)
        for e in range(len(case["origins"])):
            r, t, a = model.element(model.skybox, si, case["origins"][e], case["targets"][e])
            rows.append(r), traces.append(t)
            if a:
                alts[e] = a
    elif name == "primitive":
        world.check_tables(case["prims"]["materialId"])
        keys = ("hit", "intersection", "normal", "shadow")
        for e in range(len(case["origins"])):
            r, t, a = model.element(model.plane, si, case["prims"][e], case["origins"][e], case["directions"][e],
                                    int(case["shadows"][e]), case["initial"][e])
            rows.append(r), traces.append(t)
    else:
        raise KeyError(name)
    out = _stack(rows, keys)
    if name == "primitive":
        out["hit"], out["shadow"] = out["hit"].reshape(-1), out["shadow"].reshape(-1)
    alts = {e: [_stack([a], keys) for a in al] for e, al in alts.items()}
    return out, traces, alts


# ---- exact geometry ----------------------------------------------------------------------------------------------------
def exact_texel(I, W, H, sx=1.0, sy=1.0, centre=None):
    """the texel of the EXACT U, V of a binary32 point (`centre` None: the point is a direction to be normalised exactly;
    else the point minus the centre is), with no rounding in between: (u, v) after the truncating remainder"""
    with mpmath.workprec(256):
        x, y, z = (mpmath.mpf(float(I[c])) - (mpmath.mpf(float(centre[c])) if centre is not None else 0) for c in range(3))
        n = mpmath.sqrt(x * x + y * y + z * z)
        if n == 0:
            return None
        x, y, z = x / n, y / n, z / n
        U = (mpmath.atan2(x, z) / mpmath.pi + 1) / 2
        V = mpmath.asin(y) / mpmath.pi + mpmath.mpf(1) / 2
        u = int(W * (U * mpmath.mpf(float(sx))))            # int() truncates
        v = int(H * (V * mpmath.mpf(float(sy))))
        return (crem(u, W) if W else u), (crem(v, H) if H else v)


def cyclic_distance(a, b, n):
    d = abs(a - b)
    return min(d, n - d) if n else d
