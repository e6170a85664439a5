"""Seeded inputs that steer the texture mappers to their texel edges (test infrastructure; numpy only, no GPU).

Every case is a dict in the shape oracle.probes uses, so that engine_probes.engine_outputs, the oracle's probes and
texture_mapper_model.run take it unchanged: `intersection_shader` cases (si, prims, materials, textures, inter, areas,
attributes - element e is primitive e), `skybox` cases (origins, targets) and `primitive` cases (the planes by rays: origins,
directions, shadows, initial).  All cases but the lean planes share ONE world (`world()`): an atlas of random bytes holding
every texture shape x depth, and a table of materials over it.  A case also carries `kind` (a label per element: what the
element was placed for) and `oracle` (False for the one case the C oracle cannot be given: `x % 0` traps on the host).

The wave mix (`mix_sorted`, `mix_interleaved`) holds every element of the cube, checkerboard, triangle, sphere and fractal
batches under one SceneInfo - everything solr_hip_probe_intersection_shader evaluates; the skybox and the planes by rays go
through probes of their own and cannot share a wave with them.

`edges(name)` counts, on the MODEL's trace of a case, each edge the generator claims to steer; `EXPECT` names the
edges every case must reach (tests/test_texture_mapper_cases.py asserts them, in the style of tree_builder_cases.py).
"""
import contextlib
import importlib

import numpy as np

import texture_mapper_model as T

F, i32 = np.float32, np.int32
SHAPES = ((1, 1), (1, 5), (5, 1), (2, 2), (3, 7), (7, 3), (16, 16), (64, 32))
SMALL = SHAPES[:6]
DEPTHS = (1, 3, 4)
HOST_SHAPE = (40000, 40000)                      # the mapping the host gives a computed texture (GPUKernel.cpp:1893-1896)
NOT_FOR_THE_ORACLE = ("triangle_zero_width",)    # `x % 0` traps on the host: engine against model only
MIX_SI = dict(timestamp=3, pathTracingIteration=1, viewDistance=50000.0)


def _solr():
    return importlib.import_module("sol-r_amd")


def _si(**kw):
    from oracle import probes
    return probes._scene_info(**kw)


def _records(rows, dtype):
    """a list of 0-d records as one array of the package's dtype (np.array would drop the dtype's padding)"""
    out = np.zeros(len(rows), dtype)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def up(x):
    return np.nextafter(F(x), F(np.inf))


def down(x):
    return np.nextafter(F(x), F(-np.inf))


# ---- the world ---------------------------------------------------------------------------------------------------------
_WORLD = None


def world():
    """the shared atlas and materials; `.mat` names the materials, `.tex` the textures (offset, W, H, depth)"""
    global _WORLD
    if _WORLD is not None:
        return _WORLD
    solr = _solr()
    rng = np.random.default_rng(4101)
    atlas, tex = [], {}

    def add_texture(name, W, H, depth, data=None):
        offset = sum(len(a) for a in atlas)
        data = rng.integers(0, 256, W * H * depth).astype(np.uint8) if data is None else np.asarray(data, np.uint8)
        assert len(data) == W * H * depth
        atlas.append(data)
        tex[name] = (offset, W, H, depth)
        return name

    # six small secondary maps FIRST: read at a larger diffuse texture's index they run on into the textures behind them
    for t in range(1, 7):
        add_texture(("small", t), 2, 2, 3)
    # texels whose mean lies just below, at and just above 0.5 (the colour key of the planes), and a dark one
    add_texture("key", 2, 2, 3, [127, 128, 128, 128, 128, 128, 129, 128, 128, 10, 20, 30])
    for shape in SHAPES:
        for depth in DEPTHS:
            add_texture(("diffuse", shape, depth), shape[0], shape[1], depth)
    for shape, depth in (((7, 3), 3), ((3, 7), 3), ((16, 16), 4)):
        for t in range(1, 7):
            add_texture(("map", t, shape), shape[0], shape[1], depth)
    atlas.append(rng.integers(1, 256, 4).astype(np.uint8))     # what a depth-1 fetch of the last texel reads beyond it
    textures = np.concatenate(atlas)

    records, mat, own = [], {}, {}

    def add_material(name, color=(0.8, 0.6, 0.4, 0.35), diffuse=None, maps=None, mapping=None, fractal=None, procedural=0,
                     mapping_offset=(0.0, 0.0), wire=0, width=0, inner=0.0):
        m = np.zeros((), solr.MATERIAL_DTYPE)
        m["color"], m["specular"] = color, (0.3, 77.0, 0.1, 0.0)
        m["reflection"], m["refraction"], m["transparency"], m["opacity"] = 0.31, 1.1, 0.27, 0.43
        m["innerIllumination"][0] = inner
        m["attributes"] = (0, procedural, wire, width)
        m["textureIds"], m["advancedTextureIds"] = T.TEXTURE_NONE, T.TEXTURE_NONE
        m["mappingOffset"] = mapping_offset
        sizes = [0] * 7
        if fractal is not None:
            m["textureIds"][0] = fractal
            m["textureMapping"] = (mapping[0], mapping[1], 0, 3)
        if diffuse is not None:
            off, W, H, depth = tex[diffuse]
            m["textureIds"][0], m["textureOffset"][0] = 7, off          # (an id is only ever compared with TEXTURE_NONE)
            m["textureMapping"] = (W, H, 0, depth) if mapping is None else mapping
            sizes[0] = W * H * depth
            for t, name_t in (maps or {}).items():
                o, w, h, d = tex[name_t]
                if t < 4:
                    m["textureIds"][t], m["textureOffset"][t] = 10 + t, o
                else:
                    m["advancedTextureIds"][t - 4], m["advancedTextureOffset"][t - 4] = 10 + t, o
                sizes[t] = w * h * d
        records.append(m)
        mat[name] = len(records) - 1
        own[len(records) - 1] = sizes
        return mat[name]

    add_material("plain", color=(0.2, 0.3, 0.1, 0.6))
    for shape in SHAPES:
        for depth in DEPTHS:
            add_material(("diffuse", shape, depth), diffuse=("diffuse", shape, depth))
    for shape, depth in (((7, 3), 3), ((3, 7), 3), ((16, 16), 4)):
        d = ("diffuse", shape, depth)
        for t in range(1, 7):
            add_material(("alone", t, shape), diffuse=d, maps={t: ("map", t, shape)})
        add_material(("all", shape), diffuse=d, maps={t: ("map", t, shape) for t in range(1, 7)})
        add_material(("bump_normal", shape), diffuse=d, maps={1: ("map", 1, shape), 2: ("map", 2, shape)})
        add_material(("small", shape), diffuse=d, maps={t: ("small", t) for t in range(1, 7)})
    for shape in SMALL + (HOST_SHAPE,):
        add_material(("mandelbrot", shape), fractal=T.TEXTURE_MANDELBROT, mapping=shape, color=(0.9, 0.8, 0.7, 0.35))
        add_material(("julia", shape), fractal=T.TEXTURE_JULIA, mapping=shape, color=(0.9, 0.8, 0.7, 0.35))
    for j, offset in enumerate(((0.25, -0.5), (-1.5, 2.0), (1.5, 1.0))):
        for procedural in (1, 0, 2):
            add_material(("scroll", j, procedural), diffuse=("diffuse", (64, 32), 3), procedural=procedural,
                         mapping_offset=offset)
    # a mapping without columns over a real texture: what realignTexturesAndMaterials leaves a material whose texture nobody loaded
    add_material("zero_width", diffuse=("diffuse", (1, 5), 3), mapping=(0, 5, 0, 3))
    add_material("key", diffuse="key", color=(0.2, 0.3, 0.1, 0.6))
    _WORLD = T.World(_records(records, solr.MATERIAL_DTYPE), textures, own)
    _WORLD.mat, _WORLD.tex = mat, tex
    return _WORLD


def lean_world():
    """untextured materials only (what the renderer's lean sphere + plane instantiation is launched for): wireframes of three
    widths and an emissive material"""
    solr = _solr()
    records, mat = [], {}
    for name, wire, width, inner in (("plain", 0, 0, 0.0), (("wire", 0), 2, 0, 0.0), (("wire", 3), 2, 3, 0.0),
                                     (("wire", 30), 2, 30, 0.0), ("emissive", 0, 0, 0.5)):
        m = np.zeros((), solr.MATERIAL_DTYPE)
        m["color"], m["specular"] = (0.2, 0.3, 0.1, 0.6), (0.3, 77.0, 0.1, 0.0)
        m["innerIllumination"][0] = inner
        m["attributes"] = (0, 0, wire, width)
        m["textureIds"], m["advancedTextureIds"] = T.TEXTURE_NONE, T.TEXTURE_NONE
        m["textureMapping"] = (40000, 40000, 0, 3)
        records.append(m)
        mat[name] = len(records) - 1
    w = T.World(_records(records, solr.MATERIAL_DTYPE), np.zeros(16, np.uint8))
    w.mat, w.tex = mat, {}
    return w


# ---- batches of elements ---------------------------------------------------------------------------------------------
class Batch:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.prims, self.rows, self.kind = [], [], []

    def add(self, kind, ptype, material, inter=(0, 0, 0), areas=(0, 0, 0), p0=(0, 0, 0), size=(0, 0, 0), vt0=(0, 0),
            vt1=(1, 0), vt2=(0, 1), n0=(0, 0, 1), **rays):
        p = np.zeros((), _solr().PRIMITIVE_DTYPE)
        p["type"], p["materialId"], p["index"] = ptype, material, len(self.prims)
        p["p0"], p["size"], p["n0"], p["vt0"], p["vt1"], p["vt2"] = p0, size, n0, vt0, vt1, vt2
        p["p1"], p["p2"] = (1, 0, 0), (0, 1, 0)
        self.prims.append(p)
        self.rows.append(dict(inter=np.array(inter, F), areas=np.array(areas, F), **rays))
        self.kind.append(kind)

    def extend(self, other):
        self.prims += other.prims
        self.rows += other.rows
        self.kind += other.kind

    def shader_case(self, w, si, order=None, oracle=True):
        n = len(self.prims)
        order = np.arange(n) if order is None else order
        prims = _records(self.prims, _solr().PRIMITIVE_DTYPE)[order]
        prims["index"] = np.arange(n)
        attributes = np.random.default_rng(977).uniform(0.2, 0.9, (n, 4)).astype(F)[order]      # neither 0 nor 1
        return dict(name="intersection_shader", si=si, prims=prims, materials=w.materials, textures=w.textures,
                    inter=np.array([r["inter"] for r in self.rows], F)[order],
                    areas=np.array([r["areas"] for r in self.rows], F)[order], attributes=attributes,
                    kind=[self.kind[i] for i in order], oracle=oracle, world=w)

    def ray_case(self, w, si):
        n = len(self.prims)
        return dict(name="primitive", si=si, prims=_records(self.prims, _solr().PRIMITIVE_DTYPE), materials=w.materials, textures=w.textures,
                    origins=np.array([r["origin"] for r in self.rows], F),
                    directions=np.array([r["direction"] for r in self.rows], F),
                    shadows=np.array([r["shadows"] for r in self.rows], i32), initial=np.zeros((n, 2, 3), F),
                    kind=list(self.kind), oracle=True, world=w)


def _cube_point(ptype, x, y):
    """(intersection, p0) that hand the cube mapper exactly x on its u axis and y on its v axis (TM:385-391)"""
    if ptype in (T.ptXYPlane, T.ptCamera):
        return (x, y, 0), (0, 0, 0)
    if ptype == T.ptYZPlane:
        return (0, y, x), (0, 0, 0)
    return (x, 0, F(y) - F(2.0)), (0, 0, 2.0)               # XZ plane, checkerboard: z + p0.z, never equal to z - p0.z


CUBE_TYPES = (T.ptXYPlane, T.ptYZPlane, T.ptXZPlane, T.ptCheckboard, T.ptCamera)


def cube_batch():
    w, b = world(), Batch(4201)
    for shape in SMALL:                                     # every texel centre
        for depth in DEPTHS:
            for ptype in (CUBE_TYPES if depth == 3 else (T.ptXYPlane,)):
                for v in range(shape[1]):
                    for u in range(shape[0]):
                        inter, p0 = _cube_point(ptype, u + 0.5, v + 0.5)
                        b.add("cube centre", ptype, w.mat["diffuse", shape, depth], inter, p0=p0)
    for shape in ((3, 7), (7, 3), (16, 16), (64, 32)):      # k W and k H exactly and one binary32 step either side
        for depth in ((3,) if shape[0] < 16 else (4,)):
            m = w.mat["diffuse", shape, depth]
            for k in (-2, -1, 0, 1, 2):
                for ptype in (T.ptXYPlane, T.ptYZPlane, T.ptCheckboard):
                    for x in (down(k * shape[0]), F(k * shape[0]), up(k * shape[0])):
                        inter, p0 = _cube_point(ptype, x, 0.5)
                        b.add("cube boundary u", ptype, m, inter, p0=p0)
                for ptype in (T.ptXYPlane, T.ptYZPlane):
                    for y in (down(k * shape[1]), F(k * shape[1]), up(k * shape[1])):
                        inter, p0 = _cube_point(ptype, 0.5, y)
                        b.add("cube boundary v", ptype, m, inter, p0=p0)
            for x, y in b.rng.uniform(-3, 0, (10, 2)) * shape:
                inter, p0 = _cube_point(T.ptXYPlane, F(x), F(y))
                b.add("cube negative", T.ptXYPlane, m, inter, p0=p0)
    edge = F(2147483648.0)
    for shape in ((3, 7), (64, 32)):                        # beyond the int range: the conversion saturates
        for big in (edge, down(edge), up(edge), -edge, down(-edge), up(-edge), F(3e9), F(-3e9)):
            for ptype in (T.ptXYPlane, T.ptYZPlane):
                for x, y in ((big, 0.5), (0.5, big)):
                    inter, p0 = _cube_point(ptype, x, y)
                    b.add("cube beyond int", ptype, w.mat["diffuse", shape, 3], inter, p0=p0)
    for j, (x, y, z) in enumerate(b.rng.uniform(-20, 20, (40, 3)).astype(F)):     # x - p0.x + size.x rounds, twice
        b.add("cube rounding", CUBE_TYPES[j % 5], w.mat["diffuse", ((7, 3), (16, 16))[j % 2], 3], (x, y, z),
              p0=(0.1, -0.3, 0.7), size=(1 / 3, 2 / 3, 0.37))
    for shape in ((7, 3), (3, 7), (16, 16)):                # each map alone, all seven, bump into normal, smaller secondaries
        names = [("alone", t, shape) for t in range(1, 7)] + [("all", shape), ("bump_normal", shape), ("small", shape)]
        for name in names:
            for v in range(shape[1]):
                for u in range(shape[0]):
                    if shape == (16, 16) and (u * 5 + v * 3) % 8:
                        continue
                    inter, p0 = _cube_point(T.ptXYPlane, u + 0.5, v + 0.5)
                    b.add("cube maps", T.ptXYPlane, w.mat[name], inter, p0=p0)
    return b


def checker_batch():
    """the untextured checkerboard (GS:69-88): cells on both sides of zero, a tiny cell (the quotient saturates) and a cell
    of size 0 (the quotient is +-inf, or NaN at the centre)"""
    w, b = world(), Batch(4202)
    m = w.mat["plain"]
    for x in np.arange(-3.5, 4.0, 1.0):
        for z in np.arange(-3.5, 4.0, 1.0):
            b.add("checker cell", T.ptCheckboard, m, (10 + 100 * x, 5, -20 + 100 * z), p0=(10, 5, -20), size=(100, 0, 70))
    for x, z in ((1, 1), (-1, 1), (1, -1), (-1, -1), (0, 1), (1, 0), (0, 0), (-1, 0)):
        b.add("checker tiny cell", T.ptCheckboard, m, (x, 0, z), size=(1e-30, 0, 1))
        b.add("checker cell of size 0", T.ptCheckboard, m, (x, 0, z), size=(0, 0, 1))
    return b


def _centre_areas(shape, u, v):
    W, H = shape
    total = 2 * W * H
    ay, az = (2 * u + 1) * H, (2 * v + 1) * W
    return (total - ay - az, ay, az)


def triangle_batch(ptypes=(T.ptTriangle,)):
    w, b = world(), Batch(4203)
    for ptype in ptypes:
        for shape, depth in [(s, 3) for s in SMALL] + [((1, 1), 1), ((2, 2), 4), ((1, 5), 1)]:
            for v in range(shape[1]):
                for u in range(shape[0]):
                    b.add("triangle centre", ptype, w.mat["diffuse", shape, depth], areas=_centre_areas(shape, u, v))
    if ptypes != (T.ptTriangle,):
        b.add("triangle untextured", ptypes[0], w.mat["plain"], areas=(1, 2, 3))
        return b
    for shape, depth in (((16, 16), 4), ((64, 32), 3), ((2, 2), 3)):        # T x W an integer exactly, and either side
        W, H = shape
        m = w.mat["diffuse", shape, depth]
        for k in (-1, 0, 1, W - 1, W, 2 * W):
            a = F(k * 1024.0 / W)
            for ay in (down(a), a, up(a)):
                az = F(512.0 / H)
                b.add("triangle boundary u", T.ptTriangle, m, areas=(F(1024.0 - float(ay) - float(az)), ay, az))
        for k in (-1, 0, 1, H - 1, H, 2 * H):
            a = F(k * 1024.0 / H)
            for az in (down(a), a, up(a)):
                ay = F(512.0 / W)
                b.add("triangle boundary v", T.ptTriangle, m, areas=(F(1024.0 - float(ay) - float(az)), ay, az))
    for shape, depth in (((3, 7), 3), ((16, 16), 4)):                       # a grazing triangle: the areas sum to 0
        m = w.mat["diffuse", shape, depth]
        b.add("triangle areas all zero", T.ptTriangle, m, areas=(0, 0, 0))
        for a in (1.0, 1e30):
            for areas in ((a, -a, 0), (-a, a, 0), (0, a, -a), (0, -a, a), (a, 0, -a)):
                b.add("triangle areas cancel", T.ptTriangle, m, areas=areas)
    for j in range(40):                                                     # vt outside [0, 1] and negative
        vt = b.rng.uniform(-2, 3, (3, 2)).astype(F)
        areas = (b.rng.dirichlet([1, 1, 1]) * b.rng.uniform(10, 1e6)).astype(F)
        b.add("triangle vt outside", T.ptTriangle, w.mat[("all", (7, 3)) if j % 2 else ("diffuse", (64, 32), 3)], areas=areas,
              vt0=vt[0], vt1=vt[1], vt2=vt[2])
    for name in [("alone", t, (3, 7)) for t in range(1, 7)] + [("all", (3, 7)), ("bump_normal", (3, 7)), ("small", (3, 7)),
                                                              ("small", (7, 3))]:
        shape = name[-1]
        for v in range(shape[1]):
            for u in range(shape[0]):
                b.add("triangle maps", T.ptTriangle, w.mat[name], areas=_centre_areas(shape, u, v))
    b.extend(scroll_batch())
    return b


def scroll_batch():
    """procedural == 1: the mapping scrolls by mappingOffset x timestamp; the same materials with procedural 0 and 2 do not"""
    w, b = world(), Batch(4204)
    for j in range(3):
        for procedural in (1, 0, 2):
            for u, v in ((0, 0), (63, 31), (31, 16), (1, 30), (62, 1), (17, 5)):
                b.add("triangle scroll" if procedural == 1 else "triangle no scroll", T.ptTriangle,
                      w.mat["scroll", j, procedural], areas=_centre_areas((64, 32), u, v))
    return b


def zero_width_batch():
    w, b = world(), Batch(4205)
    for areas in ((1, 1, 2), (0, 0, 0), (1, -1, 0), (3, 5, 8), (-1, 2, 0.5), (0, 1, 0), (0, 0, 1), (1e30, 1, 1)):
        b.add("triangle zero width", T.ptTriangle, w.mat["zero_width"], areas=areas)
    return b


SPHERE_CENTRE = (10.0, -20.0, 30.0)
VT1 = ((1, 1), (2, 0.5), (0, 0), (-1, 1))


def sphere_points(rng):
    """(label, point) around SPHERE_CENTRE: both poles at several radii, the seam I.x == 0, I.z < 0 and one step either side,
    I.z == 0, and random directions"""
    cx, cy, cz = (F(c) for c in SPHERE_CENTRE)
    pts = []
    for r in (1.0, 3.0, 7.3, 1500.0, 0.1):
        pts.append(("sphere pole", (cx, F(cy + F(r)), cz)))
        pts.append(("sphere pole", (cx, F(cy - F(r)), cz)))
    for y in (0.0, 2.5, -4.0):
        for x in (down(cx), cx, up(cx)):
            pts.append(("sphere seam", (x, F(cy + F(y)), F(cz - F(5.0)))))
    for x in (5.0, -5.0):
        for y in (0.0, 1.5):
            pts.append(("sphere z == 0", (F(cx + F(x)), F(cy + F(y)), cz)))
    d = rng.normal(size=(40, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for row in d:
        pts.append(("sphere random", tuple((np.array(SPHERE_CENTRE) + 50.0 * row).astype(F))))
    return pts


def sphere_batch():
    w, b = world(), Batch(4206)
    pts = sphere_points(b.rng)
    for name in (("diffuse", (3, 7), 3), ("diffuse", (7, 3), 3), ("diffuse", (64, 32), 4), ("all", (16, 16))):
        for vt1 in VT1:
            for label, p in pts:
                b.add(label, T.ptSphere, w.mat[name], p, p0=SPHERE_CENTRE, size=(50, 0, 0), vt1=vt1)
    for name in (("diffuse", (1, 1), 1), ("diffuse", (1, 5), 3), ("diffuse", (5, 1), 3), ("diffuse", (2, 2), 1),
                 ("small", (7, 3))):
        for label, p in pts:
            b.add(label, T.ptSphere, w.mat[name], p, p0=SPHERE_CENTRE, size=(50, 0, 0), vt1=(1, 1))
    for ptype in (T.ptCylinder, T.ptCone, T.ptEllipsoid, T.ptEnvironment):      # the same points on the other records
        for label, p in pts:
            b.add(label + " (other record)", ptype, w.mat["all", (16, 16)], p, p0=SPHERE_CENTRE, size=(50, 20, 30),
                  vt1=(1, 1))
    b.add("sphere untextured", T.ptSphere, w.mat["plain"], pts[-1][1], p0=SPHERE_CENTRE, size=(50, 0, 0), vt1=(1, 1))
    return b


# texels of the host's 40000 x 40000 on which, at 10 + 7 steps, the Mandelbrot set's step count with the imaginary pitch kept
# in binary64 (TM:172-175) differs from the count with a binary32 pitch: found by a search over 24 million random texels (one
# in two million qualifies), so that a kernel with a binary32 pitch cannot hide
PITCH_TEXELS = ((9452, 29515), (24004, 38600), (9508, 18323), (9720, 19226), (19969, 38724), (7681, 22296), (9082, 21598),
                (31796, 16531), (10367, 27227), (23255, 35510), (6815, 23856), (32934, 28752))


def fractal_batch():
    """both fractals through the cube mapper (an XY plane) and the triangle mapper: every texel of the small shapes, the
    corners and the centre of the host's 40000 x 40000"""
    w, b = world(), Batch(4207)
    for which in ("mandelbrot", "julia"):
        for shape in SMALL + (HOST_SHAPE,):
            W, H = shape
            texels = [(u, v) for v in range(H) for u in range(W)] if shape != HOST_SHAPE else \
                [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2)] + \
                (list(PITCH_TEXELS) if which == "mandelbrot" else [])
            for u, v in texels:
                inter, p0 = _cube_point(T.ptXYPlane, u + 0.5, v + 0.5)
                b.add("fractal by cube", T.ptXYPlane, w.mat[which, shape], inter, p0=p0)
                b.add("fractal by triangle", T.ptTriangle, w.mat[which, shape], areas=_centre_areas(shape, u, v))
    return b


FRACTAL_FRAMES = ((0, 0), (3, 1), (123456, 7))              # (timestamp, pathTracingIteration)


# ---- skybox -------------------------------------------------------------------------------------------------------------
SKY_RADIUS = 10000                                            # r * r = 1e8 fits an int


def skybox_case(material_name, seed=4301):
    w = world()
    rng = np.random.default_rng(seed)
    R = float(SKY_RADIUS)
    origins, targets, kind = [], [], []

    def put(label, o, t):
        origins.append(o), targets.append(t), kind.append(label)
    for s in (1.0, -1.0):                                     # through the poles, from the centre and from off it
        put("sky pole", (0, 0, 0), (0, s, 0))
        put("sky pole", (0, s * 100.0, 0), (0, s * 200.0, 0))
        put("sky pole", (0, -s * 3000.0, 0), (0, s * 1.0, 0))
    for y in (0.0, 0.3, -0.8):                                # along the seam I.x == 0, I.z < 0 and a hair either side
        for x in (-1e-6, 0.0, 1e-6, -1e-3, 1e-3):
            put("sky seam", (0, 0, 0), (x, y, -1.0))
        put("sky z == 0", (0, 0, 0), (1.0, y, 0.0))
        put("sky z == 0", (0, 0, 0), (-1.0, y, 0.0))
    d = rng.normal(size=(120, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for j, row in enumerate(d):
        if j % 3 == 0:                                        # inside
            o = rng.uniform(-0.5, 0.5, 3) * R
            put("sky from inside", o, o + row * rng.uniform(10, 20000))
        elif j % 3 == 1:                                      # on the sphere: one root at the origin
            o = (row * R).astype(F)
            aim = rng.normal(size=3)
            put("sky from the sphere", o, o + aim * 100.0)
        else:                                                 # outside: towards the sphere, past it, and away from it
            o = row * R * rng.uniform(1.5, 4.0)
            t = (-o, rng.normal(size=3) * R * 0.5, 2.0 * o)[(j // 3) % 3]
            put("sky from outside", o, t)
    si = _si(skyboxRadius=SKY_RADIUS, skyboxMaterialId=w.mat[material_name])
    return dict(name="skybox", si=si, materials=w.materials, textures=w.textures, origins=np.array(origins, F),
                targets=np.array(targets, F), kind=kind, oracle=True, world=w)


SKY_MATERIALS = (("diffuse", (64, 32), 3), ("diffuse", (3, 7), 3), ("diffuse", (7, 3), 4), "plain")


# ---- planes by rays ---------------------------------------------------------------------------------------------------------
PLANES = {T.ptXYPlane: (2, (0, 1)), T.ptYZPlane: (0, (1, 2)), T.ptXZPlane: (1, (0, 2)), T.ptCheckboard: (1, (0, 2))}


def _ray(b, kind, ptype, material, c1, c2, j, level=7.0, size=4.0e9, p0=None):
    """an axis-parallel ray at in-plane coordinates (c1, c2): the hit point's in-plane coordinates are the origin's, exactly.
    j picks the side of the plane and the shadow flag, so that a batch holds both of each"""
    axis, (a1, a2) = PLANES[ptype]
    p0 = [0.0, 0.0, 0.0] if p0 is None else list(p0)
    p0[axis] = level
    side = 1.0 if j % 2 == 0 else -1.0
    origin, direction = [0.0] * 3, [0.0] * 3
    origin[a1], origin[a2], origin[axis] = c1, c2, level + side * 10.0
    direction[axis] = -side * 3.0
    n0 = [0.0] * 3
    n0[axis] = 1.0
    sz = [size] * 3
    sz[axis] = 0.0
    b.add(kind, ptype, material, p0=p0, size=sz, n0=n0, origin=origin, direction=direction, shadows=(j // 2) % 2)


def lean_planes_case():
    """wireframes and the emissive YZ pattern over untextured materials"""
    w, b = lean_world(), Batch(4401)
    j = 0
    for ptype in (T.ptXYPlane, T.ptYZPlane, T.ptXZPlane):
        for width in (0, 3, 30):
            for r in (width, width + 1, 0, 99):
                for base in (0.0, 300.0, -200.0):
                    c = base + r if base >= 0 else base - r           # |c| % 100 == r
                    for pair in ((c, 50.0), (50.0, c), (c + 0.5, -50.0)):
                        _ray(b, "wire", ptype, w.mat["wire", width], pair[0], pair[1], j)
                        j += 1
            for c in (3.0e9, -3.0e9, 2147483648.0, -2147483904.0):     # beyond the int range: |c| saturates, 47 on the grid
                _ray(b, "wire beyond int", ptype, w.mat["wire", width], c, 50.0, j)
                _ray(b, "wire beyond int", ptype, w.mat["wire", width], 50.0, c, j + 1)
                j += 2
    for y in (1999.0, 2000.0, 3999.0, 4000.0, 1999.5, -1999.0, -2000.0, -3999.5, -4000.0):
        for z in (1999.0, 2000.0, 3999.0, 4000.0, -2000.0, 10.0):
            _ray(b, "emissive pattern", T.ptYZPlane, w.mat["emissive"], y, z, j)
            j += 1
    for ptype in PLANES:
        for k in range(4):
            _ray(b, "plain plane", ptype, w.mat["plain"], 3.0, -4.0, k)
    return b.ray_case(w, _si(transparentColor=0.5))


def textured_planes_case():
    """A: the colour key on texels just below, at and just above transparentColor; B: fractal planes (the shadow intensity is
    the shade's w); C: planes with a normal map (and a bump map feeding it)"""
    w, b = world(), Batch(4402)
    j = 0
    for ptype in PLANES:
        for u, v in ((0, 0), (1, 0), (0, 1), (1, 1)):
            for k in range(4):
                c2 = v + 0.5 - (2.0 if ptype in (T.ptXZPlane, T.ptCheckboard) else 0.0)
                _ray(b, "plane colour key", ptype, w.mat["key"], u + 0.5, c2, k, size=1000.0,
                     p0=(0, 0, 2.0) if ptype in (T.ptXZPlane, T.ptCheckboard) else None)
    for which, shape in (("mandelbrot", (7, 3)), ("julia", (3, 7)), ("mandelbrot", (2, 2)), ("julia", (5, 1)),
                         ("mandelbrot", (1, 1))):
        for v in range(shape[1]):
            for u in range(shape[0]):
                _ray(b, "plane fractal", T.ptXYPlane, w.mat[which, shape], u + 0.5, v + 0.5, j, size=1000.0)
                j += 1
    for ptype in PLANES:
        for name in (("all", (7, 3)), ("bump_normal", (7, 3)), ("alone", 1, (7, 3)), ("small", (7, 3))):
            for u, v in ((0, 0), (6, 2), (3, 1), (5, 0)):
                c2 = v + 0.5 - (2.0 if ptype in (T.ptXZPlane, T.ptCheckboard) else 0.0)
                _ray(b, "plane normal map", ptype, w.mat[name], u + 0.5, c2, j, size=1000.0,
                     p0=(0, 0, 2.0) if ptype in (T.ptXZPlane, T.ptCheckboard) else None)
                j += 1
    return b.ray_case(w, _si(transparentColor=0.5, timestamp=3, pathTracingIteration=1))


# ---- the cases ------------------------------------------------------------------------------------------------------------
def mix_batch():
    b = cube_batch()
    for other in (checker_batch(), triangle_batch(), sphere_batch(), fractal_batch()):
        b.extend(other)
    return b


def mix_order(kinds):
    """a permutation that deals the elements out mapper by mapper, so that every wave of 64 holds every mapper, fractal lanes,
    untextured lanes and lanes that miss the texture"""
    groups = {}
    for i, k in enumerate(kinds):
        groups.setdefault(k.split()[0], []).append(i)
    rng = np.random.default_rng(4501)                         # (shuffled within a mapper: its misses come in runs)
    lists = [rng.permutation(np.array(v)) for _, v in sorted(groups.items())]
    n = len(kinds)
    # element i of a group of size g sits at the fraction (i + 0.5) / g of the way through: a stable sort of those fractions
    keys = np.concatenate([(np.arange(len(v)) + 0.5) / len(v) for v in lists])
    order = np.concatenate(lists)[np.argsort(keys, kind="stable")]
    assert sorted(order.tolist()) == list(range(n))
    return order


def _cases():
    w = world()
    flat_types = (T.ptSphere, T.ptXYPlane, T.ptCylinder)
    out = {
        "cube": lambda: cube_batch().shader_case(w, _si(**MIX_SI)),
        "checker_far": lambda: checker_batch().shader_case(w, _si(**MIX_SI)),
        "checker_near": lambda: checker_batch().shader_case(w, _si(timestamp=3, viewDistance=0.0)),
        "triangle": lambda: triangle_batch().shader_case(w, _si(**MIX_SI)),
        "triangle_flat": lambda: triangle_batch(flat_types).shader_case(w, _si(extendedGeometry=0, **MIX_SI)),
        "triangle_zero_width": lambda: zero_width_batch().shader_case(w, _si(**MIX_SI), oracle=False),
        "sphere": lambda: sphere_batch().shader_case(w, _si(**MIX_SI)),
        "planes_lean": lean_planes_case,
        "planes_textured": textured_planes_case,
        "mix_sorted": lambda: mix_batch().shader_case(w, _si(**MIX_SI)),
        "mix_interleaved": lambda: (lambda b: b.shader_case(w, _si(**MIX_SI), order=mix_order(b.kind)))(mix_batch()),
    }
    for ts in (0, 123456, 2 ** 31 - 1):                       # (timestamp 3 is in "triangle")
        out["scroll_t%d" % ts] = lambda ts=ts: scroll_batch().shader_case(w, _si(timestamp=ts))
    for ts, it in FRACTAL_FRAMES:
        out["fractal_t%d_i%d" % (ts, it)] = lambda ts=ts, it=it: fractal_batch().shader_case(
            w, _si(timestamp=ts, pathTracingIteration=it, viewDistance=50000.0))
    for j, name in enumerate(SKY_MATERIALS):
        out["skybox_%d" % j] = lambda name=name, j=j: skybox_case(name, seed=4301 + j)
    return out


_BUILT = {}                                      # (cases are built on first use: the package is imported then)


def names():
    return sorted(_cases())


def case(name):
    if name not in _BUILT:
        _BUILT[name] = _cases()[name]()
    return _BUILT[name]


_MODEL = {}


def model_outputs(name):
    """(outputs, traces, alternatives) of the right model for a case; computed once and shared"""
    if name not in _MODEL:
        c = case(name)
        _MODEL[name] = T.run(c, c["world"])
    return _MODEL[name]


# ---- comparing ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def rounded_oracle(loader):
    """the C oracle in its CUDA dialect with binary64 transcendentals rounded once; the setting it had is put back"""
    L = loader.lib()
    was = L.oracle_get_rounded_transcendentals()
    assert L.oracle_get_dialect() == 0
    L.oracle_set_rounded_transcendentals(1)
    try:
        yield L
    finally:
        L.oracle_set_rounded_transcendentals(1 if was else 0)


def oracle_outputs(L, case):
    from oracle import probes
    assert L.oracle_get_dialect() == 0 and L.oracle_get_rounded_transcendentals()
    return probes._oracle_outputs(L, case)


def rows_equal(a, b):
    """per element: equal as numbers, NaN equal to NaN"""
    from oracle import probes
    same = probes.same_bits(np.asarray(a), np.asarray(b))
    return same.reshape(len(same), -1).all(axis=1)


def differing(case, model, alternatives, other):
    """the elements on which `other` equals neither the model's result nor one of an ambiguous element's alternatives.  What a
    plane test leaves in its outputs on a miss is the caller's locals: hit is compared everywhere, the rest where both hit."""
    n = len(model[next(iter(model))])
    bad = np.zeros(n, bool)
    for key in model:
        if key == "features":
            continue
        same = rows_equal(model[key], other[key])
        if case["name"] == "primitive" and key != "hit":
            same |= (model["hit"] == 0) & (other["hit"] == 0)
        bad |= ~same
    for e in np.flatnonzero(bad):
        for alt in alternatives.get(int(e), ()):
            if all(rows_equal(alt[key], other[key][e:e + 1]).all() for key in alt):
                bad[e] = False
    return np.flatnonzero(bad)


# ---- which edges a case reaches (counted on the model's trace) -----------------------------------------------------------
def edges(name):
    c = case(name)
    out, traces, alts = model_outputs(name)
    kinds = c["kind"]
    count = {}

    def bump(key, by=1):
        count[key] = count.get(key, 0) + by
    for e, (t, kind) in enumerate(zip(traces, kinds)):
        bump("elements")
        bump("kind: " + kind)
        bump("mapper: " + t["mapper"])
        for k, v in t["notes"].items():
            bump(("elements with " + k) if k in ("nan", "saturated") else k)
        if t.get("fetched"):
            bump("fetched")
        elif t["mapper"] in ("cube", "triangle", "sphere"):
            bump("missed the texture")
            if t["u"] < 0 or t["v"] < 0:
                bump("missed: negative remainder")
        if t.get("fractal"):
            bump("fractal: " + t["fractal"])
        if "uv_float" in t:
            x, y = t["uv_float"]
            for axis, value, size in (("u", x, c["world"].material(int(c["prims"]["materialId"][e]))["W"]),
                                      ("v", y, c["world"].material(int(c["prims"]["materialId"][e]))["H"])):
                if np.isfinite(value) and size and float(value) == int(float(value)) and int(float(value)) % size == 0 \
                        and "boundary " + axis in kind:
                    bump("exactly on k x size (%s)" % axis)
        for k in ("inverted", "dark_square", "between_wires", "keyed_out", "back"):
            if t.get(k):
                bump(k)
        if t["mapper"] == "skybox":
            bump("sky: " + t["where"])
        if t["ambiguous"]:
            bump("ambiguous")
    if c["name"] == "primitive":
        count["hits"] = int(out["hit"].sum())
    return count


# what every case must reach at least once (per edge, on the model)
EXPECT = {
    "cube": ("kind: cube centre", "kind: cube boundary u", "kind: cube boundary v", "kind: cube negative",
             "kind: cube beyond int", "kind: cube rounding", "kind: cube maps", "blanked_row", "elements with saturated",
             "missed: negative remainder", "exactly on k x size (u)", "exactly on k x size (v)", "fetched"),
    "checker_far": ("inverted", "elements with saturated", "elements with nan", "mapper: checker"),
    "checker_near": ("inverted", "elements with saturated", "elements with nan", "mapper: checker"),
    "triangle": ("kind: triangle centre", "exactly on k x size (u)", "exactly on k x size (v)", "elements with nan",
                 "elements with saturated", "missed: negative remainder", "scrolled", "kind: triangle no scroll",
                 "kind: triangle vt outside", "kind: triangle maps", "fetched"),
    "triangle_flat": ("mapper: triangle", "mapper: none", "fetched"),
    "triangle_zero_width": ("zero_width", "missed the texture"),
    "sphere": ("kind: sphere pole", "kind: sphere seam", "kind: sphere z == 0", "kind: sphere random", "fetched",
               "missed: negative remainder", "mapper: none"),
    "planes_lean": ("between_wires", "dark_square", "back", "elements with saturated", "hits"),
    "planes_textured": ("keyed_out", "back", "fractal: mandelbrot", "fractal: julia", "fetched", "hits"),
    "mix_sorted": ("mapper: cube", "mapper: triangle", "mapper: sphere", "mapper: checker", "fractal: julia",
                   "fractal: mandelbrot", "missed the texture"),
    "scroll_t0": ("kind: triangle scroll", "fetched"),
    "scroll_t123456": ("scrolled", "fetched"),
    "scroll_t2147483647": ("scrolled", "elements with saturated", "fetched"),
    "skybox_0": ("sky: sky", "sky: behind", "sky: no root", "fetched", "kind: sky pole", "kind: sky seam"),
    "skybox_3": ("sky: untextured",),
}
for _ts, _it in FRACTAL_FRAMES:
    EXPECT["fractal_t%d_i%d" % (_ts, _it)] = ("fractal: julia", "fractal: mandelbrot", "fractal_nan", "blanked_row",
                                              "kind: fractal by cube", "kind: fractal by triangle")
