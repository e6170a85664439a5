"""Hits and shadow rays aimed at the decisions of primitiveShader and of the shadow sum (test infrastructure: a generator,
deterministic, no GPU).

GI:916-1080 (primitiveShader) is made of equalities and strict comparisons - the range of a lamp, the sign of the Lambert term,
innerIllumination.x == 0, the bounce number, three graphics-level gates, the lamp's own primitive, the gate and the two guards
of the Blinn term, the noise, the lamp choice and jitter of the accumulation passes, the wireframe return, the saturation inside
a lamp loop that shades lamp 0 nbLights times - and GI:866-908 (the sum inside processShadows) re-tests `result < shadowIntensity`
before every node and every primitive.  The cases built here put elements ON those comparisons, in the layouts
oracle.probes.case_shader / case_shadow and tests/engine_probes.py take unchanged.

STAGES are hand-written scenes of at most 16 primitives in the shape of oracle.probes.SceneData.  Everything lies around one
column, x = y = 0: lamp 0 at z = 32, and below it on the column the occluders - a glass film one ulp short of opaque (z = 26),
four glass rectangles (z = 12 ... 18; transparencies 0.5, 0.5, 0.75, 0.75 in list order: half the limit, half, a quarter, a
quarter) and an opaque ball (z = 4) - so that the height of a point on the column says what its shadow ray meets, the ray runs
along an axis (the length of (0, 0, dz) is |dz|, a dot product with an axis is a component) and the facing films are met at
|dot| == 1.  The shader is handed the hit point and the normal: a point need not lie on the primitive it shades, which is there
for its material, its index and its type.
  room, room split   spheres and planes only: the lean sphere + plane row; the glass rectangles in one leaf / in a leaf each;
                     among the shaded balls one whose index word is the lamp's and one without a material (MATERIAL_NONE)
  carriers           spheres that carry one material each: five innerIllumination.x, five Blinn exponents, three noises
  mixed              a triangle and a cylinder beside a checkerboard, wireframe materials, and films of transparency +0, -0,
                     the smallest subnormal and 2^-126 in columns of their own: the all-features row
The record that lies BEFORE the material array is a copy of record 0 in every stage: a lamp without a material
(MATERIAL_NONE) reads materials[-1] in the reference, the engine reads record 0 in its place (rt_device.h primitiveShader), and
the stages make the two the same memory.  TextScene gives the text model the same reading.

A FAMILY is one stage, one light list, one SceneInfo, and elements that differ in ONE binary32 input (stepped with
primitive_edge_cases.step across the analytically placed decision) or one small integer.  It names its decision and, where it
claims an equality, the mutant of the text model (tests/test_shader_edge_cases.py MUTANTS) that can differ from the model only
ON it.  Families with the same stage, lights and SceneInfo share a case.  Groups: `dyadic` (shadowIntensity 1,
backgroundColor.w 0, geometryEpsilon 2^-10, rayEpsilon 0), `dyadic half` (0.5, 0.25), `decimal` (0.9, 0.05, 0.001, 0.05: no
equality is claimed).  OFFSETS - consecutive floats - step the families ON an equality of the `dyadic` group; the others step
geometrically.  Nothing here judges a result."""
import numpy as np

import cuda_text_model as M
from primitive_edge_cases import COARSE, OFFSETS, SPARSE, WAVE, step

f4, i4 = np.float32, np.int32
TINY, MIN = f4(2.0 ** -149), f4(2.0 ** -126)          # the smallest subnormal, the smallest normal number
E2 = 2.0 ** -10
VIEW_DISTANCE = 50000.0
LAMP_Z = 32.0
GROUPS = {
    "dyadic": dict(shadowIntensity=1.0, background_w=0.0, geometryEpsilon=E2, rayEpsilon=0.0),
    "dyadic half": dict(shadowIntensity=0.5, background_w=0.25, geometryEpsilon=E2, rayEpsilon=0.0),
    "decimal": dict(shadowIntensity=0.9, background_w=0.05, geometryEpsilon=0.001, rayEpsilon=0.05),
}
ABOVE_4096 = float(np.nextafter(f4(4096.0), f4(8192.0)))

# ---- materials ------------------------------------------------------------------------------------------------------------
(BEFORE, PLAIN, GLASS, GLASS_D, GLASS75, ALMOST, LAMP, LAMP_STILL, EMISSIVE, WIRE1, WIRE2, X_M0, X_SUB, X_MIN, X_E10, POW_0, POW_1,
 POW_2, POW_4096, POW_ABOVE, N_M0, N_SUB, N_7, T_P0, T_M0, T_SUB, T_MIN, OPAQUE) = range(28)
NB_MATERIALS = 28


def materials(dtype, overrides=()):
    """-> the material array; the record before it (what materials[MATERIAL_NONE] reads) is a copy of record 0.
    overrides: ((material, field, component or None, value), ...)"""
    full = np.zeros(65506 + 30 + 2, dtype)
    m = full[1:]
    n = NB_MATERIALS
    for key in ("textureIds", "advancedTextureIds", "textureOffset", "advancedTextureOffset"):
        m[key][:n] = -1
    m["color"][:n] = (0.5, 0.25, 0.75, 0.0)
    m["specular"][:n] = (0.5, 2.0, 0.25, 0.0)
    # record 0: what a lamp without a material is read as - a range and a jitter like the lamp's, another strength
    m["innerIllumination"][BEFORE] = (0.25, 0.25, 64.0, 0.0)
    m["color"][BEFORE] = (1.0, 1.0, 1.0, 0.0)
    m["innerIllumination"][LAMP] = (0.5, 0.25, 64.0, 0.0)
    m["innerIllumination"][LAMP_STILL] = (0.5, 0.0, 64.0, 0.0)
    m["color"][LAMP], m["color"][LAMP_STILL] = (1.0, 1.0, 1.0, 0.0), (1.0, 1.0, 1.0, 0.0)
    for k, t, colour in ((GLASS, 0.5, (0.5, 0.25, 0.125)), (GLASS_D, 0.5, (0.125, 0.5, 0.25)), (GLASS75, 0.75, (0.25, 0.125, 0.5)),
                         (ALMOST, 2.0 ** -24, (0.75, 0.5, 0.25)), (T_P0, 0.0, (0.5, 0.25, 0.125)), (T_M0, -0.0, (0.5, 0.25, 0.125)),
                         (T_SUB, TINY, (0.5, 0.25, 0.125)), (T_MIN, MIN, (0.5, 0.25, 0.125))):
        m["transparency"][k], m["color"][k, :3] = t, colour
        m["refraction"][k], m["reflection"][k], m["opacity"][k] = 1.1, 0.5, 0.2
    m["innerIllumination"][EMISSIVE, 0] = 2.0 ** -10
    m["attributes"][WIRE1, 2], m["attributes"][WIRE2, 2] = 1, 2
    for k, x in ((X_M0, -0.0), (X_SUB, TINY), (X_MIN, MIN), (X_E10, 2.0 ** -10)):
        m["innerIllumination"][k, 0] = x
    for k, e in ((POW_0, 0.0), (POW_1, 1.0), (POW_2, 2.0), (POW_4096, 4096.0), (POW_ABOVE, ABOVE_4096)):
        m["specular"][k, 1] = e
    for k, w in ((N_M0, -0.0), (N_SUB, TINY), (N_7, 2.0 ** -7)):
        m["innerIllumination"][k, 3] = w
    for k, field, comp, value in overrides:
        if comp is None:
            m[field][k] = value
        else:
            m[field][k, comp] = value
    full[0] = full[1]
    return m


# ---- records ----------------------------------------------------------------------------------------------------------------
def _rec(P, ptype, p0, size, mat, p1=(0, 0, 0), p2=(0, 0, 0), n=(0, 0, 0)):
    p = np.zeros(1, P)[0]
    p["type"], p["p0"], p["p1"], p["p2"], p["size"], p["materialId"] = ptype, p0, p1, p2, size, mat
    p["n0"], p["n1"], p["n2"] = n, n, n
    p["vt1"], p["vt2"] = (1.0, 0.0), (0.0, 1.0)
    return p


def _ball(P, p0, mat, r=1.0):
    return _rec(P, M.ptSphere, p0, (r, 0, 0), mat)


def _film(P, z, mat, x=0.0, n=(0, 0, 1)):
    """a rectangle across the column at height z, 4 x 4"""
    return _rec(P, M.ptXYPlane, (x, 0, z), (2, 2, 0), mat, n=n)


def _reach(r):
    t = int(r["type"])
    reach = np.full(3, r["size"][0], f4) if t in (M.ptSphere, M.ptCylinder) else np.abs(r["size"]).astype(f4)
    pts = [r["p0"] - reach, r["p0"] + reach]
    if t in (M.ptTriangle, M.ptCylinder):
        pts += [r["p1"] - reach, r["p1"] + reach, r["p2"]]
    return np.min(pts, axis=0) - f4(0.5), np.max(pts, axis=0) + f4(0.5)


LAMP_AT = ((0.0, 0.0, LAMP_Z), (0.0, 32.0, 24.0), (-32.0, 16.0, 28.0))


def _stage_records(P, name):
    """-> [(name, record)], [leaves as lists of names]"""
    floor = ("FLOOR", _rec(P, M.ptXZPlane, (0, -16, 0), (48, 0, 48), PLAIN, n=(0, 1, 0)))
    lamps = [("L%d" % k, _ball(P, LAMP_AT[k], LAMP if k != 1 else LAMP_STILL)) for k in range(3)]
    opaque = ("OPQ", _ball(P, (0, 0, 4), OPAQUE))
    if name in ("room", "room split"):
        recs = [floor, ("WALL", _rec(P, M.ptXYPlane, (0, 0, -40), (48, 48, 0), PLAIN, n=(0, 0, 1)))] + lamps + [opaque]
        glass = [("A", _film(P, 12, GLASS)), ("D", _film(P, 18, GLASS_D)), ("B", _film(P, 14, GLASS75)), ("C", _film(P, 16, GLASS75)),
                 ("ALMOST", _film(P, 26, ALMOST))]
        shaded = [("BALL", _ball(P, (-40, -12, 0), PLAIN)), ("GLASSBALL", _ball(P, (-40, -12, 8), GLASS)),
                  ("TWIN", _ball(P, (40, -12, 0), PLAIN)), ("EMI", _ball(P, (40, -12, 8), EMISSIVE)),
                  ("NOBALL", _ball(P, (40, -12, 16), M.MATERIAL_NONE))]      # (a primitive without a material: GI:925 reads materials[-1])
        leaves = [[n] for n, _ in recs]
        leaves += [[n] for n, _ in glass] if name == "room split" else [[n for n, _ in glass]]
        leaves += [["BALL", "GLASSBALL"], ["TWIN", "EMI", "NOBALL"]]
        return recs + glass + shaded, leaves
    if name == "carriers":
        recs = [floor, lamps[0], opaque, ("BALL", _ball(P, (-40, -12, 0), PLAIN))]
        carried = (("X_M0", X_M0), ("X_SUB", X_SUB), ("X_MIN", X_MIN), ("X_E10", X_E10), ("POW_0", POW_0), ("POW_1", POW_1),
                   ("POW_2", POW_2), ("POW_4096", POW_4096), ("POW_ABOVE", POW_ABOVE), ("N_M0", N_M0), ("N_SUB", N_SUB), ("N_7", N_7))
        balls = [(n, _ball(P, (-40 + 4 * (k % 6), -12, 8 + 8 * (k // 6)), mat)) for k, (n, mat) in enumerate(carried)]
        return recs + balls, [["FLOOR"], ["L0"], ["OPQ"], ["BALL"] + [n for n, _ in balls[:5]], [n for n, _ in balls[5:]]]
    assert name == "mixed"
    films = [("F_P0", _film(P, 8, T_P0, 0.0)), ("F_M0", _film(P, 8, T_M0, 8.0)), ("F_SUB", _film(P, 8, T_SUB, 16.0)),
             ("F_MIN", _film(P, 8, T_MIN, 24.0)), ("GRAZE", _film(P, 8, GLASS, 32.0, n=(1, 0, 0)))]
    others = [("TRI", _rec(P, M.ptTriangle, (-44, -12, 0), (0, 0, 0), PLAIN, p1=(-40, -12, 0), p2=(-44, -8, 0), n=(0, 0, 1))),
              ("CYL", _rec(P, M.ptCylinder, (-44, -12, 8), (1, 1, 1), PLAIN, p1=(-44, -8, 8), p2=(-44, -10, 8), n=(0, 1, 0))),
              ("CHECKER", _rec(P, M.ptCheckboard, (0, -14, 0), (4, 0, 4), PLAIN, n=(0, 1, 0))),
              ("BALL", _ball(P, (-40, -12, 16), PLAIN)), ("WIREBALL", _ball(P, (40, -12, 16), WIRE1)),
              ("WIRE2BALL", _ball(P, (40, -12, 8), WIRE2)), ("ELL", _rec(P, M.ptEllipsoid, (40, -12, 0), (2, 1, 1), PLAIN))]
    recs = [floor, lamps[0]] + films + others
    return recs, [["FLOOR"], ["L0"], [n for n, _ in films], ["TRI", "CYL"], ["CHECKER"], ["BALL", "WIREBALL", "WIRE2BALL", "ELL"]]


LIGHTS = {          # name -> [(lamp primitive, material, colour)]
    "one": [("L0", LAMP)],
    "bare": [("L0", M.MATERIAL_NONE)],
    "two": [("L0", LAMP), ("L1", LAMP_STILL)],
    "three": [("L0", LAMP), ("L1", LAMP_STILL), ("L2", LAMP)],
}
LIGHT_COLOURS = ((1.0, 0.5, 0.25, 2.0), (0.25, 1.0, 0.5, 1.0), (0.5, 0.25, 1.0, 0.5))


def scene_info(group, **overrides):
    from oracle import probes
    g = dict(GROUPS[group])
    w = g.pop("background_w")
    g.update(overrides)
    si = probes._scene_info(viewDistance=VIEW_DISTANCE, maxPathTracingIterations=20, **g)
    si.backgroundColor[3] = w
    return si


class Stage:
    """hand-made arrays in the shape of oracle.probes.SceneData (as tests/walk_margin_cases.py Scene)"""

    def __init__(self, solr, name, lights, si, mats=()):
        from oracle import loader, probes
        self._loader = loader
        self.name = name
        recs, leaves = _stage_records(solr.PRIMITIVE_DTYPE, name)
        self.names = {n: k for k, (n, _) in enumerate(recs)}
        assert len(recs) <= 16 and [n for leaf in leaves for n in leaf] == [n for n, _ in recs], name
        self.prims = np.zeros(len(recs), solr.PRIMITIVE_DTYPE)
        for k, (_, r) in enumerate(recs):
            self.prims[k] = r
        self.prims["index"] = np.arange(len(recs))
        if "TWIN" in self.names:          # a primitive that is no lamp and carries the lamp's index word
            self.prims["index"][self.names["TWIN"]] = self.names["L0"]
        self.boxes = np.zeros(len(leaves) + 1, solr.BOX_DTYPE)
        start = 0
        for k, leaf in enumerate(leaves):
            lo, hi = zip(*[_reach(self.prims[self.names[n]]) for n in leaf])
            b = self.boxes[k + 1]
            b["min"], b["max"], b["nbPrimitives"], b["startIndex"], b["indexForNextBox"] = np.min(lo, 0), np.max(hi, 0), len(leaf), start, (1, 0)
            start += len(leaf)
        self.boxes[0]["min"], self.boxes[0]["max"] = self.boxes["min"][1:].min(axis=0), self.boxes["max"][1:].max(axis=0)
        self.boxes[0]["indexForNextBox"] = (len(self.boxes), 0)
        self.materials = materials(solr.MATERIAL_DTYPE, mats)
        self.textures = np.zeros(16, np.uint8)
        chosen = LIGHTS[lights]
        self.lights = np.zeros(len(chosen), solr.LIGHT_DTYPE)
        for k, (lamp, mat) in enumerate(chosen):
            at = self.names[lamp]
            self.lights[k]["primitiveId"], self.lights[k]["materialId"] = at, mat
            self.lights[k]["location"], self.lights[k]["color"] = self.prims["p0"][at], LIGHT_COLOURS[k]
        self.nb_lamps = len(chosen)
        self.randoms = probes.default_randoms()
        self.si = si
        self.ppi = solr.PostProcessingInfo()

    def oracle_scene(self):
        return self._loader.OracleScene(self.boxes.ctypes.data, len(self.boxes), self.prims.ctypes.data, len(self.prims),
                                        self.lights.ctypes.data, len(self.lights), self.nb_lamps, self.materials.ctypes.data,
                                        self.textures.ctypes.data, self.randoms.ctypes.data, len(self.randoms))


class TextScene(M.Scene):
    """the text model's scene of a stage: materials[MATERIAL_NONE] is the record before the array - in a stage a copy of record 0"""

    def __init__(self, stage):
        import types
        super().__init__(types.SimpleNamespace(boxes=stage.boxes, primitives=stage.prims, lights=stage.lights,
                                               materials=stage.materials[:NB_MATERIALS], randoms=stage.randoms))

    def material(self, i):
        return self.M[0] if i == M.MATERIAL_NONE else super().material(i)


# ---- families -----------------------------------------------------------------------------------------------------------------
BASE = dict(index=0, eye=(0.0, 0.0, 30.0), normal=(0.0, 0.0, 1.0), shade="BALL", inter=(0.0, 0.0, 28.0), areas=(0.0, 0.0, 0.0),
            closest_color=(0.0, 0.0, 0.0), iteration=0, total_blinn=(0.0, 0.0, 0.0),
            lamp=(0.0, 0.0, LAMP_Z))                 # (lamp: the far point of a shadow case)
UNDER_THE_BALL = (0.0, 0.0, 0.0)                     # a point whose shadow ray meets the opaque ball first ...
UNDER_THE_FILM = (0.0, 0.0, 25.0)                    # ... the film one ulp short of opaque and nothing else ...
IN_THE_LIGHT = (0.0, 0.0, 28.0)                      # ... nothing
BEHIND_THE_BALL = ((0.0, -8.0, -1.0), (8.0, -4.0, -2.0))   # points from which lamp 1 / lamp 2 lies behind the opaque ball's centre


class Family:
    """kind: `shader` or `shadow`; elements: dicts over BASE; si: SceneInfo fields beside the group's; mats: material overrides;
    equality: the mutant that differs from the model only where the compared numbers are equal (None: none is claimed);
    occluded: shadow rays of the family meet something (held on the GPU)"""

    def __init__(self, decision, elements, kind="shader", stage="room", lights="one", si=(), mats=(), equality=None, occluded=False,
                 parts=None):
        self.decision, self.kind, self.stage, self.lights, self.equality, self.occluded = decision, kind, stage, lights, equality, occluded
        # parts: the family's ONE input is a SceneInfo field or a material's - its elements once per (si, mats) of the list
        parts = [dict(si=si, mats=mats)] if parts is None else parts
        self.keys = [(kind, stage, lights, tuple(sorted(dict(p.get("si", ())).items())), tuple(p.get("mats", ()))) for p in parts]
        self.elements = [dict(BASE, **e) for e in elements]


def _set(vec, axis, value):
    out = [float(x) for x in vec]
    out[axis] = float(value)
    return tuple(out)


def stepped(field, vec, axis, offsets, **more):
    """elements that differ in component `axis` of `field`: the floats `offsets` places from vec[axis]"""
    return [dict(more, **{field: _set(vec, axis, x)}) for x in step(vec[axis], offsets)]


AROUND_ZERO = [0.0, -0.0, float(TINY), -float(TINY), float(MIN), -float(MIN), 2.0 * float(MIN), -2.0 * float(MIN), 2.0 ** -100,
               -2.0 ** -100, 2.0 ** -24, -2.0 ** -24]


def half_normal():
    """an input normal (x, 0, 1) that the text's normalize - v * (1.f / sqrtf(dot)) - turns into (., 0, 0.5) exactly"""
    x = f4(np.sqrt(3.0))
    for k in range(-8, 9):
        c = step(x, np.array([k], np.int64))[0]
        if f4(1.0) * (f4(1.0) / np.sqrt(c * c + f4(0.0) * f4(0.0) + f4(1.0) * f4(1.0))) == f4(0.5):
            return (float(c), 0.0, 1.0)
    raise AssertionError("no float near sqrt(3) gives 0.5")


def shader_families(group):
    eq = group != "decimal"
    fine = OFFSETS if group == "dyadic" else (COARSE if eq else SPARSE)     # ON an equality
    coarse = COARSE if group == "dyadic" else SPARSE
    E = lambda name: name if eq else None     # noqa: E731
    F, out = Family, []
    every_sphere = ("BALL", "GLASSBALL", "EMI")

    # range: lightRayLength < innerIllumination.z - from (0, 0, z) the light ray is (0, 0, 32 - z), 64 long at z = -32; the
    # shadow ray of a point in range meets the opaque ball
    for lights in ("one", "bare"):
        out.append(F("range: lightRayLength < innerIllumination.z", stepped("inter", (0.0, 0.0, LAMP_Z - 64.0), 2, fine, eye=(0.0, 8.0, -20.0)),
                     lights=lights, equality=E("range <"), occluded=True))
    out.append(F("photon energy: up to pred(innerIllumination.z)",
                 stepped("inter", (0.0, -64.0, LAMP_Z), 1, np.arange(0, 17), normal=(0.0, 1.0, 0.0), eye=(0.0, -60.0, 40.0))))
    # lambert: the component of the input normal along the light ray through +-0, under the opaque ball
    for shade in every_sphere:
        zs = AROUND_ZERO + [float(x) for x in step(-(2.0 ** -10), coarse)]
        out.append(F("lambert sign: normal.z through 0 (%s)" % shade, [dict(normal=(1.0, 0.0, z), inter=UNDER_THE_BALL, shade=shade) for z in zs],
                     equality=E("lambert > 0") if shade != "EMI" else None, occluded=shade != "EMI"))      # (an emissive material casts no shadow ray)
        out.append(F("lambert sign: a normal perpendicular to the light ray (%s)" % shade,
                     [dict(normal=n, inter=UNDER_THE_BALL, shade=shade) for n in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (-1.0, 0.0, 0.0),
                                                                                   (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (3.0, 4.0, 0.0))], occluded=shade != "EMI"))
    # innerIllumination.x == 0: the shadow ray and the scaling of closestColor
    xs = ("BALL", "X_M0", "X_SUB", "X_MIN", "X_E10")
    out.append(F("innerIllumination.x == 0", [dict(shade=s, inter=p, closest_color=(0.5, 0.25, 0.125)) for s in xs
                                              for p in (UNDER_THE_BALL, IN_THE_LIGHT)], stage="carriers", occluded=True))
    # integers
    out.append(F("iteration < 4", [dict(iteration=i, inter=p) for i in (3, 4, 5) for p in (UNDER_THE_BALL, UNDER_THE_FILM, IN_THE_LIGHT)],
                 equality=E("iteration < 4"), occluded=True))
    points = [dict(inter=p, shade=s, closest_color=(0.5, 0.25, 0.125), total_blinn=(0.125, 0.0, 0.25))
              for p in (UNDER_THE_BALL, UNDER_THE_FILM, IN_THE_LIGHT) for s in ("BALL", "EMI", "NOBALL", "L0")]
    out.append(F("graphicsLevel 0 ... 4", points, parts=[dict(si=dict(graphicsLevel=level)) for level in range(5)], occluded=True))
    out.append(F("attributes.z 0 / 1 / 2 (the wireframe return)",
                 [dict(shade=s, inter=p, closest_color=(0.5, 0.25, 0.125)) for s in ("BALL", "WIREBALL", "WIRE2BALL") for p in ((0.0, 0.0, 0.0), IN_THE_LIGHT)],
                 stage="mixed", parts=[dict(si=dict(graphicsLevel=level)) for level in (4, 0)], equality=E("wireframe == 1"), occluded=True))
    indices = (0, 1000, M.MAX_BITMAP_SIZE - 21, M.MAX_BITMAP_SIZE - 20, M.MAX_BITMAP_SIZE - 19, M.MAX_BITMAP_SIZE - 1)
    for lights, claim in (("one", "pass >= 10 (the jitter)"), ("two", None), ("three", "pass >= 10 (the lamp choice)")):
        out.append(F("pathTracingIteration 9 ... 12, %s" % lights,
                     [dict(index=i, inter=p) for i in indices for p in (UNDER_THE_BALL, IN_THE_LIGHT, (0.0, 24.0, 24.0)) + BEHIND_THE_BALL], lights=lights,
                     parts=[dict(si=dict(pathTracingIteration=it, timestamp=17)) for it in (9, 10, 11, 12)], equality=E(claim) if claim else None,
                     occluded=True))
    # lit: the lamp's own primitive, a primitive with the lamp's index word, their neighbours
    out.append(F("lit: lightPrimitiveId != index", [dict(shade=s, inter=IN_THE_LIGHT, closest_color=(0.5, 0.25, 0.125))
                                                    for s in ("L0", "TWIN", "L1", "OPQ", "EMI", "NOBALL")]))
    # the lamp loop: lamp 0 nbLights times below pass 10, saturation after every trip
    presets = [dict(shade=s, inter=p, closest_color=c, total_blinn=b)
               for s in ("BALL", "EMI", "L1") for p in (IN_THE_LIGHT, UNDER_THE_BALL, (0.0, 0.0, 13.0))
               for c in ((0.0, 0.0, 0.0), (0.5, 0.75, 1.0), (1024.0, -1024.0, -2048.0)) for b in ((0.0, 0.0, 0.0), (0.5, 0.75, 0.9375), (-2.0, -0.5, 2.0))]
    for lights in ("two", "three"):
        out.append(F("lamp loop: lamp 0 shaded %s times, saturation per trip" % lights, presets, lights=lights, occluded=True))
    out.append(F("lamp loop: one lamp, the same presets", presets, occluded=True))
    # the Blinn gate: the shadow at the limit (opaque), one ulp below it (the film), 0
    for lights in ("one", "bare"):
        out.append(F("Blinn gate: shadowIntensity < si.shadowIntensity", [dict(inter=p) for p in (UNDER_THE_BALL, UNDER_THE_FILM, IN_THE_LIGHT,
                                                                                                   (0.0, 0.0, 8.0), (0.0, 0.0, 13.0), (0.0, 0.0, 15.0))],
                     lights=lights, equality=E("Blinn gate <"), occluded=True))
    # temp != 0: eye, point and lamp on the column, the point between them - view ray == light ray
    out.append(F("temp != 0: the eye stepped off the axis", stepped("eye", (0.0, 0.0, 20.0), 0, fine) +
                 [dict(eye=(x, 0.0, 20.0)) for x in (2.0 ** -60, 2.0 ** -30, 2.0 ** -12, -2.0 ** -6, 1.0, -1.0)], equality=E("temp != 0")))
    # blinnTerm < 0: the half vector is (0, 0, 1), the Blinn base the normalised normal's z
    out.append(F("blinnTerm < 0: normal.z through 0", [dict(normal=(1.0, 0.0, z)) for z in AROUND_ZERO + [0.5, -0.5, 1.0, -1.0]]))
    # the power: only pairs whose power is a binary32 number
    bases = {"+0": (1.0, 0.0, 0.0), "subnormal": (1.0, 0.0, float(TINY)), "2^-126": (1.0, 0.0, float(MIN)), "0.5": half_normal(),
             "1": (0.0, 0.0, 1.0)}
    exact = {"POW_0": bases, "POW_1": bases, "POW_2": ("+0", "0.5", "1"), "POW_4096": ("+0", "1"), "POW_ABOVE": ("+0", "1"), "BALL": ("+0", "0.5", "1")}
    out.append(F("power domain: bases +0 ... 1, exponents 0 ... above 4096",
                 [dict(shade=s, normal=bases[b]) for s, bs in exact.items() for b in bs] * 2, stage="carriers"))
    # the noise: innerIllumination.w against known entries of the random buffer, picked by index / timestamp pairs (one wraps)
    out.append(F("noise: innerIllumination.w != 0", [dict(shade=s, index=i) for s in ("BALL", "N_M0", "N_SUB", "N_7") for i in (0, 1, 1000, 2073000)],
                 stage="carriers", parts=[dict(), dict(si=dict(timestamp=17)), dict(si=dict(timestamp=2073600 - 3 - 1000))]))
    # glNoShading returns the texel; the checkerboard's parity of (int)(viewDistance + (x - p0.x) / size.x): two cell borders
    for level in (0, 4):
        for border in (4.0, 8.0):
            out.append(F("checkerboard: the cell border at x = %d, graphicsLevel %d" % (border, level),
                         stepped("inter", (border, -14.0, 2.0), 0, fine, shade="CHECKER", normal=(0.0, 1.0, 0.0), eye=(0.0, 0.0, 30.0)),
                         stage="mixed", si=dict(graphicsLevel=level)))
    out.append(F("every type shaded", [dict(shade=s, inter=p) for s in ("TRI", "CYL", "CHECKER", "BALL", "F_P0") for p in ((0.0, 0.0, 0.0), IN_THE_LIGHT)],
                 stage="mixed", occluded=True))
    return out


def shadow_families(group):
    eq = group != "decimal"
    fine = OFFSETS if group == "dyadic" else (COARSE if eq else SPARSE)
    E = lambda name: name if eq else None     # noqa: E731
    F, out = Family, []
    heights = (-8.0, 2.0, 8.0, 13.0, 15.0, 17.0, 25.0, 28.0)
    column = [dict(inter=(0.0, 0.0, z), shade=s) for z in heights for s in ("BALL", "A", "D")]
    half = f4(0.5)
    for stage in ("room", "room split"):
        # D's transparency around 0.5: the sum of A and D (list order) below, ON and above the limit
        around = (float(np.nextafter(half, f4(1.0))), 0.5, float(np.nextafter(half, f4(0.0))))
        out.append(F("early exit: result < shadowIntensity, D's transparency around 0.5", column, kind="shadow", stage=stage,
                     parts=[dict(mats=((GLASS_D, "transparency", None, t),)) for t in around], equality=E("shadow exit <"), occluded=True))
        out.append(F("final clamp: shadowIntensity 0 and the group's", column, kind="shadow", stage=stage,
                     parts=[dict(si=dict(shadowIntensity=0.0)), dict()], occluded=True))
    out.append(F("final clamp: a sum below 0 (D's transparency 2.5)", column, kind="shadow", mats=((GLASS_D, "transparency", None, 2.5),),
                 occluded=True))
    # the occluder's transparency != 0: +0, -0, the smallest subnormal, 2^-126, each film in a column of its own
    films = [dict(inter=(x, 0.0, z), lamp=(x, 0.0, LAMP_Z)) for x in (0.0, 8.0, 16.0, 24.0) for z in (0.0, 12.0)]
    out.append(F("transparency != 0: +0, -0, subnormal, 2^-126", films, kind="shadow", stage="mixed", occluded=True))
    # grazing: the film's normal is (1, 0, 0), the ray runs along z; the lamp stepped sideways
    out.append(F("grazing: a glass film whose normal is perpendicular to the ray", stepped("lamp", (32.0, 0.0, LAMP_Z), 0, fine, inter=(32.0, 0.0, 0.0)),
                 kind="shadow", stage="mixed", occluded=True))
    return out


def families(group):
    return shader_families(group) + shadow_families(group)


# ---- cases ----------------------------------------------------------------------------------------------------------------------
_CASES = {}


def cases(solr, group):
    """-> [(case, families of the group, stage)]: families that share stage, lights, SceneInfo and materials share a case;
    case["family"]: per element, the family's number in families(group); case["occluded"]: per element"""
    if group in _CASES:
        return _CASES[group]
    fams = families(group)
    keys = []
    for f in fams:
        keys += [k for k in f.keys if k not in keys]
    out = []
    for key in keys:
        kind, stage_name, lights, si, mats = key
        stage = Stage(solr, stage_name, lights, scene_info(group, **dict(si)), mats)
        elements, family, occluded = [], [], []
        for j, f in enumerate(fams):
            if key in f.keys:
                elements += f.elements
                family += [j] * len(f.elements)
                occluded += [f.occluded] * len(f.elements)
        n = len(elements)
        col = lambda k, dtype=f4: np.ascontiguousarray(np.array([e[k] for e in elements], dtype))     # noqa: E731
        shaded = np.array([stage.names[e["shade"]] for e in elements], i4)
        common = dict(scene=stage, si=stage.si, iteration=col("iteration", i4), family=np.array(family, i4),
                      occluded=np.array(occluded, bool), key=repr(key))
        if kind == "shader":
            mats_of = stage.materials[stage.prims["materialId"][shaded]]
            attributes = np.stack([mats_of["reflection"], mats_of["transparency"], mats_of["refraction"], mats_of["opacity"]], 1).astype(f4)
            case = dict(name="shader", ppi=stage.ppi, index=col("index", i4), origins=col("eye"), normal=col("normal"), object_id=shaded,
                        inter=col("inter"), areas=col("areas"), closest_color=col("closest_color"), total_blinn=col("total_blinn"),
                        attributes=np.ascontiguousarray(attributes), **common)
        else:
            case = dict(name="shadow", lamps=col("lamp"), origins=col("inter"), object_id=np.full(n, stage.names["L0"], i4), shaded=shaded,
                        **common)
        out.append((case, fams, stage))
    _CASES[group] = out
    return out


PER_ELEMENT = {"shader": ("index", "origins", "normal", "object_id", "inter", "areas", "closest_color", "total_blinn", "attributes",
                          "iteration", "family", "occluded"),
               "shadow": ("lamps", "origins", "object_id", "shaded", "iteration", "family", "occluded")}


def reordered(case, order):
    """the same case with its elements in another order (elements may repeat)"""
    order = np.asarray(order)
    out = dict(case)
    for k in PER_ELEMENT[case["name"]]:
        out[k] = np.ascontiguousarray(case[k][order])
    return out


def orders(n):
    """name -> order: as built (sorted by family: pure waves); interleaved by a fixed stride (every wave mixes the families);
    ragged (the elements once, then the first ones again until the count is 37 beyond a multiple of 64)"""
    stride = 37                                    # (coprime to any n that is no multiple of 37: checked)
    while np.gcd(stride, n) != 1:
        stride += 2
    base = np.arange(n)
    return {"sorted": base, "interleaved": (base * stride) % n, "ragged": np.resize(base, n + (37 - n) % WAVE)}


def digest(case):
    """sha1 over the arrays of a case and of its stage"""
    from oracle import probes
    s = case["scene"]
    flat = {k: v for k, v in case.items() if k not in ("scene", "key")}
    flat.update(z_boxes=s.boxes, z_prims=s.prims, z_lights=s.lights, z_materials=s.materials[:NB_MATERIALS],
                z_before=s.materials.base[:1])
    return probes.input_digest(flat)
