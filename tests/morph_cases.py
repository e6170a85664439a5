"""Key-frame scenes for the morphing tests (tests/test_morph_host.py, tests/test_morph_gpu.py): four small scenes at
96 x 64, each with a first key frame (frame 0), a last key frame (frame 2) and the frame between them as
GPUKernel::morphPrimitives makes it (frame 1, the current frame when build() returns, flattened).

  mesh        13 x 13 vertices = 288 triangles with per-vertex normals and texture coordinates, a lamp and a backdrop
              plane: heights and normals differ between the keys; 290 primitives cross one 256-thread block and end in a
              partly filled wave
  sticks      40 spheres, 39 cylinders, 3 cones, 2 ellipsoids and a lamp: positions and radii differ; fewer than two
              waves, the second one ragged
  mix         every primitive type the walks dispatch on, the three planes and the checkerboard among them; one
              unmovable primitive, glass, a mirror and a textured triangle
  lamp_moves  sticks with the lamp at another place in the last key frame

Also the binary32 model of the blend the tests hold the engines to (morph_model)."""
import importlib
import math

import numpy as np

solr = importlib.import_module("sol-r_amd")
S = solr.scenes

WIDTH, HEIGHT = 96, 64
NAMES = ("mesh", "sticks", "mix", "lamp_moves")


def _materials(k, name):
    rng = S.LCG(31)
    m = dict(walls=[k.add_material(*S._wall_color(rng), specValue=0.6, specPower=80.0) for _ in range(6)])
    if name == "mix":
        m["mirror"] = k.add_material(0.2, 0.6, 0.8, reflection=0.6, specValue=1.0, specPower=200.0)
        m["glass"] = k.add_material(0.9, 0.95, 1.0, reflection=0.8, refraction=1.2, transparency=0.6, opacity=0.2,
                                    specValue=1.0, specPower=150.0)
        rs = np.random.RandomState(5)
        k.set_texture(0, rs.randint(0, 256, size=(16, 32, 3)).astype(np.uint8), texture_type=0)
        m["textured"] = k.add_material(1, 1, 1, diffuseTextureId=0)
        m["wire"] = k.add_material(1.0, 1.0, 0.2, wireframe=True, wireframeWidth=0)
    m["lamp"] = k.add_material(1.0, 1.0, 1.0, innerIllumination=2.0)
    return m


def _lamp(k, m, position):
    return k.add_primitive(solr.ptSphere, position, size=(10.0, 0, 0), material=m["lamp"])


def _mesh(k, m, key):
    n = 12
    phase = (0.4, 1.1, 2.0) if key == 0 else (2.3, 0.2, 4.0)
    amplitude = 1500.0 if key == 0 else 2100.0

    def point(i, j):
        u, v = (i / n) * 2.0 - 1.0, (j / n) * 2.0 - 1.0
        y = amplitude * (math.sin(3.0 * u + phase[0]) * math.cos(2.0 * v + phase[1]) + 0.5 * math.sin(5.0 * u + 4.0 * v + phase[2]))
        return (u * 7000.0, y - 2000.0, v * 7000.0)

    def normal(i, j):
        a, b, c, d = point(i - 1, j), point(i + 1, j), point(i, j - 1), point(i, j + 1)
        tx = (b[0] - a[0], b[1] - a[1], b[2] - a[2])
        tz = (d[0] - c[0], d[1] - c[1], d[2] - c[2])
        return (tz[1] * tx[2] - tz[2] * tx[1], tz[2] * tx[0] - tz[0] * tx[2], tz[0] * tx[1] - tz[1] * tx[0])

    def uv(i, j):
        return (i / n, j / n)

    for i in range(n):
        for j in range(n):
            mat = m["walls"][(i // 4 + j // 4) % 6]
            corners = [(i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1)]
            for tri in ((0, 1, 2), (0, 2, 3)):
                c = [corners[t] for t in tri]
                t = k.add_primitive(solr.ptTriangle, point(*c[0]), point(*c[1]), point(*c[2]), material=mat)
                k.set_normals(t, normal(*c[0]), normal(*c[1]), normal(*c[2]))
                k.set_texture_coordinates(t, uv(*c[0]), uv(*c[1]), uv(*c[2]))
    _lamp(k, m, (8000.0, 8000.0, -8000.0))
    k.add_primitive(solr.ptXYPlane, (0.0, 0.0, 9000.0 if key == 0 else 9600.0), size=(12000.0, 9000.0, 0.0),
                    material=m["walls"][0])


def _sticks(k, m, key, lamp_moves=False, one_more=False, swap_type=False):
    rng = S.LCG(99 if key == 0 else 177)
    prev = None
    for a in range(40):
        turn = 0.5 * a + (0.0 if key == 0 else 0.35)
        p = (3500.0 * math.cos(turn) + rng.uniform(-200, 200), -3000.0 + 150.0 * a + (0.0 if key == 0 else 400.0),
             3500.0 * math.sin(turn))
        kind = solr.ptEllipsoid if (swap_type and key == 2 and a == 7) else solr.ptSphere
        k.add_primitive(kind, p, size=(250.0 + 10 * (a % 7) + (0.0 if key == 0 else 60.0), 0, 0), material=m["walls"][a % 6])
        if prev:
            k.add_primitive(solr.ptCylinder, prev, p, size=(80.0 if key == 0 else 110.0, 0, 0), material=m["walls"][(a + 1) % 6])
        prev = p
    for c in range(3):
        x = -2500.0 + 2500.0 * c
        k.add_primitive(solr.ptCone, (x, -3500.0, -1500.0), (x + (300.0 if key == 0 else -500.0), -1200.0 - 300.0 * key, -1800.0),
                        size=(300.0 + 40.0 * c + 30.0 * key, 0, 0), material=m["walls"][c])
    for e in range(2):
        k.add_primitive(solr.ptEllipsoid, (-1500.0 + 3000.0 * e, 3500.0 - 250.0 * key, 500.0),
                        size=(900.0 + 100.0 * key, 400.0, 600.0 - 50.0 * key), material=m["walls"][3 + e])
    _lamp(k, m, (-1000.0, 6500.0, -12000.0) if (lamp_moves and key == 2) else (-5000.0, 5000.0, -15000.0))
    if one_more and key == 2:
        k.add_primitive(solr.ptSphere, (0.0, 0.0, 0.0), size=(100.0, 0, 0), material=m["walls"][0])


def _mix(k, m, key):
    d = 0.0 if key == 0 else 1.0   # how far the last key frame is from the first
    w = m["walls"]
    k.add_primitive(solr.ptSphere, (-3000 + 500 * d, 500, 0), size=(1500 - 300 * d, 0, 0), material=m["mirror"])
    k.add_primitive(solr.ptSphere, (800, -500 + 700 * d, -2500), size=(1100 + 200 * d, 0, 0), material=m["glass"])
    fixed = k.add_primitive(solr.ptSphere, (3200 - 400 * d, 900, 500 + 300 * d), size=(1300, 0, 0), material=w[1])
    k.set_movable(fixed, False)
    k.add_primitive(solr.ptEllipsoid, (0, -2500 - 300 * d, 1000), size=(2200 - 500 * d, 700 + 200 * d, 1200), material=w[2])
    k.add_primitive(solr.ptCylinder, (-4500, -3000 + 600 * d, -1000), (-2500 - 700 * d, 2500, 500), size=(350 + 100 * d, 0, 0),
                    material=w[3])
    k.add_primitive(solr.ptCone, (4500, -3500, 0), (3800 + 600 * d, 1500 - 400 * d, -800), size=(400 - 80 * d, 0, 0),
                    material=m["mirror"])
    for i in range(6):   # a small fan of triangles with interpolated normals; the odd ones textured
        a0, a1 = 0.6 * i + 0.2 * d, 0.6 * (i + 1) + 0.2 * d
        p0 = (0.0, 3500.0 + 500.0 * d, 2500.0)
        p1 = (2500.0 * math.cos(a0), 3500.0 + 900.0 * math.sin(3 * a0), 2500.0 + 2500.0 * math.sin(a0))
        p2 = (2500.0 * math.cos(a1), 3500.0 + 900.0 * math.sin(3 * a1), 2500.0 + 2500.0 * math.sin(a1))
        t = k.add_primitive(solr.ptTriangle, p0, p1, p2, material=m["textured"] if i % 2 else w[4])
        k.set_normals(t, (0.1 + 0.2 * d, -1, 0.2), (0.3 * math.cos(a0), -1, 0.3 * math.sin(a0)),
                      (0.3 * math.cos(a1), -1, 0.3 * math.sin(a1)))
        k.set_texture_coordinates(t, (0.1, 0.1), (0.9, 0.2), (0.4, 0.95))
    k.add_primitive(solr.ptTriangle, (-6000, -4000, 3000), (-4000, -4000 + 800 * d, 3000), (-5000, -1500, 3500 - 600 * d),
                    material=w[5])   # (no normals of its own: its keys hold the face normals setPrimitive derived)
    k.add_primitive(solr.ptXYPlane, (0, 0, 9000 + 700 * d), size=(9000, 6000 + 500 * d, 0), material=w[0])
    k.add_primitive(solr.ptYZPlane, (-9000 - 400 * d, 0, 3000), size=(0, 6000, 6000), material=w[1])
    k.add_primitive(solr.ptYZPlane, (9000, 0, 3000 + 300 * d), size=(0, 6000, 6000 - 800 * d), material=w[2])
    k.add_primitive(solr.ptXZPlane, (0, 6000 + 500 * d, 3000), size=(9000, 0, 6000), material=m["wire"])
    k.add_primitive(solr.ptCheckboard, (0, -4500 - 300 * d, 2000), size=(9000 - 1000 * d, 0, 7000), material=w[3])
    _lamp(k, m, (6000.0, 7000.0, -9000.0))


def _key_frame(k, m, name, key, **flaws):
    if name == "mesh":
        _mesh(k, m, key)
    elif name == "mix":
        _mix(k, m, key)
    else:
        _sticks(k, m, key, lamp_moves=(name == "lamp_moves"), **flaws)


def build(k, name, nb_frames=3, morph=True, **flaws):
    """the scene `name` in kernel k: key frames 0 and nb_frames - 1 and - morph - the frames between them by
    morph_primitives, frame 1 current and flattened.  flaws: one_more (a primitive more in the last key frame), swap_type
    (one primitive of the last key frame of another type) - of the sticks only"""
    assert name in NAMES
    k.initialize(width=WIDTH, height=HEIGHT, nbRayIterations=3 if name == "mix" else 2)
    m = _materials(k, name)
    k.set_nb_frames(nb_frames)
    for key in (0, 2):
        k.set_frame(0 if key == 0 else nb_frames - 1)
        _key_frame(k, m, name, key, **flaws)
        k.compact_boxes(True)
    if morph and nb_frames > 2:
        k.morph_primitives()
        k.set_frame(1)
        k.compact_boxes(False)
    if name == "mesh":
        k.set_camera((0.0, 4000.0, -15000.0))
    elif name == "mix":
        k.set_camera((200.0, 300.0, -14000.0), look_at=(0.0, 0.0, 0.0), angles=(0.05, -0.1, 0.02))
    else:
        k.set_camera((0.0, 0.0, -14000.0))
    return k


def key_frames(k, nb_frames=3):
    """the flattened primitives of the two key frames of kernel k by rank in id order (the current frame is 1 again
    afterwards, flattened anew)"""
    keys = []
    for frame in (0, nb_frames - 1):
        k.set_frame(frame)
        k.compact_boxes(False)
        p = k.flat_scene().primitives
        keys.append(p[np.argsort(p["index"], kind="stable")])
    k.set_frame(1)
    k.compact_boxes(False)
    return keys


def _normalized(v):
    """GPUKernel::normalizeVector on (n, 3) binary32: division by the length, a zero vector left alone"""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    length = np.sqrt(x * x + y * y + z * z)   # ((x * x + y * y) + z * z), every step binary32
    out = v.copy()
    moving = length != 0
    out[moving] = v[moving] / length[moving, None]
    return out


def morph_model(first, last, current, weight):
    """What morph_frame(weight) leaves of the flattened primitives `current`, from the key frames by rank (key_frames):
    GPUKernel::morphPrimitives' statements with r = weight, every operation a binary32 step of its own."""
    assert first.dtype == solr.PRIMITIVE_DTYPE and len(first) == len(last) == len(current)
    ids = np.sort(current["index"])
    rank = np.searchsorted(ids, current["index"])
    a, b = first[rank], last[rank]
    r = np.float32(weight)
    f32 = np.float32

    def mix(field):
        x, y = a[field].astype(f32), b[field].astype(f32)
        return (x + (r * (y - x)).astype(f32)).astype(f32)

    out = current.copy()
    kind = a["type"]
    p0, p1, p2, size = mix("p0"), mix("p1"), mix("p2"), mix("size")
    n0 = np.zeros_like(p0)
    n1, n2 = n0.copy(), n0.copy()
    # setPrimitive: what it derives per type
    ball = np.isin(kind, (solr.ptSphere, solr.ptCylinder, solr.ptCone))
    size[ball] = size[ball][:, [0, 0, 0]]
    rod = np.isin(kind, (solr.ptCylinder, solr.ptCone))
    axis = _normalized((p1 - p0).astype(f32))
    n1[rod] = axis[rod]
    p2[rod] = ((p0[rod] + p1[rod]).astype(f32) / f32(2)).astype(f32)
    for plane, normal in ((solr.ptXYPlane, (0, 0, 1)), (solr.ptYZPlane, (1, 0, 0)), (solr.ptXZPlane, (0, 1, 0)),
                          (solr.ptCheckboard, (0, 1, 0))):
        n0[kind == plane] = n1[kind == plane] = n2[kind == plane] = np.array(normal, f32)
    tri = kind == solr.ptTriangle
    v0, v1 = _normalized((p1 - p0).astype(f32)), _normalized((p2 - p0).astype(f32))
    face = np.stack([(v0[:, 1] * v1[:, 2] - v0[:, 2] * v1[:, 1]).astype(f32), (v0[:, 2] * v1[:, 0] - v0[:, 0] * v1[:, 2]).astype(f32),
                     (v0[:, 0] * v1[:, 1] - v0[:, 1] * v1[:, 0]).astype(f32)], axis=1)
    face = _normalized(face)
    n0[tri] = n1[tri] = n2[tri] = face[tri]
    # setPrimitiveNormals: all three, whatever setPrimitive derived
    n0, n1, n2 = _normalized(mix("n0")), _normalized(mix("n1")), _normalized(mix("n2"))
    for field, value in (("p0", p0), ("p1", p1), ("p2", p2), ("size", size), ("n0", n0), ("n1", n1), ("n2", n2)):
        out[field] = value
    # setPrimitive's material, setPrimitiveTextureCoordinates: the first key's
    out["materialId"] = a["materialId"]
    for field in ("vt0", "vt1", "vt2"):
        out[field] = a[field]
    return out
