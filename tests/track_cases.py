"""Key-frame tracks for the tests of GPUKernel::morphBetween (tests/test_track_host.py, tests/test_track_gpu.py): five small
scenes at 96 x 64, each with K = 4 key frames of one model in frames 0 ... 3 and a stage in frame 4, built from key 0's
parameters with a tree of its own (compact_boxes(True)); the stage is the current frame when build() returns.

  mesh        13 x 13 vertices = 288 triangles with per-vertex normals and texture coordinates, a lamp and a backdrop
              plane: heights and normals differ from key to key; 290 primitives cross one 256-lane workgroup and end in a
              ragged wave
  sticks      40 spheres, 39 cylinders, 3 cones, 2 ellipsoids and a lamp, 85 primitives of four types: positions and radii
              differ
  mix         every primitive type the walks dispatch on, the three planes and the checkerboard among them; one
              unmovable primitive, glass, a mirror and a textured triangle
  lamp_moves  sticks with the lamp at another place in key 2 only
  other_uv    mesh with other texture coordinates in key 3 only

Materials, the lamp and the binary32 model of the blend are tests/morph_cases.py's (morph_model)."""
import importlib
import math

import numpy as np

import morph_cases

solr = importlib.import_module("sol-r_amd")
S = solr.scenes

WIDTH, HEIGHT = morph_cases.WIDTH, morph_cases.HEIGHT
NAMES = ("mesh", "sticks", "mix", "lamp_moves", "other_uv")
NB_KEYS = 4
KEY_FRAMES = (0, 1, 2, 3)
THIRD = float(np.float32(1) / np.float32(3))
# (frame A, frame B, weight): neighbours forwards, a weight of 0 and one of 1/3, the way back extrapolated, a key with itself
STEPS = [(0, 1, 0.5), (1, 2, 0.0), (2, 3, THIRD), (3, 0, 1.5), (1, 1, 0.3)]


def _kind(name):
    return {"lamp_moves": "sticks", "other_uv": "mesh"}.get(name, name)


def _mesh(k, m, key, other_uv=False):
    n = 12
    phase = (0.4 + 0.6 * key, 1.1 - 0.3 * key, 2.0 + 0.7 * key)
    amplitude = 1500.0 + 200.0 * key

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
        return (j / n, 1.0 - i / n) if other_uv else (i / n, j / n)

    for i in range(n):
        for j in range(n):
            mat = m["walls"][(i // 4 + j // 4) % 6]
            corners = [(i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1)]
            for tri in ((0, 1, 2), (0, 2, 3)):
                c = [corners[t] for t in tri]
                t = k.add_primitive(solr.ptTriangle, point(*c[0]), point(*c[1]), point(*c[2]), material=mat)
                k.set_normals(t, normal(*c[0]), normal(*c[1]), normal(*c[2]))
                k.set_texture_coordinates(t, uv(*c[0]), uv(*c[1]), uv(*c[2]))
    morph_cases._lamp(k, m, (8000.0, 8000.0, -8000.0))
    k.add_primitive(solr.ptXYPlane, (0.0, 0.0, 9000.0 + 200.0 * key), size=(12000.0, 9000.0, 0.0), material=m["walls"][0])


def _sticks(k, m, key, lamp_elsewhere=False, one_more=False, swap_type=False):
    rng = S.LCG(99 + 26 * key)
    prev = None
    for a in range(40):
        turn = 0.5 * a + 0.12 * key
        p = (3500.0 * math.cos(turn) + rng.uniform(-200, 200), -3000.0 + 150.0 * a + 130.0 * key, 3500.0 * math.sin(turn))
        kind = solr.ptEllipsoid if (swap_type and a == 7) else solr.ptSphere
        k.add_primitive(kind, p, size=(250.0 + 10 * (a % 7) + 20.0 * key, 0, 0), material=m["walls"][a % 6])
        if prev:
            k.add_primitive(solr.ptCylinder, prev, p, size=(80.0 + 10.0 * key, 0, 0), material=m["walls"][(a + 1) % 6])
        prev = p
    for c in range(3):
        x = -2500.0 + 2500.0 * c
        k.add_primitive(solr.ptCone, (x, -3500.0, -1500.0), (x + 300.0 - 270.0 * key, -1200.0 - 200.0 * key, -1800.0),
                        size=(300.0 + 40.0 * c + 20.0 * key, 0, 0), material=m["walls"][c])
    for e in range(2):
        k.add_primitive(solr.ptEllipsoid, (-1500.0 + 3000.0 * e, 3500.0 - 170.0 * key, 500.0),
                        size=(900.0 + 70.0 * key, 400.0, 600.0 - 30.0 * key), material=m["walls"][3 + e])
    morph_cases._lamp(k, m, (-1000.0, 6500.0, -12000.0) if lamp_elsewhere else (-5000.0, 5000.0, -15000.0))
    if one_more:
        k.add_primitive(solr.ptSphere, (0.0, 0.0, 0.0), size=(100.0, 0, 0), material=m["walls"][0])


def _mix(k, m, key):
    d = key / 3.0   # how far the key frame is from key 0
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
    morph_cases._lamp(k, m, (6000.0, 7000.0, -9000.0))


def _frame(k, m, name, key, flaw=None):
    """the model with key frame `key`'s parameters into the current frame; flaw: one_more / swap_type (sticks only)"""
    if _kind(name) == "mesh":
        _mesh(k, m, key, other_uv=(name == "other_uv" and key == 3))
    elif name == "mix":
        _mix(k, m, key)
    else:
        _sticks(k, m, key, lamp_elsewhere=(name == "lamp_moves" and key == 2), one_more=(flaw == "one_more"),
                swap_type=(flaw == "swap_type"))


def build(k, name, frames=KEY_FRAMES, flaw=None, flawed="stage"):
    """the scene `name` in kernel k: key k in frame frames[k], the stage - key 0's parameters again - in the frame behind the
    last of them, current and flattened.  flaw: one_more (a primitive more) or swap_type (one primitive of another type)
    in the frame `flawed` - a key's number 0 ... 3 or "stage" -, of the sticks only"""
    assert name in NAMES and len(frames) == NB_KEYS
    k.initialize(width=WIDTH, height=HEIGHT, nbRayIterations=3 if name == "mix" else 2)
    m = morph_cases._materials(k, _kind(name))
    stage = max(frames) + 1
    k.set_nb_frames(stage + 1)
    for key, frame in enumerate(frames):
        k.set_frame(frame)
        _frame(k, m, name, key, flaw if flawed == key else None)
        k.compact_boxes(True)
    k.set_frame(stage)
    _frame(k, m, name, 0, flaw if flawed == "stage" else None)
    k.compact_boxes(True)
    if _kind(name) == "mesh":
        k.set_camera((0.0, 4000.0, -15000.0))
    elif name == "mix":
        k.set_camera((200.0, 300.0, -14000.0), look_at=(0.0, 0.0, 0.0), angles=(0.05, -0.1, 0.02))
    else:
        k.set_camera((0.0, 0.0, -14000.0))
    return k


def key_frames(k, frames=KEY_FRAMES):
    """the flattened primitives of every key frame of kernel k by rank in id order (the stage is current again afterwards,
    flattened anew)"""
    keys = []
    for frame in frames:
        k.set_frame(frame)
        k.compact_boxes(False)
        p = k.flat_scene().primitives
        keys.append(p[np.argsort(p["index"], kind="stable")])
    k.set_frame(max(frames) + 1)
    k.compact_boxes(False)
    return keys
