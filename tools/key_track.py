"""Frame time of an animation of K key frames of one mesh: the 100 k-triangle height field with K seeds as the key frames
in frames 0 ... K - 1 and one more frame as the stage, played back
 - by the route the reference's animation scene takes: SolRx_SetFrame + SolR_CompactBoxes(false) + render per displayed
   frame (a flatten and a full upload each), and
 - by the device route: play(t) + render on the resident stage (solr_hip_morph_between), the morph + refit share broken out.
Also the hand-over of a key frame: per key through solr_hip_set_morph_track_key (k_packMorphKeys packs it on the device), as
the engine call alone and as the request that names a new key pays it; and, on the same run, of the two keys of
morph_frame through solr_hip_set_morph_keys, which the host re-packs into the resident order first.
usage: python tools/key_track.py [--n 224] [--keys 8] [--frames 200] [--laps 2] [--out FILE]"""
import argparse
import importlib
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
solr = importlib.import_module("sol-r_amd")
S = solr.scenes

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=224, help="2 n n triangles (224: 100 352)")
ap.add_argument("--keys", type=int, default=8, help="key frames")
ap.add_argument("--frames", type=int, default=200, help="displayed frames of the device route")
ap.add_argument("--laps", type=int, default=2, help="times the frame-switch route plays its key frames")
ap.add_argument("--seed", type=int, default=1234, help="of key 0; key k: seed + 1111 k")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--out", default=None)
a = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def field(k, seed, mats, n):
    """solr.scenes.height_field's mesh for that seed, into the current frame; the lamp is solr.scenes.add_light's with one
    material for every frame (a key whose materials are not the stage's is not handed over)"""
    rng = S.LCG(seed)
    phase = [rng.uniform(0.0, 6.28) for _ in range(4)]
    scale = 10000.0

    def point(i, j):
        u, v = ((i / n) * 2.0 - 1.0) * 3.0, ((j / n) * 2.0 - 1.0) * 3.0
        y = 1500.0 * (math.sin(3.0 * u + phase[0]) * math.cos(2.0 * v + phase[1]) + 0.5 * math.sin(7.0 * u + 5.0 * v + phase[2]))
        return (u / 3.0 * scale, y - 3000.0, v / 3.0 * scale)

    def normal(i, j):
        p, q, r, s = point(i - 1.0, j), point(i + 1.0, j), point(i, j - 1.0), point(i, j + 1.0)
        tx = (q[0] - p[0], q[1] - p[1], q[2] - p[2])
        tz = (s[0] - r[0], s[1] - r[1], s[2] - r[2])
        return (tz[1] * tx[2] - tz[2] * tx[1], tz[2] * tx[0] - tz[0] * tx[2], tz[0] * tx[1] - tz[1] * tx[0])

    pts = [[point(i, j) for j in range(n + 1)] for i in range(n + 1)]
    nrm = [[normal(i, j) for j in range(n + 1)] for i in range(n + 1)]
    for i in range(n):
        for j in range(n):
            m = mats[((i // 28) + (j // 28)) % (len(mats) - 1)]
            p, q, r, s = pts[i][j], pts[i + 1][j], pts[i + 1][j + 1], pts[i][j + 1]
            np_, nq, nr, ns = nrm[i][j], nrm[i + 1][j], nrm[i + 1][j + 1], nrm[i][j + 1]
            t = k.add_primitive(solr.ptTriangle, p, q, r, material=m)
            k.set_normals(t, np_, nq, nr)
            t = k.add_primitive(solr.ptTriangle, p, r, s, material=m)
            k.set_normals(t, np_, nr, ns)
    k.add_primitive(solr.ptSphere, (8000.0, 8000.0, -8000.0), size=(10.0, 0, 0), material=mats[-1], movable=0)


def ms(seconds):
    return 1e3 * seconds


hip = solr.hip_lib()
k = solr.Kernel(engine="hip", deterministic_seed=1)
k.initialize(width=a.width, height=a.height, nbRayIterations=2, graphicsLevel=solr.glFull)
rng = S.LCG(a.seed)
mats = [k.add_material(*S._wall_color(rng), reflection=0.3 if m % 4 == 0 else 0.0, specValue=0.6, specPower=80.0)
        for m in range(8)]
mats.append(k.add_material(1.0, 1.0, 1.0, innerIllumination=2.0))
K = a.keys
stage = K
seeds = [a.seed + 1111 * key for key in range(K)]
k.set_nb_frames(K + 1)
for frame, seed in list(enumerate(seeds)) + [(stage, seeds[0])]:
    k.set_frame(frame)
    field(k, seed, mats, a.n)
    k.compact_boxes(True)
    print("frame %d built" % frame, flush=True)
k.set_camera((0.0, 4000.0, -15000.0))
say("height field, %d triangles, %d x %d, %d key frames (seeds %d ...), a stage built like key 0"
    % (2 * a.n * a.n, a.width, a.height, K, a.seed))

# the route the reference's animation scene takes: every displayed frame is a key, switched to, flattened and uploaded
k.set_frame(0)
k.compact_boxes(False)
k.render()
t = []
for _ in range(a.laps):
    for frame in range(K):
        t0 = time.perf_counter()
        k.set_frame(frame)
        k.compact_boxes(False)
        t1 = time.perf_counter()
        k.render()
        t2 = time.perf_counter()
        t.append((t1 - t0, t2 - t1))
say("frame switch route: %.2f ms per displayed frame: set frame + flatten %.2f ms, upload + render + read-back %.2f ms (%d frames)"
    % (ms(sum(x[0] + x[1] for x in t)) / len(t), ms(sum(x[0] for x in t)) / len(t), ms(sum(x[1] for x in t)) / len(t), len(t)))

# the key frames as the engine takes them, for the calls timed on their own below: records in id order, ranks of the stage
records = []
for frame in range(K):
    k.set_frame(frame)
    k.compact_boxes(False)
    p = k.flat_scene().primitives
    records.append(np.ascontiguousarray(p[np.argsort(p["index"], kind="stable")]))

# the device route: the stage stays resident and is blended anew for every displayed frame
k.set_frame(stage)
k.compact_boxes(False)
k.render()
flat = k.flat_scene().primitives
rank_of = np.ascontiguousarray(np.searchsorted(np.sort(flat["index"]), flat["index"]), np.int32)
n = len(flat)
view_distance = k.info["viewDistance"]
hip.solr_hip_synchronize()
alone = []
for key in range(K):
    t0 = time.perf_counter()
    assert hip.solr_hip_set_morph_track_key(key, records[key].ctypes.data, rank_of.ctypes.data, n) == 1
    alone.append(time.perf_counter() - t0)
say("solr_hip_set_morph_track_key alone (two copies up, k_packMorphKeys, %d primitives): first key %.2f ms, the others %.2f ms "
    "each (%d keys)" % (n, ms(alone[0]), ms(sum(alone[1:])) / max(1, K - 1), K - 1))
t0 = time.perf_counter()
re_packed = [np.ascontiguousarray(records[key][rank_of]) for key in (0, K - 1)]
t1 = time.perf_counter()
assert hip.solr_hip_set_morph_keys(re_packed[0].ctypes.data, re_packed[1].ctypes.data, n) == 1
t2 = time.perf_counter()
say("solr_hip_set_morph_keys alone, two keys: %.2f ms, after %.2f ms of re-packing both into the resident order with numpy"
    % (ms(t2 - t1), ms(t1 - t0)))
# (keys handed to the engine directly are unknown to the scene store: an upload drops them, the requests below hand their own)
k.L.SolR_SetPrimitiveMaterial(0, k.L.SolR_GetPrimitiveMaterial(0))
k.compact_boxes(False)
k.render()
assert hip.solr_hip_morph_track_keys() == 0
hip.solr_hip_synchronize()

served = hip.solr_hip_device_track_morphs()
span = float(K - 1)
handing, blending, morph, dt = [], [], 0.0, 0.0
for f in range(a.frames):
    time_in_keys = span * (0.5 - 0.5 * math.cos(2.0 * math.pi * f / a.frames))     # forwards, then backwards
    held = hip.solr_hip_morph_track_keys()
    t0 = time.perf_counter()
    assert k.play(time_in_keys) == 0
    t1 = time.perf_counter()
    k.render()
    t2 = time.perf_counter()
    new = hip.solr_hip_morph_track_keys() - held
    if new:
        handing.append((t1 - t0, new))
    else:
        blending.append(t1 - t0)
        morph += t1 - t0
        dt += t2 - t0
hip.solr_hip_synchronize()
assert hip.solr_hip_device_track_morphs() == served + a.frames and k.pending_morph(), "a request took the host route"
assert hip.solr_hip_morph_track_keys() == K
steady = sum(blending) / len(blending)
say("device route      : %.3f ms per displayed frame, of which morph + refit %.3f ms (%d frames that hand no key over)"
    % (ms(dt) / len(blending), ms(morph) / len(blending), len(blending)))
say("hand-over per key : %.2f ms beyond such a request (%d keys in %d requests; the store's records, the ranks once per upload, "
    "k_packMorphKeys)" % (ms(sum(x[0] for x in handing) - steady * len(handing)) / sum(x[1] for x in handing),
                          sum(x[1] for x in handing), len(handing)))
t0 = time.perf_counter()
k.sync_host()
say("host store catches up on the pending morph in %.1f ms" % ms(time.perf_counter() - t0))

# the two keys of morph_frame on the same scene: one more frame behind the stage, a copy of the last key
k.set_nb_frames(K + 2)
k.set_frame(K + 1)
field(k, seeds[-1], mats, a.n)
k.compact_boxes(True)
k.set_frame(stage)
k.compact_boxes(False)
k.render()
hip.solr_hip_synchronize()
two_key = hip.solr_hip_device_morphs()
t0 = time.perf_counter()
assert k.morph_frame(0.5) == 0 and k.pending_morph(), "the morph took the host route"
first = time.perf_counter() - t0
k.render()
again = []
for f in range(20):
    t0 = time.perf_counter()
    k.morph_frame(0.5 + 0.02 * f)
    again.append(time.perf_counter() - t0)
    k.render()
assert hip.solr_hip_device_morphs() == two_key + 21
say("morph_frame       : the first request after the upload %.2f ms, the later ones %.3f ms: %.2f ms for handing two keys over "
    "through solr_hip_set_morph_keys, the host's re-pack into the resident order included"
    % (ms(first), ms(sum(again)) / len(again), ms(first - sum(again) / len(again))))
k.finalize()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        out.write("\n".join(lines) + "\n")
