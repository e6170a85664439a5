"""Frame time of a deforming scene: the 100 k-triangle height field with two seeds as the key frames, played back
 - by the route the reference offers: the frames GPUKernel::morphPrimitives made, SolRx_SetFrame + SolR_CompactBoxes(false)
   + render per displayed frame (a flatten and a full upload each), and
 - by the device route: morph_frame(weight) + render on the resident scene (solr_hip_morph_primitives), the morph + refit
   share broken out.
usage: python tools/morphed_frame.py [--n 224] [--nb-frames 6] [--frames 200] [--laps 3] [--out FILE]"""
import argparse
import importlib
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
solr = importlib.import_module("sol-r_amd")
S = solr.scenes

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=224, help="2 n n triangles (224: 100 352)")
ap.add_argument("--nb-frames", type=int, default=6, help="key frames included")
ap.add_argument("--frames", type=int, default=200, help="displayed frames of the device route")
ap.add_argument("--laps", type=int, default=3, help="times the parent route plays its in-between frames")
ap.add_argument("--seeds", type=int, nargs=2, default=(1234, 4321))
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--out", default=None)
a = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def field(k, seed, mats, n):
    """solr.scenes.height_field's mesh for that seed, into the current frame"""
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
            m = mats[((i // 28) + (j // 28)) % len(mats)]
            p, q, r, s = pts[i][j], pts[i + 1][j], pts[i + 1][j + 1], pts[i][j + 1]
            np_, nq, nr, ns = nrm[i][j], nrm[i + 1][j], nrm[i + 1][j + 1], nrm[i][j + 1]
            t = k.add_primitive(solr.ptTriangle, p, q, r, material=m)
            k.set_normals(t, np_, nq, nr)
            t = k.add_primitive(solr.ptTriangle, p, r, s, material=m)
            k.set_normals(t, np_, nr, ns)
    S.add_light(k)


hip = solr.hip_lib()
k = solr.Kernel(engine="hip", deterministic_seed=1)
k.initialize(width=a.width, height=a.height, nbRayIterations=2, graphicsLevel=solr.glFull)
rng = S.LCG(a.seeds[0])
mats = [k.add_material(*S._wall_color(rng), reflection=0.3 if m % 4 == 0 else 0.0, specValue=0.6, specPower=80.0)
        for m in range(8)]
k.set_nb_frames(a.nb_frames)
for frame, seed in ((0, a.seeds[0]), (a.nb_frames - 1, a.seeds[1])):
    k.set_frame(frame)
    field(k, seed, mats, a.n)
    k.compact_boxes(True)
t0 = time.perf_counter()
k.morph_primitives()
made = time.perf_counter() - t0
k.set_camera((0.0, 4000.0, -15000.0))
between = list(range(1, a.nb_frames - 1))
say("height field, %d triangles, %d x %d, key frames: seeds %d and %d, %d frames between them"
    % (2 * a.n * a.n, a.width, a.height, a.seeds[0], a.seeds[1], len(between)))
say("morphPrimitives made the %d frames between the keys (a tree each) in %.1f ms" % (len(between), 1e3 * made))

# the route the reference offers: switch to a frame morphPrimitives made, flatten it, upload it with the next frame
k.set_frame(between[0])
k.compact_boxes(False)
k.render()
t = []
for _ in range(a.laps):
    for frame in between:
        t0 = time.perf_counter()
        k.set_frame(frame)
        k.compact_boxes(False)
        t1 = time.perf_counter()
        k.render()
        t2 = time.perf_counter()
        t.append((t1 - t0, t2 - t1))
assert not k.pending_morph()
say("frame switch route: %.2f ms per displayed frame: set frame + flatten %.2f ms, upload + render + read-back %.2f ms (%d frames)"
    % (1e3 * sum(x[0] + x[1] for x in t) / len(t), 1e3 * sum(x[0] for x in t) / len(t), 1e3 * sum(x[1] for x in t) / len(t), len(t)))

# the device route: one frame between the keys stays resident and is blended anew for every displayed frame
k.set_frame(between[len(between) // 2])
k.compact_boxes(False)
k.render()
t0 = time.perf_counter()
assert k.morph_frame(0.5) == 0 and k.pending_morph(), "the morph took the host route"
first = time.perf_counter() - t0
k.render()
hip.solr_hip_synchronize()
served = hip.solr_hip_device_morphs()
t0 = time.perf_counter()
morph = 0.0
for f in range(a.frames):
    weight = 0.5 + 0.5 * math.sin(2.0 * math.pi * f / 100.0)
    m0 = time.perf_counter()
    k.morph_frame(weight)
    morph += time.perf_counter() - m0
    k.render()
hip.solr_hip_synchronize()
dt = time.perf_counter() - t0
assert hip.solr_hip_device_morphs() == served + a.frames and k.pending_morph()
say("device route      : %.3f ms per displayed frame, of which morph + refit %.3f ms (%d frames); the first morph after the "
    "upload, which hands the keys over: %.1f ms" % (1e3 * dt / a.frames, 1e3 * morph / a.frames, a.frames, 1e3 * first))
t0 = time.perf_counter()
k.sync_host()
say("host store catches up on the pending morph in %.1f ms" % (1e3 * (time.perf_counter() - t0)))
k.finalize()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        out.write("\n".join(lines) + "\n")
