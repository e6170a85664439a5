"""Frame time of a model that is pushed along and of a lamp that is dragged: translatePrimitives, rotatePrimitives +
translatePrimitives (apps/scenes/Scene.cpp:1546-1548) and a lamp's setPrimitiveCenter (apps/solrViewer.cpp:1058-1069), each
followed by compactBoxes(false) + render per displayed frame,
 - by the host route: the move and the flatten on the host, a full upload (SOLR_HIP_DEBUG_TIMING=1 shows its phases), and
 - by the device route: solr_hip_translate_primitives / solr_hip_rotate_primitives / solr_hip_move_lamp on the resident scene,
next to a plain device rotation for scale.  One run, one box.
usage: python tools/moved_frame.py [--n 224] [--frames 200] [--host-frames 3] [--out FILE]"""
import argparse
import importlib
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
solr = importlib.import_module("sol-r_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=224, help="2 n n triangles (224: 100 352)")
ap.add_argument("--frames", type=int, default=200, help="displayed frames of a device route")
ap.add_argument("--host-frames", type=int, default=3, help="displayed frames of a host route")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--out", default=None)
a = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


hip = solr.hip_lib()
k = solr.Kernel(engine="hip", deterministic_seed=1)
solr.scenes.height_field(k, n=a.n, width=a.width, height=a.height)
lamp = k.L.SolR_GetLight(0)
assert lamp >= 0
k.render()
say("height field, %d triangles, %d x %d, one lamp" % (2 * a.n * a.n, a.width, a.height))

TURN = ((0.0, 0.0, 0.0), (0.0, 0.02, 0.0))


def push(f):
    """back and forth: the model stays in the picture"""
    return (40.0 if (f // 25) % 2 == 0 else -40.0, 0.0, 25.0 if (f // 50) % 2 == 0 else -25.0)


def drag(f):
    turn = 2.0 * math.pi * f / 100.0
    return (8000.0 + 1500.0 * math.cos(turn), 8000.0 + 1500.0 * math.sin(turn), -8000.0)


def rotate(f):
    k.rotate_primitives(*TURN)


def translate(f):
    k.translate_primitives(push(f))


def rotate_translate(f):
    k.rotate_primitives(*TURN)
    k.translate_primitives(push(f))


def move_lamp(f):
    k.set_primitive_center(lamp, drag(f))


def counters():
    return hip.solr_hip_device_rotations(), hip.solr_hip_device_translations(), hip.solr_hip_device_lamp_moves()


def host_route(move):
    """a touch of the scene store before every move keeps it off the device"""
    t = []
    served = counters()
    for f in range(a.host_frames):
        k.L.SolR_SetPrimitiveMaterial(0, k.L.SolR_GetPrimitiveMaterial(0))
        t0 = time.perf_counter()
        move(f)
        t1 = time.perf_counter()
        k.render()
        t2 = time.perf_counter()
        t.append((t1 - t0, t2 - t1))
    assert k.pending_moves() == 0 and counters() == served, "a move of the host route ran on the device"
    return 1e3 * sum(x[0] for x in t) / len(t), 1e3 * sum(x[1] for x in t) / len(t)


def device_route(move, per_frame):
    move(0)                              # from the last upload on the scene is resident and untouched
    k.render()
    hip.solr_hip_synchronize()
    before = k.pending_moves()
    t0 = time.perf_counter()
    moving = 0.0
    for f in range(a.frames):
        m0 = time.perf_counter()
        move(f + 1)
        moving += time.perf_counter() - m0
        k.render()
    hip.solr_hip_synchronize()
    dt = time.perf_counter() - t0
    assert k.pending_moves() == before + per_frame * a.frames, "a move of the device route ran on the host"
    return 1e3 * dt / a.frames, 1e3 * moving / a.frames


for name, move, per_frame in (("rotate + render (for scale)", rotate, 1), ("translate + render", translate, 1),
                              ("rotate + translate + render", rotate_translate, 2), ("lamp move + render", move_lamp, 1)):
    moved, rendered = host_route(move)
    say("%-30s host route  : %8.2f ms per displayed frame: move + flatten %.2f ms, upload + render + read-back %.2f ms (%d frames)"
        % (name, moved + rendered, moved, rendered, a.host_frames))
    frame, moving = device_route(move, per_frame)
    say("%-30s device route: %8.3f ms per displayed frame, of which the move %.3f ms (%d frames)"
        % (name, frame, moving, a.frames))
t0 = time.perf_counter()
pending = k.pending_moves()
k.sync_host()
say("host store catches up on %d pending moves in %.1f ms" % (pending, 1e3 * (time.perf_counter() - t0)))
k.render()
t = []
for _ in range(20):
    t0 = time.perf_counter()
    k.render()
    t.append(time.perf_counter() - t0)
say("render alone: %.3f ms per displayed frame (%d frames)" % (1e3 * sum(t) / len(t), len(t)))
k.finalize()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        out.write("\n".join(lines) + "\n")
