"""Frame time of an animation of whole meshes - the reference's AnimationScene restated (scenes.animation: one height field
per frame, each with another triangle count and a tree of its own, shown with set_frame + compact_boxes(False): scenes.animation_step) -
per displayed frame,
 - with the frame bank off: a flatten, a walk-order list and a full upload per displayed frame, what a frame switch cost before
   the bank (asserted: one scene upload per displayed frame), and
 - with the frame bank on (Kernel.set_frame_bank): the frames stay on the engine and a switch uploads nothing (asserted),
alternating in one process, with 1 and 3 frames in flight; also the first lap with the bank on (it uploads every frame
once), what a parked frame holds of device memory, and a lap in which every resume follows an h2d_materials (pulled,
retagged and laid out again).  One run, one box.
A sample is the wall clock between two device synchronisations over whole laps, divided by its displayed frames: one lap with
the bank off (about half a second), --on-laps laps with the bank on (a lap takes some 10 ms there: a window of one would
measure the clock and the scheduler).
usage: python tools/frame_bank.py [--frames 8] [--cells 220] [--rounds 5] [--laps 5] [--on-laps 25] [--out FILE]"""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
solr = importlib.import_module("sol-r_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8, help="frames of the animation")
ap.add_argument("--cells", type=int, default=220, help="frame f is a height field of 2 (cells + f)^2 triangles (220: 96 800 ... 103 058)")
ap.add_argument("--rounds", type=int, default=5, help="rounds of bank off, bank on")
ap.add_argument("--laps", type=int, default=5, help="samples per route and round, behind two warm-up laps")
ap.add_argument("--on-laps", type=int, default=25, help="laps in a sample with the bank on")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--bank", type=int, default=8 << 30, help="bytes of device memory the bank may hold")
ap.add_argument("--out", default=None)
a = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


hip = solr.hip_lib()
k = solr.Kernel(engine="hip", deterministic_seed=1)
t0 = time.perf_counter()
solr.scenes.animation(k, frames=a.frames, cells=a.cells, width=a.width, height=a.height)
K = a.frames
say("animation of %d frames, %s primitives, %d x %d (built in %.1f s)"
    % (K, ", ".join(str(c) for c in k.animation["counts"]), a.width, a.height, time.perf_counter() - t0))
materials = np.ascontiguousarray(k.flat_scene().materials)      # (for the lap behind h2d_materials, at the end)
step = [0]


def lap(laps=1):
    """laps x K displayed frames in one timed window; returns (seconds, scene uploads, frame switches served from the bank),
    each per lap"""
    before = (k.scene_uploads(), k.frame_switches())
    hip.solr_hip_synchronize()
    t = time.perf_counter()
    for _ in range(laps * K):
        solr.scenes.animation_step(k, step[0])
        step[0] += 1
        k.render()
    k.L.SolRx_FlushFrames()
    hip.solr_hip_synchronize()
    return (time.perf_counter() - t) / laps, (k.scene_uploads() - before[0]) / laps, (k.frame_switches() - before[1]) / laps


def figures(ms):
    ms = sorted(ms)
    return "median %8.3f ms, min %8.3f, max %8.3f, p10 %8.3f, p90 %8.3f (%d samples)" % (
        statistics.median(ms), ms[0], ms[-1], ms[len(ms) // 10], ms[min(len(ms) - 1, (9 * len(ms)) // 10)], len(ms))


for flights in (1, 3):
    k.L.SolRx_SetFramesInFlight(flights)
    per_frame = {"off": [], "on": []}
    first_lap = []
    for r in range(a.rounds):
        for route in ("off", "on"):
            k.set_frame_bank(a.bank if route == "on" else 0)
            for warm in range(2):
                seconds, uploads, switches = lap()
                if route == "on" and warm == 0:
                    first_lap.append(1e3 * seconds / K)
                    # (the frame the bank-off laps left resident is parked by the first switch and comes back at the end)
                    assert uploads + switches == K and uploads >= K - 1, "the first lap with the bank on uploads the frames once"
            for _ in range(a.laps):
                seconds, uploads, switches = lap(a.on_laps if route == "on" else 1)
                if route == "off":
                    assert (uploads, switches) == (K, 0), "bank off is the route of before: an upload per displayed frame"
                else:
                    assert (uploads, switches) == (0, K), "bank on: no upload, every switch from the bank"
                per_frame[route].append(1e3 * seconds / K)
    say("%d frame(s) in flight, per displayed frame (set_frame + compact_boxes(False) + render; a sample: 1 lap off, %d laps on):"
        % (flights, a.on_laps))
    say("  bank off: " + figures(per_frame["off"]))
    say("  bank on : " + figures(per_frame["on"]))
    say("  bank on, first lap (the frames flattened and uploaded once, all but the one that was resident): " + figures(first_lap))
    off, on = statistics.median(per_frame["off"]), statistics.median(per_frame["on"])
    say("  bank off / bank on: %.1f x%s" % (off / on, "" if on <= off else "  (THE BANK'S FRAME IS SLOWER)"))
k.L.SolRx_SetFramesInFlight(1)

# the bank is on and full: K - 1 frames parked
parked, held = hip.solr_hip_parked_scenes(), hip.solr_hip_parked_bytes()
usage = (C.c_ulonglong * 4)()
hip.solr_hip_memory_usage(usage)
say("parked: %d scenes, %.1f MB, %.1f MB per frame; the resident scene %.1f MB" % (parked, held / 1e6, held / 1e6 / max(parked, 1), usage[0] / 1e6))

# render alone: the resident frame again and again
ms = []
for _ in range(20):
    hip.solr_hip_synchronize()
    t = time.perf_counter()
    k.render()
    ms.append(1e3 * (time.perf_counter() - t))
say("render alone, the resident frame: " + figures(ms))

# h2d_materials behind the host's back (the same table: the host goes on taking the fast path), so that every resume of the
# next lap finds its scene tagged under another table
ms = []
for _ in range(5):
    hip.h2d_materials(0, C.c_void_p(materials.ctypes.data), len(materials))
    seconds, uploads, switches = lap()
    assert (uploads, switches) == (0, K)
    ms.append(1e3 * seconds / K)
say("1 frame in flight, bank on, every resume behind an h2d_materials (pull, retag, lay out again): " + figures(ms))
seconds, uploads, switches = lap()
say("  ... and the lap after: %.3f ms per displayed frame" % (1e3 * seconds / K))
k.check(0, "frame_bank")
k.finalize()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        out.write("\n".join(lines) + "\n")
