"""How long the iso-surface of the metaballs scene takes at the reference's size (grid 50, 50 balls on the scene's
trajectories) on the host-only engine (csrc/iso_surface.h in CPU loops) and on the device (solr_hip_metaballs, with its
copies to and from the device), and how long the HIP engine takes from add_metaballs to the first frame of the scene.
Host clock around calls that are synchronous on both engines; the two engines take turns, block by block, and every block
is warmed up first.  For information: no bar rests on it.

    python tools/iso_surface_time.py [--grid 50] [--balls 50] [--seconds 1.0] [--output profiles/r10/iso_surface.txt]

    extraction     balls to triangles in a buffer the surface fits in: SolRx_IsoField + SolRx_IsoSurface on the host-only
                   engine, one solr_hip_metaballs on the device
    add_metaballs  Kernel.add_metaballs after reset_frame on either engine: the extraction and the append to the scene
    first frame    HIP engine: reset_frame, add_metaballs, the box and the lamp, compact_boxes(True), one 512 x 512 frame
Needs a GPU: without one the HIP engine would fall back to the CPU loops, and the tool stops instead of timing that."""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(call, seconds):
    for _ in range(2):
        call()
    times, spent = [], 0.0
    while spent < seconds or len(times) < 5:
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
        spent += times[-1]
    return times


def block(solr, engine, grid, balls, seconds):
    """(extraction times, add_metaballs times, first-frame times or [], the triangles)"""
    hip = solr.hip_lib()
    k = solr.Kernel(engine=engine, deterministic_seed=1)
    solr.scenes.metaballs_begin(k, width=512, height=512)
    g = solr.iso_grid(grid, (150.0,) * 3, 1.0, (0.0, 0.0, -2500.0), (40.0,) * 3, 40.0)
    field = np.zeros(((grid + 1) ** 3, 4), np.float32)
    if engine == "hip":
        count = hip.solr_hip_metaballs(C.byref(g), balls.ctypes.data, len(balls), None, 0)
    else:
        assert k.L.SolRx_IsoField(C.byref(g), balls.ctypes.data, len(balls), field.ctypes.data) == 0
        count = k.L.SolRx_IsoSurface(C.byref(g), field.ctypes.data, None, 0)
    assert count > 0
    triangles = np.zeros(count, solr.ISO_TRIANGLE_DTYPE)

    def extraction():
        if engine == "hip":
            assert hip.solr_hip_metaballs(C.byref(g), balls.ctypes.data, len(balls), triangles.ctypes.data, count) == count
        else:
            assert k.L.SolRx_IsoField(C.byref(g), balls.ctypes.data, len(balls), field.ctypes.data) == 0
            assert k.L.SolRx_IsoSurface(C.byref(g), field.ctypes.data, triangles.ctypes.data, count) == count

    def add():
        k.reset_frame()
        assert k.add_metaballs(balls, grid_size=grid, material=k.metaballs_materials["surface"]) == count

    def first_frame():
        add()
        solr.scenes.metaballs_surroundings(k)
        k.compact_boxes(True)
        k.render()

    out = [timed(extraction, seconds), timed(add, seconds), timed(first_frame, seconds) if engine == "hip" else []]
    k.finalize()
    return out + [triangles.copy()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=50)
    ap.add_argument("--balls", type=int, default=50)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "r10", "iso_surface.txt"))
    args = ap.parse_args()
    solr = importlib.import_module("sol-r_amd")
    hip = solr.hip_lib()
    if hip.solr_hip_device_count() < 1:
        sys.exit("iso_surface_time.py: no GPU; nothing measured")
    balls = solr.scenes.metaball_positions(7.5, count=args.balls)
    engines = ("host-only", "hip")
    times = {e: [[], [], []] for e in engines}
    triangles = {}
    for _ in range(3):
        for engine in engines:
            before = hip.solr_hip_iso_cubes()
            *parts, triangles[engine] = block(solr, engine, args.grid, balls, args.seconds / 3)
            assert (hip.solr_hip_iso_cubes() > before) == (engine == "hip")
            for kept, part in zip(times[engine], parts):
                kept += part
    assert triangles["host-only"].tobytes() == triangles["hip"].tobytes(), "the two engines made different triangles"

    def figure(t):
        return "%.3f ms median (%.3f fastest of %d)" % (1e3 * statistics.median(t), 1e3 * min(t), len(t))

    lines = ["tools/iso_surface_time.py: grid %d, %d balls, %d triangles (%d bytes of records); host clock, both engines in "
             "turn, identical triangles" % (args.grid, args.balls, len(triangles["hip"]), triangles["hip"].nbytes)]
    for engine in engines:
        lines.append("%-9s extraction %s; add_metaballs %s" % (engine + ":", figure(times[engine][0]),
                                                                figure(times[engine][1])))
    lines.append("hip:      reset_frame to the end of the first 512 x 512 frame %s" % figure(times["hip"][2]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
