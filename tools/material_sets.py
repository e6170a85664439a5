"""Frame time of a scene that gives some of its primitives another material every frame, on the 100 k-triangle mesh, per
displayed frame,
 - the walk of the reference's SwcScene::doAnimate (scenes.swc_walk): the primitive marked by the frame before gets its
   material back, the next one the light material, the lamp is moved next to it - along 64 made-up samples that sit on
   triangles of the mesh - and
 - a recolour of 1 000 triangles,
each by the host route - SolR_SetPrimitiveMaterial one record at a time (and SolRx_SetPrimitiveCenter for the lamp),
compactBoxes(false), a full upload with the frame: what a request cost before set_primitive_materials - and by the device
route: Kernel.set_primitive_materials (solr_hip_set_primitive_materials on the resident scene) and the lamp move on the
device.  Also the share of the device route that is the requests themselves.  One run, one box.
usage: python tools/material_sets.py [--n 224] [--frames 100] [--host-frames 3] [--out FILE]"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
solr = importlib.import_module("sol-r_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=224, help="2 n n triangles (224: 100 352)")
ap.add_argument("--frames", type=int, default=100, help="displayed frames of a device route")
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
flat = k.flat_scene()
triangles = flat.primitives[flat.primitives["type"] == solr.ptTriangle]
triangles = triangles[np.argsort(triangles["index"])]
lamp = k.L.SolR_GetLight(0)
light = k.get_primitive_material(lamp)
k.render()
say("height field, %d triangles, %d x %d, one lamp" % (len(triangles), a.width, a.height))

# 64 samples on triangles spread over the mesh, 400 above them: the lamp next to a sample stays inside its cell
samples = np.zeros(64, solr.SWC_SAMPLE_DTYPE)
on = triangles[np.linspace(0, len(triangles) - 1, len(samples)).astype(int)]
samples["id"] = np.arange(len(samples))
samples["primitiveId"] = on["index"]
samples["x"], samples["y"], samples["z"] = on["p0"][:, 0], on["p0"][:, 1] + np.float32(400.0), on["p0"][:, 2]
RECOLOURED = 1000
recoloured = triangles[np.linspace(0, len(triangles) - 1, RECOLOURED).astype(int)]
recolour_indices = recoloured["index"].astype(np.int32)


def recolour_materials(f):
    """the materials the mesh has (eight plain ones), every triangle one further with every frame"""
    return ((recoloured["materialId"] + 1 + f) % 8).astype(np.int32)


def walk_by_the_old_calls(step, marked):
    """SwcScene::doAnimate with the calls that were there before; returns what is marked now"""
    s = samples[step % len(samples)]
    primitive = int(s["primitiveId"])
    if marked is not None:
        k.L.SolR_SetPrimitiveMaterial(*marked)
    marked = (primitive, k.L.SolR_GetPrimitiveMaterial(primitive))
    k.L.SolR_SetPrimitiveMaterial(primitive, light)
    k.set_primitive_center(lamp, (float(s["x"]), float(s["y"]), float(np.float32(s["z"] - np.float32(50.0)))))
    return marked


def host_route(request):
    """request(f): frame f's request by the setters; their first touch of the scene store keeps the rest off the device"""
    t = []
    k.sync_host()                            # (what a device route before this left pending is not this route's cost)
    served = hip.solr_hip_device_material_sets()
    for f in range(a.host_frames):
        t0 = time.perf_counter()
        request(f)
        t1 = time.perf_counter()
        k.render()
        t2 = time.perf_counter()
        t.append((t1 - t0, t2 - t1))
    assert k.pending_moves() == 0 and hip.solr_hip_device_material_sets() == served, "a request of the host route ran on the device"
    return 1e3 * sum(x[0] for x in t) / len(t), 1e3 * sum(x[1] for x in t) / len(t)


def device_route(request, per_frame):
    """request(f): frame f's request through the new call; per_frame: the moves a frame leaves pending"""
    k.render()                               # from this upload on the scene is resident and untouched
    request(0)
    k.render()
    hip.solr_hip_synchronize()
    k.sync_host()
    before, served = k.pending_moves(), hip.solr_hip_device_material_sets()
    t0 = time.perf_counter()
    requesting = 0.0
    for f in range(a.frames):
        m0 = time.perf_counter()
        request(f + 1)
        requesting += time.perf_counter() - m0
        k.render()
    hip.solr_hip_synchronize()
    dt = time.perf_counter() - t0
    assert before == 0 and k.pending_moves() == per_frame * a.frames and hip.solr_hip_device_material_sets() == served + a.frames, \
        "a request of the device route ran on the host"
    return 1e3 * dt / a.frames, 1e3 * requesting / a.frames


old = {"marked": None}


def walk_old(f):
    old["marked"] = walk_by_the_old_calls(f, old["marked"])      # (set_primitive_center flattens: compactBoxes(false), once)


state = {}


def walk_new(f):
    if old["marked"] is not None:            # (what the host route's walk left marked goes back first)
        k.L.SolR_SetPrimitiveMaterial(*old["marked"])
        k.compact_boxes(False)
        old["marked"] = None
        k.render()
    solr.scenes.swc_walk(k, samples, lamp, light, f, state)


def recolour_old(f):
    set_material = k.L.SolR_SetPrimitiveMaterial
    for index, material in zip(recolour_indices.tolist(), recolour_materials(f).tolist()):
        set_material(index, material)
    k.compact_boxes(False)


def recolour_new(f):
    assert k.set_primitive_materials(recolour_indices, recolour_materials(f)) == 0


for name, by_old, by_new, per_frame in (("swc_walk + render", walk_old, walk_new, 2),
                                        ("%d materials + render" % RECOLOURED, recolour_old, recolour_new, 1)):
    requested, rendered = host_route(by_old)
    say("%-24s host route  : %8.2f ms per displayed frame: setters + flatten %.2f ms, upload + render + read-back %.2f ms (%d frames)"
        % (name, requested + rendered, requested, rendered, a.host_frames))
    frame, requesting = device_route(by_new, per_frame)
    say("%-24s device route: %8.3f ms per displayed frame, of which the requests - slots, batch, kernels%s - %.3f ms (%.0f %%) (%d frames)"
        % (name, frame, ", the lamp" if per_frame == 2 else "", requesting, 100.0 * requesting / frame, a.frames))
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
