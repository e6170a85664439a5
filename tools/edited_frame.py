"""Frame time of a scene that sets some of its primitives anew every frame - the reference's WaterScene::doAnimate: 1152
triangles through setPrimitive + setPrimitiveNormals + setPrimitiveTextureCoordinates, the box updates, compactBoxes(false) -
on the 100 k-triangle mesh, per displayed frame,
 - by the host route: the three setters one record at a time, a translation by -0 for the box updates, compactBoxes(false), a
   full upload with the frame (SOLR_HIP_DEBUG_TIMING=1 shows its phases), and
 - by the device route: the same records through Kernel.set_primitives (solr_hip_set_primitives on the resident scene),
at two batch sizes: 1152 records, and every triangle.  Also the share of the device route that is the batch itself - slots,
upload of the batch, kernel, refit.  One run, one box.
usage: python tools/edited_frame.py [--n 224] [--frames 100] [--host-frames 3] [--out FILE]"""
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
k.render()
say("height field, %d triangles, %d x %d, one lamp" % (len(triangles), a.width, a.height))


def batch_at(f, count):
    """the first `count` triangles, heaving: every vertex up and down with the frame, normals and texture coordinates given"""
    t = triangles[:count]
    batch = np.zeros(count, solr.EDIT_DTYPE)
    batch["index"], batch["materialId"] = t["index"], t["materialId"]
    batch["flags"] = solr.EDIT_NORMALS | solr.EDIT_TEXTURE_COORDINATES
    lift = np.float32(60.0 * np.sin(0.3 * f))
    for field in ("p0", "p1", "p2"):
        batch[field] = t[field]
        batch[field][:, 1] += lift * np.sin(t[field][:, 0] / np.float32(900.0))
    for field in ("n0", "n1", "n2"):
        batch[field] = t[field]
    batch["vt0"], batch["vt1"], batch["vt2"] = (0.0, 0.0), (1.0, 0.0), (1.0, 1.0)
    return batch


def host_route(count):
    """the setters that were there before; their first touch of the scene store keeps the rest off the device"""
    t = []
    k.sync_host()                            # (what a device route before this left pending is not this route's cost)
    served = hip.solr_hip_device_edits()
    set_primitive, set_normals, set_uv = k.L.SolR_SetPrimitive, k.L.SolR_SetPrimitiveNormals, k.L.SolR_SetPrimitiveTextureCoordinates
    for f in range(a.host_frames):
        batch = batch_at(f, count)
        rows = [(int(e["index"]), [float(c) for field in ("p0", "p1", "p2", "size") for c in e[field]], int(e["materialId"]),
                 [float(c) for field in ("n0", "n1", "n2") for c in e[field]],
                 [float(c) for field in ("vt0", "vt1", "vt2") for c in e[field]]) for e in batch]
        t0 = time.perf_counter()
        for index, geometry, material, normals, uv in rows:
            set_primitive(index, *geometry, material)
            set_normals(index, *normals)
            set_uv(index, *uv)
        k.translate_primitives((-0.0, -0.0, -0.0))
        k.compact_boxes(False)
        t1 = time.perf_counter()
        k.render()
        t2 = time.perf_counter()
        t.append((t1 - t0, t2 - t1))
    assert k.pending_moves() == 0 and hip.solr_hip_device_edits() == served, "a batch of the host route ran on the device"
    return 1e3 * sum(x[0] for x in t) / len(t), 1e3 * sum(x[1] for x in t) / len(t)


def device_route(count):
    k.set_primitives(batch_at(0, count))     # from the last upload on the scene is resident and untouched
    k.render()
    hip.solr_hip_synchronize()
    batches = [batch_at(f + 1, count) for f in range(8)]      # (made before the clock starts; eight frames of the heave, cycled)
    k.sync_host()
    before, served = k.pending_moves(), hip.solr_hip_device_edits()
    t0 = time.perf_counter()
    editing = 0.0
    for f in range(a.frames):
        m0 = time.perf_counter()
        k.set_primitives(batches[f % len(batches)])
        editing += time.perf_counter() - m0
        k.render()
    hip.solr_hip_synchronize()
    dt = time.perf_counter() - t0
    # (the store catches up on its own when the journal's batches pass 2^20 records: the pending count starts anew then)
    assert before == 0 and 0 < k.pending_moves() <= a.frames and hip.solr_hip_device_edits() == served + a.frames, \
        "a batch of the device route ran on the host"
    return 1e3 * dt / a.frames, 1e3 * editing / a.frames


for count in (1152, len(triangles)):
    name = "%d edits + render" % count
    edited, rendered = host_route(count)
    say("%-24s host route  : %8.2f ms per displayed frame: setters + box updates + flatten %.2f ms, upload + render + read-back %.2f ms (%d frames)"
        % (name, edited + rendered, edited, rendered, a.host_frames))
    frame, editing = device_route(count)
    say("%-24s device route: %8.3f ms per displayed frame, of which slots + batch upload + kernel + refit %.3f ms (%.0f %%) (%d frames)"
        % (name, frame, editing, 100.0 * editing / frame, a.frames))
t0 = time.perf_counter()
pending = k.pending_moves()
k.sync_host()
say("host store catches up on %d pending batches in %.1f ms" % (pending, 1e3 * (time.perf_counter() - t0)))
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
