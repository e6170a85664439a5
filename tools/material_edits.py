"""Frame time of a host that edits one material every frame, on the 100 k-triangle mesh at 1080p, per displayed frame, with
Kernel.set_material_edits off - the table uploaded (h2d_materials: every primitive retagged on the host, the whole arena laid
out and uploaded again) - and on - the edit followed on the resident scene (solr_hip_edit_materials, k_retagMaterials):
 - scenes.material_pulse: a colour along a sine, transparency 0 <-> 0.5 every other frame (the tags and the colour keys of the
   primitives that have the material change; a frame with the material transparent costs more to render on both sides),
 - a reflection-only edit (two records copied, no kernel),
 - the pulse again with 1 000 materials more in the table (the comparison of the table is the part that grows).
Both sides in one process on one box, the same frames in the same order; per side some warm-up frames, then the median and
the quartiles over the timed frames, each frame timed from the edit to the image on the host.
usage: python tools/material_edits.py [--n 224] [--frames 60] [--off-frames 12] [--warmup 4] [--out FILE]"""
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
ap.add_argument("--frames", type=int, default=60, help="timed frames with the switch on")
ap.add_argument("--off-frames", type=int, default=12, help="timed frames with the switch off")
ap.add_argument("--warmup", type=int, default=4)
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
material = int(np.bincount(flat.primitives["materialId"][flat.primitives["type"] == solr.ptTriangle]).argmax())
share = int((flat.primitives["materialId"] == material).sum())
for _ in range(4):      # the scene resident, its order-free lists built and in the arena
    k.render()
say("height field, %d primitives, %d x %d, %d materials; material %d is edited, %d primitives have it"
    % (len(flat.primitives), a.width, a.height, len(flat.materials), material, share))


def pulse(f):
    solr.scenes.material_pulse(k, material, float(f), specValue=0.6, specPower=80.0)


def reflection(f):
    k.set_material(material, 0.7, 0.6, 0.3, reflection=0.05 + 0.01 * (f % 7), specValue=0.6, specPower=80.0)


def timed(edit, on, frames):
    """ms per displayed frame: (median, first quartile, third quartile), the share of it that is the edit's own call, and how
    many of the frames the engine followed in place / launched the kernel for"""
    k.set_material_edits(on)
    for f in range(a.warmup):
        edit(f)
        k.render()
    hip.solr_hip_synchronize()
    served, retagged, uploads = hip.solr_hip_device_material_edits(), hip.solr_hip_device_material_retags(), k.scene_uploads()
    whole, setting = [], []
    for f in range(a.warmup, a.warmup + frames):
        t0 = time.perf_counter()
        edit(f)
        t1 = time.perf_counter()
        k.render()
        whole.append(time.perf_counter() - t0)
        setting.append(t1 - t0)
    k.check(0, "the timed frames")
    assert k.scene_uploads() == uploads
    served, retagged = hip.solr_hip_device_material_edits() - served, hip.solr_hip_device_material_retags() - retagged
    assert served == (frames if on else 0), "%d of %d frames were followed in place" % (served, frames)
    q = np.percentile(1e3 * np.array(whole), [50, 25, 75])
    return q, 1e3 * float(np.median(setting)), served, retagged


def compare(name, edit):
    off, _, _, _ = timed(edit, False, a.off_frames)
    say("%-28s switch off: %8.2f ms per displayed frame (quartiles %.2f .. %.2f, %d frames, %d warm-up)"
        % (name, off[0], off[1], off[2], a.off_frames, a.warmup))
    on, setting, served, retagged = timed(edit, True, a.frames)
    say("%-28s switch on : %8.3f ms per displayed frame (quartiles %.3f .. %.3f, %d frames, %d warm-up); SolR_SetMaterial itself "
        "%.3f ms; %d edits followed in place, %d launched k_retagMaterials; %.1f x" %
        (name, on[0], on[1], on[2], a.frames, a.warmup, setting, served, retagged, off[0] / on[0]))


compare("material_pulse + render", pulse)
compare("reflection only + render", reflection)
for _ in range(1000):
    k.add_material(0.5, 0.5, 0.5)
k.render()
say("1 000 materials more: %d in the table" % len(k.flat_scene().materials))
k.render()
compare("pulse, long table + render", pulse)
t = []
k.set_material_edits(False)
for _ in range(20):
    t0 = time.perf_counter()
    k.render()
    t.append(time.perf_counter() - t0)
say("render alone: %.3f ms per displayed frame (median of %d frames, the material as the last edit left it)" % (1e3 * float(np.median(t)), len(t)))
k.finalize()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        out.write("\n".join(lines) + "\n")
