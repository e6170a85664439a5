"""How long SolR_LoadTextureFromFile takes for a JPEG texture on the host-only engine (pixel stage in a CPU loop) and on
the HIP engine (pixel stage in k_jpegPixels, with its copies to and from the device): host clock around the call, which
is synchronous on both engines.  The two engines take turns, block by block, and every block is warmed up first.

    python tools/texture_load.py [--file tests/golden/textures/0100d.jpg] [--tile N] [--seconds 1.0]

--tile N (needs PIL): times an N x N tiling of the file's picture instead (quality 90, the file's own sampling left to
PIL's default 4:2:0), written to a temporary directory - the reference's textures are 512 x 512; a user's may not be.
Needs a GPU: without one the HIP engine would fall back to the CPU loop, and the tool stops instead of timing that."""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def block(solr, engine, path, seconds):
    k = solr.Kernel(engine=engine)
    for _ in range(3):
        assert k.load_texture(0, path), path
    times, spent = [], 0.0
    while spent < seconds or len(times) < 5:
        t0 = time.perf_counter()
        k.load_texture(0, path)
        times.append(time.perf_counter() - t0)
        spent += times[-1]
    pixels = k.flat_scene().textures.copy()
    w, h, d = C.c_int(), C.c_int(), C.c_int()
    k.L.SolR_GetTextureSize(0, C.byref(w), C.byref(h), C.byref(d))
    return times, pixels[-w.value * h.value * d.value:], (w.value, h.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--file", default=os.path.join(ROOT, "tests", "golden", "textures", "0100d.jpg"))
    ap.add_argument("--tile", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=1.0)
    args = ap.parse_args()
    solr = importlib.import_module("sol-r_amd")
    hip = solr.hip_lib()
    if hip.solr_hip_device_count() < 1:
        sys.exit("texture_load.py: no GPU; nothing measured")
    path = args.file
    tmp = None
    if args.tile > 1:
        from PIL import Image
        tmp = tempfile.TemporaryDirectory()
        picture = np.tile(np.asarray(Image.open(args.file).convert("RGB")), (args.tile, args.tile, 1))
        path = os.path.join(tmp.name, "tiled.jpg")
        Image.fromarray(picture).save(path, "JPEG", quality=90)
    results = {"host-only": [], "hip": []}
    pixels = {}
    for _ in range(3):
        for engine in ("host-only", "hip"):
            before = hip.solr_hip_jpeg_blocks()
            times, pixels[engine], size = block(solr, engine, path, args.seconds / 3)
            assert (hip.solr_hip_jpeg_blocks() > before) == (engine == "hip")
            results[engine] += times
    assert np.array_equal(pixels["host-only"], pixels["hip"]), "the two engines decoded different textures"
    line = "%s (%d x %d, %d bytes)" % (os.path.basename(args.file) + (" tiled %d x %d" % (args.tile, args.tile)
                                                                      if args.tile > 1 else ""),
                                       size[0], size[1], os.path.getsize(path))
    for engine, times in results.items():
        line += "; %s %.3f ms median, %.3f ms fastest of %d loads" % (engine, 1e3 * statistics.median(times),
                                                                      1e3 * min(times), len(times))
    print(line + "; identical bytes")


if __name__ == "__main__":
    main()
