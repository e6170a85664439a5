"""How long the pixel stage of the screenshot's JPEG encoder takes for one picture on the host-only engine (csrc/jpeg_encode.h
in a CPU loop) and on the HIP engine (k_jpegCoefficients, with its copies to and from the device): host clock around
SolRx_JpegCoefficients, which is synchronous on both engines, and around the whole encode_jpeg (pixel stage, Huffman coder,
file).  The two engines take turns, block by block, and every block is warmed up first.  For information: no bar rests on it.

    python tools/screenshot_encode.py [--width 1920] [--height 1080] [--seconds 1.0]

The picture is a smooth ramp with seeded noise of +-16 on it, JPEG quality 85, 2x2 chroma, read turned as a screenshot is.
Needs a GPU: without one the HIP engine would fall back to the CPU loop, and the tool stops instead of timing that."""
import argparse
import importlib
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def block(solr, engine, pixels, seconds, path):
    k = solr.Kernel(engine=engine)
    height, width, _ = pixels.shape
    blocks = np.zeros((-(-width // 16) * -(-height // 16) * 6, 64), np.int16)

    def stage():
        assert k.L.SolRx_JpegCoefficients(pixels.ctypes.data, width, height, 85, 2, 2, 1, 0, blocks.ctypes.data,
                                          len(blocks)) == 0

    def whole():
        k.encode_jpeg(path, pixels, turned=True)

    out = []
    for call in (stage, whole):
        for _ in range(2):
            call()
        times, spent = [], 0.0
        while spent < seconds or len(times) < 5:
            t0 = time.perf_counter()
            call()
            times.append(time.perf_counter() - t0)
            spent += times[-1]
        out.append(times)
    return out[0], out[1], blocks.copy(), open(path, "rb").read()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--seconds", type=float, default=1.0)
    args = ap.parse_args()
    solr = importlib.import_module("sol-r_amd")
    hip = solr.hip_lib()
    if hip.solr_hip_device_count() < 1:
        sys.exit("screenshot_encode.py: no GPU; nothing measured")
    yy, xx = np.indices((args.height, args.width))
    rng = np.random.RandomState(9)
    ramp = np.stack([255 * xx // max(args.width - 1, 1), 255 * yy // max(args.height - 1, 1),
                     255 * (xx + yy) // max(args.width + args.height - 2, 1)], axis=-1)
    pixels = np.ascontiguousarray(np.clip(ramp + rng.randint(-16, 17, ramp.shape), 0, 255).astype(np.uint8))
    stage, whole, blocks, files = {"host-only": [], "hip": []}, {"host-only": [], "hip": []}, {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(3):
            for engine in ("host-only", "hip"):
                before = hip.solr_hip_jpeg_encoded_blocks()
                s, w, blocks[engine], files[engine] = block(solr, engine, pixels, args.seconds / 3,
                                                            os.path.join(tmp, "out.jpg"))
                assert (hip.solr_hip_jpeg_encoded_blocks() > before) == (engine == "hip")
                stage[engine] += s
                whole[engine] += w
    assert np.array_equal(blocks["host-only"], blocks["hip"]) and files["host-only"] == files["hip"], \
        "the two engines encoded different files"
    line = "%d x %d, quality 85, 2x2, %d blocks, file %d bytes" % (args.width, args.height, len(blocks["hip"]),
                                                                   len(files["hip"]))
    for engine in ("host-only", "hip"):
        line += "; %s: pixel stage %.3f ms median (%.3f fastest of %d), whole encode %.3f ms median (%.3f fastest of %d)" % (
            engine, 1e3 * statistics.median(stage[engine]), 1e3 * min(stage[engine]), len(stage[engine]),
            1e3 * statistics.median(whole[engine]), 1e3 * min(whole[engine]), len(whole[engine]))
    print(line + "; identical blocks and bytes")


if __name__ == "__main__":
    main()
