"""How long a frame of a stream of JPEG frames takes: Cornell at 1920 x 1080, JPEG quality 85, 2x2 chroma.

    python tools/jpeg_stream.py [--root TREE] [--width 1920] [--height 1080] [--frames 200] [--blocks 5] [--label NAME]
                                [--loop N [--depth D] [--optimise]]

Routes, taking turns block by block (a block is --frames frames, the host clock around it, the pipeline drained inside it;
the median block is reported, the fastest and the slowest beside it):
  render_jpeg one at a time              a frame rendered, coded and collected before the next begins
  jpeg_stream at depth 1, 2, 3           render_jpeg_begin / render_jpeg_end with that many tickets outstanding and as
                                         many frames in flight, standard and optimised tables (where the tree has them)
  raw frames, 3 in flight                SolR_RunKernel with SolRx_SetFramesInFlight(3): what a frame costs without any
                                         JPEG - the floor
--root names another checkout of the project (built): the tool then measures that tree; one without jpeg_stream gives
render_jpeg and the raw frames only, which is how the parent commit's figure is taken in the same session.

--loop N: no timing, N frames of jpeg_stream at --depth (with --optimise: optimised tables) after a warm-up - the program
to put behind `rocprofv3 --kernel-trace --memory-copy-trace --stats --`.  SOLR_HIP_JPEG_ZERO_BOUND=1 in the environment
makes the engine zero the whole bound of the stream in front of every emit instead of clearing behind a use.

Needs a GPU: without one there is nothing to measure, and the tool stops."""
import argparse
import importlib
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--loop", type=int, default=0)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--optimise", action="store_true")
    ap.add_argument("--label", default="this tree")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    solr = importlib.import_module("sol-r_amd")
    hip = solr.hip_lib()
    if hip.solr_hip_device_count() < 1:
        sys.exit("jpeg_stream.py: no GPU; nothing measured")
    import numpy as np
    k = solr.Kernel(engine="hip")
    solr.scenes.cornell(k, width=args.width, height=args.height, iterations=3)
    streaming = hasattr(k, "jpeg_stream")
    image = np.zeros((args.height, args.width, 3), np.uint8)

    def stream(frames, depth, optimise):
        k.L.SolRx_SetFramesInFlight(depth)
        size = 0
        for file in k.jpeg_stream(frames, depth=depth, optimise=optimise):
            size = len(file)
        return size

    if args.loop:
        if not streaming:
            sys.exit("jpeg_stream.py: this tree has no jpeg_stream")
        stream(8, args.depth, args.optimise)
        stream(args.loop, args.depth, args.optimise)
        k.finalize()
        return

    def one_at_a_time(frames):
        k.L.SolRx_SetFramesInFlight(1)
        for _ in range(frames):
            k.render_jpeg()

    def raw(frames):
        k.L.SolRx_SetFramesInFlight(3)
        for _ in range(frames):
            k.L.SolR_RunKernel(0.0, image.ctypes.data)
        k.L.SolRx_FlushFrames()

    routes = {"render_jpeg one at a time": one_at_a_time}
    if streaming:
        for depth in (1, 2, 3):
            routes["jpeg_stream depth %d" % depth] = lambda n, d=depth: stream(n, d, False)
            routes["jpeg_stream depth %d optimised" % depth] = lambda n, d=depth: stream(n, d, True)
    routes["raw frames, 3 in flight"] = raw
    want = k.render_jpeg()
    if streaming:
        assert list(k.jpeg_stream(5, depth=3)) == [want] * 5, "jpeg_stream's files are not render_jpeg's"
    times = {name: [] for name in routes}
    for _ in range(args.blocks):
        for name, call in routes.items():
            call(8)
            hip.solr_hip_synchronize()
            t0 = time.perf_counter()
            call(args.frames)
            times[name].append((time.perf_counter() - t0) / args.frames)
    k.L.SolRx_SetFramesInFlight(1)
    k.check(0, "jpeg_stream")
    k.finalize()
    print("%s: cornell %d x %d, quality 85, 2x2, file %d bytes, %d blocks of %d frames" % (
        args.label, args.width, args.height, len(want), args.blocks, args.frames))
    for name, t in times.items():
        print("  %-34s %.3f ms per frame median (%.3f ... %.3f)" % (name, 1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t)))
    if not streaming:
        print("  (no jpeg_stream in this tree)")


if __name__ == "__main__":
    main()
