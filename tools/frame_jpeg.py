"""How long one delivered JPEG frame takes: Cornell (or the 100 k-triangle height field) at 1920 x 1080, JPEG quality 85,
2x2 chroma.

    python tools/frame_jpeg.py [--root TREE] [--scene cornell|height_field] [--width 1920] [--height 1080] [--seconds 2.0]
                               [--loop N [--optimise]] [--label NAME]

Two routes to the same bytes, taking turns block by block, every block warmed up first, host clock around calls that end in
a device synchronise:
  render_jpeg                 the frame is rendered, converted, coded and stuffed on the device, the file's bytes copied
  render() + encode_jpeg      the frame copied to the host as RGB8 and handed back to the encoder, the file written to a
                              tmpfs path - the only route to these bytes before render_jpeg existed (then with 128 bytes
                              per block copied back and one host thread coding them; now the encoder codes on the device too)
  render_jpeg(optimise=True)  the same with Huffman tables counted and built on the device for the frame's own symbols (where
                              the tree has the option): the file's size is printed beside the one-pass file's
and render() alone, for what a frame costs without any JPEG.  --root names another checkout of the project (built): the
tool then measures that tree - one without render_jpeg gives the host route only, which is how the parent commit's figure
in profiles/r24/frame_jpeg.txt was taken, in the same session on the same machine.

--loop N: no timing, N calls of render_jpeg (with --optimise: of render_jpeg(optimise=True)) after a warm-up - the program to put behind `rocprofv3 --kernel-trace
--memory-copy-trace --stats --` for the split by kernel and the copy of the bytes.

Needs a GPU: without one there is nothing to measure, and the tool stops."""
import argparse
import importlib
import inspect
import os
import statistics
import sys
import tempfile
import time


def timed(call, seconds):
    for _ in range(3):
        call()
    times, spent = [], 0.0
    while spent < seconds or len(times) < 5:
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
        spent += times[-1]
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--loop", type=int, default=0)
    ap.add_argument("--optimise", action="store_true")
    ap.add_argument("--scene", default="cornell", choices=("cornell", "height_field"))
    ap.add_argument("--label", default="this tree")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    solr = importlib.import_module("sol-r_amd")
    hip = solr.hip_lib()
    if hip.solr_hip_device_count() < 1:
        sys.exit("frame_jpeg.py: no GPU; nothing measured")
    k = solr.Kernel(engine="hip")
    if args.scene == "cornell":
        solr.scenes.cornell(k, width=args.width, height=args.height, iterations=3)
    else:
        solr.scenes.height_field(k, width=args.width, height=args.height)
    device_route = hasattr(k, "render_jpeg")
    optimised_route = device_route and "optimise" in inspect.signature(k.render_jpeg).parameters
    if args.loop:
        for _ in range(3 + args.loop):
            k.render_jpeg(optimise=True) if args.optimise else k.render_jpeg()
        k.finalize()
        return
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp:
        path = os.path.join(tmp, "frame.jpg")

        def host_route():
            k.encode_jpeg(path, k.render(), turned=True)

        routes = {"render() alone": k.render, "render() + encode_jpeg": host_route}
        if device_route:
            routes["render_jpeg"] = k.render_jpeg
        if optimised_route:
            routes["render_jpeg(optimise=True)"] = lambda: k.render_jpeg(optimise=True)
        times = {name: [] for name in routes}
        for _ in range(4):
            for name, call in routes.items():
                times[name] += timed(call, args.seconds / 4)
        host_route()
        want = open(path, "rb").read()
        if device_route:
            coded = hip.solr_hip_jpeg_coded_blocks()
            assert k.render_jpeg() == want, "the two routes gave different files"
            assert hip.solr_hip_jpeg_coded_blocks() > coded, "render_jpeg did not code the frame on the device"
        optimised = k.render_jpeg(optimise=True) if optimised_route else None
    k.check(0, "frame_jpeg")
    k.finalize()
    line = "%s: %s %d x %d, quality 85, 2x2, file %d bytes" % (args.label, args.scene, args.width, args.height, len(want))
    if optimised is not None:
        line += ", optimised %d bytes (%.3f of it)" % (len(optimised), len(optimised) / len(want))
    for name, t in times.items():
        line += "; %s %.3f ms median (%.3f fastest of %d)" % (name, 1e3 * statistics.median(t), 1e3 * min(t), len(t))
    print(line + ("; identical bytes on both routes" if device_route else "; no render_jpeg in this tree"))


if __name__ == "__main__":
    main()
