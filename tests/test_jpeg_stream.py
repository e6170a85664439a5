"""JPEG frames in flight, the parts that need no device: the ticket rule of SolRx_RenderJpegBegin / SolRx_RenderJpegEnd
(GPUKernel::renderJpegBegin, renderJpegEnd), Kernel.jpeg_stream's order, the plan arithmetic of the resident entropy
pipeline (sol-r_amd/csrc/jpeg_entropy.h, planScan) and that pipeline's loops under the sanitizers
(tests/jpeg_stream_check.cpp).  The device's side is tests/test_jpeg_stream_gpu.py.

The host-only engine renders nothing - SolRx_RenderJpeg fails there, and so does SolRx_RenderJpegBegin - so the protocol is
driven here with frames that come as pixels: SolRx_JpegParkPixels encodes them at once, read as a frame is read, and parks
the file under a ticket exactly as a declined SolRx_RenderJpegBegin parks its frame's (one store, one rule).  The frames
are 40 x 24 and 37 x 21, as the rendered ones of the device's tests are, in both modes, and every file is held byte for byte
to the synchronous encoder's (encode_jpeg, SolRx_EncodeJpeg[Optimised])."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import jpeg_entropy_cases as JC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SENTINEL = 0x5A
SIZES = [(40, 24), (37, 21)]


@pytest.fixture(scope="module")
def host(solr):
    k = solr.Kernel(engine="host-only")
    yield k
    k.finalize()


def frame(width, height, seed):
    """pixels that differ from frame to frame: a gradient and noise"""
    rng = np.random.RandomState(1000 * seed + width)
    y, x = np.mgrid[0:height, 0:width]
    base = np.stack([(x * 6 + seed * 17) % 256, (y * 9 + seed * 5) % 256, (x + y) * 3 % 256], axis=-1)
    return ((base + rng.randint(0, 40, (height, width, 3))) % 256).astype(np.uint8)


def synchronous(k, tmp_path, pixels, optimise, quality=85, sampling=(2, 2)):
    path = str(tmp_path / "synchronous.jpg")
    k.encode_jpeg(path, pixels, quality=quality, sampling=sampling, turned=True, swap_red_blue=False, optimise=optimise)
    return open(path, "rb").read()


def park(k, pixels, optimise, quality=85, sampling=(2, 2)):
    pixels = np.ascontiguousarray(pixels, np.uint8)
    return k.L.SolRx_JpegParkPixels(pixels.ctypes.data, pixels.shape[1], pixels.shape[0], quality, sampling[0], sampling[1], 0,
                                    int(optimise))


def end(k, ticket, capacity=1 << 16):
    """SolRx_RenderJpegEnd into a buffer with a sentinel behind `capacity`: (status, size, the buffer)"""
    out = np.full(capacity + 16, SENTINEL, np.uint8)
    size = C.c_long(77)
    status = k.L.SolRx_RenderJpegEnd(ticket, out.ctypes.data, capacity, C.byref(size))
    assert (out[capacity:] == SENTINEL).all()
    return status, size.value, out


def ticket_error(k):
    text = C.create_string_buffer(512)
    return k.L.SolRx_RenderJpegTicketError(text, 512), text.value.decode()


@pytest.mark.parametrize("optimise", [False, True], ids=["standard", "optimised"])
@pytest.mark.parametrize("width, height", SIZES)
def test_a_ticket_delivers_the_synchronous_file(host, tmp_path, width, height, optimise):
    pixels = frame(width, height, 1)
    want = synchronous(host, tmp_path, pixels, optimise)
    ticket = park(host, pixels, optimise)
    assert ticket >= 0
    assert host.render_jpeg_end(ticket) == want
    assert host.render_jpeg_end(ticket) == want, "a ticket may be collected again"
    assert ticket_error(host) == (0, "")


@pytest.mark.parametrize("optimise", [False, True], ids=["standard", "optimised"])
@pytest.mark.parametrize("width, height", SIZES)
def test_four_tickets_collected_in_reverse_order_and_the_fifth_makes_the_first_stale(solr, host, tmp_path, width, height, optimise):
    frames = [frame(width, height, seed) for seed in range(5)]
    want = [synchronous(host, tmp_path, pixels, optimise) for pixels in frames]
    assert len(set(want)) == 5
    tickets = [park(host, pixels, optimise) for pixels in frames[:4]]
    assert len(set(tickets)) == 4 and min(tickets) >= 0
    for i in (3, 2, 1, 0):
        assert host.render_jpeg_end(tickets[i]) == want[i], "ticket %d" % i
    fifth = park(host, frames[4], optimise)
    assert fifth >= 0 and fifth not in tickets
    status, size, out = end(host, tickets[0])
    assert status == -1 and size == 0 and (out == SENTINEL).all(), "a stale ticket delivered something"
    code, text = ticket_error(host)
    assert code != 0 and "no such ticket" in text
    with pytest.raises(solr.SolrError, match="no such ticket"):
        host.render_jpeg_end(tickets[0])
    for i in (1, 2, 3):
        assert host.render_jpeg_end(tickets[i]) == want[i], "ticket %d after the fifth" % i
    assert host.render_jpeg_end(fifth) == want[4]
    assert ticket_error(host) == (0, "")


@pytest.mark.parametrize("optimise", [False, True], ids=["standard", "optimised"])
def test_a_capacity_too_small_returns_the_size_and_leaves_the_ticket_good(host, tmp_path, optimise):
    pixels = frame(40, 24, 7)
    want = synchronous(host, tmp_path, pixels, optimise)
    ticket = park(host, pixels, optimise)
    status, size, out = end(host, ticket, capacity=100)
    assert status == -1 and size == len(want) and (out == SENTINEL).all()
    assert ticket_error(host) == (0, ""), "a buffer too small is no error"
    status, size, out = end(host, ticket, capacity=len(want) - 1)
    assert status == -1 and size == len(want) and (out == SENTINEL).all()
    status, size, out = end(host, ticket, capacity=len(want))
    assert status == 0 and size == len(want) and out[:size].tobytes() == want
    # Kernel.render_jpeg_end's own retry: one more call, no other ticket handed out in between
    assert host.render_jpeg_end(ticket, room=64) == want


def test_a_ticket_that_was_never_issued_gives_minus_one(host):
    """a ticket is serial * 4 + serial % 4: negative numbers, numbers of no serial, and serials not yet reached"""
    issued = park(host, frame(40, 24, 3), False)
    assert issued % 4 == (issued // 4) % 4
    for ticket in (-1, -5, issued + 1, issued + 4, issued + 16, issued + 16 * 1000, 2 ** 31 - 1):
        status, size, out = end(host, ticket)
        assert status == -1 and size == 0 and (out == SENTINEL).all(), ticket
        code, text = ticket_error(host)
        assert code != 0 and "no such ticket" in text
    # null buffer, negative capacity, null size: refused, the ticket still good
    size = C.c_long(77)
    out = np.full(64, SENTINEL, np.uint8)
    assert host.L.SolRx_RenderJpegEnd(issued, None, 64, C.byref(size)) == -1 and size.value == 0
    assert host.L.SolRx_RenderJpegEnd(issued, out.ctypes.data, -1, C.byref(size)) == -1 and size.value == 0
    assert host.L.SolRx_RenderJpegEnd(issued, out.ctypes.data, 64, None) == -1
    assert (out == SENTINEL).all()
    assert end(host, issued)[0] == 0


def test_bad_quality_or_sampling_issues_no_ticket(solr, host):
    pixels = frame(40, 24, 2)
    good = park(host, pixels, False)
    for quality, h, v in ((0, 2, 2), (101, 2, 2), (85, 1, 2), (85, 3, 1)):
        assert park(host, pixels, False, quality, (h, v)) == -1
        assert host.L.SolRx_RenderJpegBegin(0.0, quality, h, v, 0) == -1
    nxt = park(host, pixels, False)
    assert nxt // 4 == good // 4 + 1, "a refused call took a ticket"
    assert end(host, good)[0] == 0
    # the host-only engine renders nothing: a frame it is asked for fails as SolRx_RenderJpeg does, and takes no ticket
    assert host.L.SolRx_RenderJpegBegin(0.0, 85, 2, 2, 0) == -1
    with pytest.raises(solr.SolrError):
        host.render_jpeg_begin()
    after = park(host, pixels, False)
    assert after // 4 == nxt // 4 + 1, "a failed frame took a ticket"


def test_jpeg_stream_yields_the_files_in_order_with_a_step_between_them(solr, host, tmp_path):
    """six frames, a `step` that alternates between two pictures (where a device renders: two camera positions), every depth:
    every file is the synchronous one of the picture of its turn, in order, and step(i) comes before frame i is submitted
    and after frame i - depth has been collected at the latest.  (The frames come as pixels here: render_jpeg_begin is
    pointed at SolRx_JpegParkPixels; with a device the same generator runs over rendered frames, test_jpeg_stream_gpu.py.)"""
    pictures = [frame(37, 21, 11), frame(37, 21, 12)]
    for optimise in (False, True):
        want = [synchronous(host, tmp_path, pixels, optimise) for pixels in pictures]
        assert want[0] != want[1]
        for depth in (None, 1, 2, 3, 4, 9):
            log = []

            state = {"picture": None}

            def step(i):
                log.append(("step", i))
                state["picture"] = pictures[i % 2]

            def begin(**jpeg):
                log.append(("begin", len([e for e in log if e[0] == "begin"])))
                return park(host, state["picture"], jpeg.get("optimise", False))

            host.render_jpeg_begin = begin   # (on the instance: jpeg_stream asks self)
            try:
                files = []
                for file in host.jpeg_stream(6, step=step, depth=depth, optimise=optimise):
                    log.append(("file", len(files)))
                    files.append(file)
            finally:
                del host.render_jpeg_begin
            assert files == [want[i % 2] for i in range(6)], "depth %s" % depth
            deep = 1 if depth is None else min(depth, 4)   # (the host-only engine has one frame in flight)
            for i in range(6):
                assert log.index(("step", i)) < log.index(("begin", i)) < log.index(("file", i))
                if i + deep < 6:
                    assert log.index(("file", i)) < log.index(("step", i + deep)), "more than %d tickets outstanding" % deep
                if i + deep - 1 < 6:
                    assert log.index(("begin", i + deep - 1)) < log.index(("file", i)), "fewer than %d submitted ahead" % deep


BITS_1080P = (120 * 68 * 6) * 1665 + 7


@pytest.mark.parametrize("total", [0, 1, 7, 8, 31, 32, 33, 2047, 2048, 2049, BITS_1080P])
def test_the_plan_is_the_stream_sizes_of_the_header(host, total):
    sizes = (C.c_ulonglong * 3)()
    host.L.SolRx_JpegEntropyStreamSizes(total, sizes)
    nb_bytes, nb_words, tail = sizes[0], sizes[1], sizes[2]
    assert nb_bytes == -(-total // 8) and nb_words == -(-total // 32) and tail == -total % 8   # (the header's, by hand)
    plan = (C.c_ulonglong * 9)()
    host.L.SolRx_JpegEntropyPlan(total, 0, 120 * 68 * 6, plan)
    assert plan[0] == total and plan[1] == nb_bytes and plan[4] == 0
    with_tail = (C.c_ulonglong * 3)()
    host.L.SolRx_JpegEntropyStreamSizes(total + tail, with_tail)
    assert plan[2] == with_tail[1] == -(-nb_bytes // 4), "the words emit touches are the words stuff reads"
    assert plan[3] == -(-nb_bytes // 256)
    # the bounds of a 1080p frame at 2x2: what the slots are cut by
    assert plan[5] == BITS_1080P and plan[6] == -(-BITS_1080P // 8) and plan[7] == -(-plan[6] // 256) and plan[8] == 2 * plan[6]
    assert plan[0] <= plan[5] and plan[3] <= plan[7]
    # flagged: no extent whatever the total
    host.L.SolRx_JpegEntropyPlan(total, 1, 120 * 68 * 6, plan)
    assert list(plan[:5]) == [0, 0, 0, 0, 1]


@pytest.mark.parametrize("nb_bytes, chunks", [(255, 1), (256, 1), (257, 2)])
def test_the_chunk_count_around_a_chunks_bytes(host, nb_bytes, chunks):
    granularity = (C.c_int * 2)()
    host.L.SolRx_JpegEntropyGranularity(granularity)
    assert granularity[1] == 256
    plan = (C.c_ulonglong * 9)()
    for total in (8 * nb_bytes, 8 * nb_bytes - 7):
        host.L.SolRx_JpegEntropyPlan(total, 0, 6, plan)
        assert plan[1] == nb_bytes and plan[3] == chunks, (total, list(plan))


def test_the_resident_loops_are_clean_under_the_sanitizers(tmp_path):
    """tests/jpeg_stream_check.cpp: three synthetic cases - large, small, large - twice through one set of buffers that is
    never zeroed in between, compiled with the address and undefined-behaviour sanitizers and run as a program of its own
    (no device code in it, nothing loaded into Python); its buffers are cut exactly by the slots' bounds"""
    cases = {c["name"]: c for c in JC.cases()}
    chosen = [cases[name] for name in ("row_of_512_mcus", "one_mcu", "ff_chunk_edge")]
    assert len(chosen[0]["blocks"]) > len(chosen[2]["blocks"]) > len(chosen[1]["blocks"])
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(chosen)))
        for c in chosen:
            scan, _, _ = JC.model_scan(c["blocks"], c["sampling"])
            f.write(struct.pack("<iiiiqq", c["sampling"][0], c["sampling"][1], c["width"], c["height"], len(c["blocks"]),
                                len(scan)))
            f.write(np.ascontiguousarray(c["blocks"], np.int16).tobytes())
            f.write(scan)
    exe = str(tmp_path / "jpeg_stream_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "jpeg_stream_check.cpp")], check=True)
    run = subprocess.run([exe, path], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "6 uses of one slot" in run.stdout
