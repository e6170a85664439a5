"""JPEG frames in flight on the device (sol-r_amd/csrc/solr_jpeg_entropy.hip: the resident slots, k_jpegPlan,
k_jpegCountFFResident, k_jpegStuffResident; include/solr_hip.h solr_hip_frame_to_jpeg_async, solr_hip_jpeg_wait): coefficient
blocks through the probe solr_hip_probe_jpeg_stream_blocks - the same slots and steps as a frame's - and rendered frames
through Kernel.render_jpeg_begin / render_jpeg_end / jpeg_stream.

Every comparison is byte equality against the synchronous path, which this feature leaves as it was:
solr_hip_jpeg_blocks_to_scan[_optimised] on the same blocks (tables included), render_jpeg and encode_jpeg of render() for
frames.  No tolerance, no excluded case.  What the tests aim at is the resident stream buffer: k_jpegEmit ORs into zeros, so a
slot that a longer stream used before must be zero again - large and small cases alternate in every slot, the modes too,
tickets are collected late and out of order, and a 1080p frame of noise is followed by the smallest case in its slot."""
import ctypes as C

import numpy as np
import pytest

import jpeg_entropy_cases as JC
from test_jpeg_encoder_gpu import source_of

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
CASES = JC.cases()
CASE_NAMES = [c["name"] for c in CASES]
MODES = [False, True]
_REFERENCE = {}


def reference(solr, c, optimise):
    """(segment, tables) of the synchronous entry on the case's blocks, computed once per case and mode"""
    key = (c["name"], optimise)
    if key not in _REFERENCE:
        _REFERENCE[key] = synchronous(solr, c["blocks"], c["width"], c["height"], c["sampling"], c["quality"], optimise)
    return _REFERENCE[key]


def synchronous(solr, blocks, width, height, sampling, quality, optimise):
    hip = solr.hip_lib()
    blocks = np.ascontiguousarray(blocks, np.int16)
    source = source_of(solr, width, height, sampling, quality)
    out = np.empty(len(blocks) * 420 + 64, np.uint8)     # (twice 1665 bits a block and seven)
    size = C.c_long(0)
    tables = solr.JpegHuffman()
    if optimise:
        status = hip.solr_hip_jpeg_blocks_to_scan_optimised(C.byref(source), blocks.ctypes.data, len(blocks), out.ctypes.data,
                                                            len(out), C.byref(size), C.byref(tables))
    else:
        status = hip.solr_hip_jpeg_blocks_to_scan(C.byref(source), blocks.ctypes.data, len(blocks), out.ctypes.data, len(out),
                                                  C.byref(size))
    assert status == 0 and hip.solr_hip_last_error(None, 0) == 0
    return out[:size.value].tobytes(), bytes(tables) if optimise else None


def submit(solr, c, optimise):
    hip = solr.hip_lib()
    blocks = np.ascontiguousarray(c["blocks"], np.int16)
    source = source_of(solr, c["width"], c["height"], c["sampling"], c["quality"])
    ticket = hip.solr_hip_probe_jpeg_stream_blocks(C.byref(source), blocks.ctypes.data, len(blocks), int(optimise))
    assert ticket >= 0 and hip.solr_hip_last_error(None, 0) == 0
    return ticket


def collect(solr, ticket, optimise):
    """solr_hip_jpeg_wait: the size first (capacity 0: nothing written, no error, the ticket stays good), then into a buffer
    of exactly that size with a sentinel behind it.  (segment, tables)"""
    hip = solr.hip_lib()
    size = C.c_long(0)
    none = np.full(16, SENTINEL, np.uint8)
    tables = solr.JpegHuffman()
    C.memset(C.byref(tables), SENTINEL, C.sizeof(tables))
    untouched = bytes(tables)
    at = C.byref(tables) if optimise else None
    assert hip.solr_hip_jpeg_wait(ticket, none.ctypes.data, 0, C.byref(size), at) == -1
    assert size.value > 0 and (none == SENTINEL).all() and hip.solr_hip_last_error(None, 0) == 0
    assert bytes(tables) == untouched, "the tables were written by a wait that delivered nothing"
    needed = size.value
    out = np.full(needed + 64, SENTINEL, np.uint8)
    assert hip.solr_hip_jpeg_wait(ticket, out.ctypes.data, needed, C.byref(size), at) == 0
    assert size.value == needed and (out[needed:] == SENTINEL).all(), "bytes behind the segment were written"
    assert hip.solr_hip_last_error(None, 0) == 0
    return out[:needed].tobytes(), bytes(tables) if optimise else None


def assert_same(got, want, what):
    if got == want:
        return
    first = next((i for i, (a, b) in enumerate(zip(got[0], want[0])) if a != b), min(len(got[0]), len(want[0])))
    raise AssertionError("%s: not the synchronous entry's result (segment %d bytes against %d, first difference at byte %d, "
                         "tables %s)" % (what, len(got[0]), len(want[0]), first, "equal" if got[1] == want[1] else "differ"))


@pytest.fixture(autouse=True)
def clean(solr):
    solr.hip_lib().solr_hip_clear_error()
    yield
    solr.hip_lib().solr_hip_clear_error()
    solr.hip_lib().solr_hip_set_frames_in_flight(1)         # (the knob outlives a kernel: not a failed test's for the next)


@pytest.mark.parametrize("optimise", MODES, ids=["standard", "optimised"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_probe_gives_the_synchronous_segment_on_the_synthetic_cases(solr, name, optimise):
    c = CASES[CASE_NAMES.index(name)]
    hip = solr.hip_lib()
    want = reference(solr, c, optimise)
    coded = hip.solr_hip_jpeg_coded_blocks()
    ticket = submit(solr, c, optimise)
    assert hip.solr_hip_jpeg_coded_blocks() == coded, "blocks are counted when they are collected"
    assert_same(collect(solr, ticket, optimise), want, name)
    assert hip.solr_hip_jpeg_coded_blocks() - coded == len(c["blocks"]), "counted once, by the wait that delivered"
    assert_same(collect(solr, ticket, optimise), want, name + ", collected again")
    assert hip.solr_hip_jpeg_coded_blocks() - coded == len(c["blocks"])


def dirty_sequence():
    """twelve cases: the six with the longest streams and the six with the shortest, large and small in turn, the turn
    reversed in every window of four - so that the slot of ticket j, which ticket j + 4 takes over, goes from large to
    small to large (or the other way round)"""
    by_length = sorted(CASES, key=lambda c: c["edges"]["unstuffed_bytes"])
    small, large = by_length[:6], by_length[-6:][::-1]
    assert small[-1]["edges"]["unstuffed_bytes"] * 8 < large[-1]["edges"]["unstuffed_bytes"]
    sequence = []
    for j in range(12):
        take_large = (j + j // 4) % 2 == 0
        sequence.append((large if take_large else small)[j // 2])
    for j in range(8):
        a, b = sequence[j]["edges"]["unstuffed_bytes"], sequence[j + 4]["edges"]["unstuffed_bytes"]
        assert a > 8 * b or b > 8 * a
    assert sum(1 for j in range(8) if sequence[j]["edges"]["unstuffed_bytes"] >
               sequence[j + 4]["edges"]["unstuffed_bytes"]) >= 4
    return sequence


@pytest.mark.parametrize("alternate", [False, True], ids=["standard", "modes_alternating"])
def test_slots_that_held_a_longer_stream_give_the_synchronous_segment(solr, alternate):
    """twelve tickets over the four slots; in every window of four the tickets are collected late - all four are outstanding
    first - and out of order"""
    sequence = dirty_sequence()
    mode = lambda j: alternate and (j + j // 4) % 2 == 1     # (ticket j + 4, in the same slot, has the other mode)
    if alternate:
        assert all(mode(j) != mode(j + 4) for j in range(8))
    for window in range(3):
        tickets = {}
        for j in range(4 * window, 4 * window + 4):
            tickets[j] = submit(solr, sequence[j], mode(j))
        assert len({t % 4 for t in tickets.values()}) == 4, "four tickets, four slots"
        for j in (4 * window + 2, 4 * window, 4 * window + 3, 4 * window + 1):
            c = sequence[j]
            assert_same(collect(solr, tickets[j], mode(j)), reference(solr, c, mode(j)),
                        "ticket %d (%s, %s)" % (j, c["name"], "optimised" if mode(j) else "standard"))


def test_a_1080p_frame_of_noise_at_quality_100_and_the_smallest_case_behind_it(solr):
    """48 960 blocks, megabytes of stream, thousands of chunks - and then, in the slot that stream dirtied, the case with
    the shortest stream there is"""
    hip = solr.hip_lib()
    pixels = np.random.RandomState(1080).randint(0, 256, (1080, 1920, 3)).astype(np.uint8)
    blocks = np.zeros((120 * 68 * 6, 64), np.int16)
    source = source_of(solr, 1920, 1080, (2, 2), 100)
    assert hip.solr_hip_rgb_to_jpeg_blocks(C.byref(source), pixels.ctypes.data, blocks.ctypes.data, len(blocks)) == 0
    noise = dict(name="noise", blocks=blocks, width=1920, height=1080, sampling=(2, 2), quality=100)
    want = synchronous(solr, blocks, 1920, 1080, (2, 2), 100, False)
    assert len(want[0]) > 2 << 20
    smallest = min(CASES, key=lambda c: c["edges"]["unstuffed_bytes"])
    first = submit(solr, noise, False)
    fillers = [submit(solr, smallest, False) for _ in range(3)]
    assert_same(collect(solr, first, False), want, "1920 x 1080 noise")
    behind = submit(solr, smallest, True)
    assert behind % 4 == first % 4, "the same slot"
    assert_same(collect(solr, behind, True), reference(solr, smallest, True), smallest["name"] + " behind the noise")
    for ticket in fillers:
        assert_same(collect(solr, ticket, False), reference(solr, smallest, False), smallest["name"])
    size = C.c_long(0)
    out = np.full(64, SENTINEL, np.uint8)
    assert hip.solr_hip_jpeg_wait(first, out.ctypes.data, 64, C.byref(size), None) == -1, "a stale ticket"
    assert hip.solr_hip_last_error(None, 0) != 0 and (out == SENTINEL).all()


OUTSIDE = [(0, 0, 2048), (3, 0, 1024), (1, 1, 1024), (5, 63, -1024)]


@pytest.mark.parametrize("optimise", MODES, ids=["standard", "optimised"])
@pytest.mark.parametrize("block, position, value", OUTSIDE)
def test_a_block_outside_the_domain_is_reported_by_the_wait_and_the_slot_is_good_afterwards(solr, block, position, value, optimise):
    hip = solr.hip_lib()
    blocks = np.zeros((6, 64), np.int16)
    blocks[0, 0] = -1024
    blocks[block, position] = value
    bad = dict(name="outside", blocks=blocks, width=16, height=8, sampling=(1, 1), quality=85)
    good = CASES[CASE_NAMES.index("ff_chunk_edge")]
    assert_same(collect(solr, submit(solr, good, optimise), optimise), reference(solr, good, optimise), "before")
    for _ in range(3):
        submit(solr, good, optimise)
    coded = hip.solr_hip_jpeg_coded_blocks()
    ticket = submit(solr, bad, optimise)           # in the slot the first good ticket dirtied and cleared
    out = np.full(4096, SENTINEL, np.uint8)
    size = C.c_long(77)
    tables = solr.JpegHuffman()
    assert hip.solr_hip_jpeg_wait(ticket, out.ctypes.data, len(out), C.byref(size), C.byref(tables)) == -1
    message = C.create_string_buffer(512)
    assert hip.solr_hip_last_error(message, 512) != 0 and b"solr_hip_jpeg_wait" in message.value and b"outside" in message.value
    assert (out == SENTINEL).all() and hip.solr_hip_jpeg_coded_blocks() == coded
    hip.solr_hip_clear_error()
    later = [submit(solr, good, optimise) for _ in range(4)]
    assert later[3] % 4 == ticket % 4
    assert_same(collect(solr, later[3], optimise), reference(solr, good, optimise), "the next ticket in that slot")


def host_bitmap(k, nb_bytes):
    ptr = k.L.SolRx_GetBitmap()
    assert ptr
    return np.frombuffer((C.c_ubyte * nb_bytes).from_address(ptr), np.uint8)


EYES = [(0.0, 0.0, -15000.0), (900.0, 300.0, -14000.0), (-1200.0, 0.0, -15500.0), (0.0, 800.0, -13000.0),
        (400.0, -600.0, -16000.0), (-300.0, 200.0, -14500.0)]


@pytest.mark.parametrize("optimise", MODES, ids=["standard", "optimised"])
@pytest.mark.parametrize("flights", [1, 3])
@pytest.mark.parametrize("frame_buffer, width, height", [("ftRGB", 40, 24), ("ftRGB", 37, 21), ("ftBGR", 32, 32)])
def test_frames_in_flight_are_the_files_of_their_own_frames(solr, tmp_path, frame_buffer, width, height, flights, optimise):
    """six frames, the camera moved between them, up to four tickets outstanding (the four that stay good), collected late;
    every file is render_jpeg's of that camera and encode_jpeg of its render() - taken first, on the same engine: the engine
    is a singleton and a second kernel would be the same one"""
    hip = solr.hip_lib()
    fb = getattr(solr, frame_buffer)
    k = solr.Kernel(engine="hip")
    solr.scenes.cornell(k, width=width, height=height, iterations=2, frameBufferType=fb)
    want, images = [], []
    by_hand = str(tmp_path / "by_hand.jpg")
    for eye in EYES:
        k.set_camera(eye)
        images.append(k.render())
        k.encode_jpeg(by_hand, images[-1], quality=85, sampling=(2, 2), turned=True, swap_red_blue=fb != solr.ftRGB,
                      optimise=optimise)
        want.append(open(by_hand, "rb").read())
        assert k.render_jpeg(quality=85, sampling=(2, 2), optimise=optimise) == want[-1]
    assert len(set(want)) == len(EYES), "the camera moves the picture"
    bitmap = host_bitmap(k, width * height * 3)             # (brings the host bitmap up to date first)
    bitmap[:] = SENTINEL
    k.L.SolRx_SetFramesInFlight(flights)
    stats = (C.c_ulonglong * 4)()
    hip.solr_hip_jpeg_stream_stats(stats)
    issued, waits = stats[0], stats[2]
    nb_blocks = -(-width // 16) * -(-height // 16) * 6
    encoded, coded = hip.solr_hip_jpeg_encoded_blocks(), hip.solr_hip_jpeg_coded_blocks()
    tickets, got = [], {}
    for i, eye in enumerate(EYES):
        if len(tickets) == 4:                                # frames 0 and 1 make room for 4 and 5
            j, t = tickets.pop(0)
            got[j] = k.render_jpeg_end(t)
        k.set_camera(eye)
        tickets.append((i, k.render_jpeg_begin(quality=85, sampling=(2, 2), optimise=optimise)))
    for j, t in reversed(tickets):                           # ... and the last four come out of order
        got[j] = k.render_jpeg_end(t)
    hip.solr_hip_jpeg_stream_stats(stats)
    assert stats[0] - issued == len(EYES) and stats[2] == waits, "six tickets of the engine's, no wait while submitting"
    assert hip.solr_hip_jpeg_encoded_blocks() - encoded == len(EYES) * nb_blocks == hip.solr_hip_jpeg_coded_blocks() - coded
    for i in range(len(EYES)):
        what = "frame %d of %dx%d %s, %d in flight" % (i, width, height, frame_buffer, flights)
        assert got[i][:2] == b"\xff\xd8" and got[i][-2:] == b"\xff\xd9" and got[i] == want[i], what + ": not its own frame's file"
    assert (bitmap == SENTINEL).all(), "the host bitmap was written"
    # the same through the generator
    files = list(k.jpeg_stream(len(EYES), step=lambda i: k.set_camera(EYES[i]), quality=85, sampling=(2, 2), optimise=optimise))
    assert files == want
    assert (bitmap == SENTINEL).all(), "the host bitmap was written"
    k.L.SolRx_SetFramesInFlight(1)
    k.set_camera(EYES[0])
    assert np.array_equal(k.render(), images[0]), "the frame rendered afterwards is not the one rendered before"
    k.check(0, "render_jpeg_begin / render_jpeg_end")
    k.finalize()


@pytest.mark.parametrize("optimise", MODES, ids=["standard", "optimised"])
def test_begins_after_the_first_allocate_nothing_and_wait_for_nothing(solr, optimise):
    hip = solr.hip_lib()
    k = solr.Kernel(engine="hip")
    width, height = 72, 40
    solr.scenes.cornell(k, width=width, height=height, iterations=1)
    k.L.SolRx_SetFramesInFlight(3)
    nb_blocks = -(-width // 16) * -(-height // 16) * 6
    stats = (C.c_ulonglong * 4)()
    first = [k.render_jpeg_begin(optimise=optimise) for _ in range(4)]    # every slot once at this size
    want = k.render_jpeg_end(first[3])
    hip.solr_hip_jpeg_stream_stats(stats)
    before = list(stats)
    coded = hip.solr_hip_jpeg_coded_blocks()
    delivered = 0
    for i in range(10):
        ticket = k.render_jpeg_begin(optimise=optimise)
        hip.solr_hip_jpeg_stream_stats(stats)
        assert stats[1] == before[1] and stats[2] == before[2] == 0, "begin %d allocated or waited" % i
        assert hip.solr_hip_jpeg_coded_blocks() == coded + i * nb_blocks
        file = k.render_jpeg_end(ticket)
        assert file == want, "the same camera, the same file"
        assert k.render_jpeg_end(ticket) == file
        delivered += len(file)
        assert hip.solr_hip_jpeg_coded_blocks() == coded + (i + 1) * nb_blocks, "blocks advance once per collected ticket"
    hip.solr_hip_jpeg_stream_stats(stats)
    assert stats[0] == before[0] + 10
    # bytes delivered are the segments': the files less EOI and header - 623 bytes with the standard tables, fewer with
    # tables that list only the symbols there are
    header = delivered - (stats[3] - before[3]) - 10 * 2
    assert header == 10 * 623 if not optimise else 10 * 200 < header < 10 * 623 and header % 10 == 0
    k.L.SolRx_SetFramesInFlight(1)                         # (the engine's knob outlives the kernel)
    k.check(0, "render_jpeg_begin")
    k.finalize()


def test_a_capacity_too_small_on_a_frames_ticket_costs_no_second_frame(solr):
    hip = solr.hip_lib()
    k = solr.Kernel(engine="hip")
    solr.scenes.cornell(k, width=40, height=24, iterations=1)
    want = k.render_jpeg()
    k.render()
    ticket = hip.solr_hip_frame_to_jpeg_async(85, 2, 2, 0)
    assert ticket >= 0
    stats = (C.c_ulonglong * 4)()
    hip.solr_hip_jpeg_stream_stats(stats)
    issued = stats[0]
    out = np.full(1 << 16, SENTINEL, np.uint8)
    size = C.c_long(0)
    assert hip.solr_hip_jpeg_wait(ticket, out.ctypes.data, 10, C.byref(size), None) == -1
    assert size.value > 10 and (out == SENTINEL).all() and hip.solr_hip_last_error(None, 0) == 0
    needed = size.value
    assert hip.solr_hip_jpeg_wait(ticket, out.ctypes.data, needed, C.byref(size), None) == 0 and size.value == needed
    assert (out[needed:] == SENTINEL).all()
    hip.solr_hip_jpeg_stream_stats(stats)
    assert stats[0] == issued, "the second wait took a ticket"
    assert out[:needed].tobytes() == want[-needed - 2:-2], "the segment of render_jpeg's file"
    # ... and through the host layer, whose first buffer is too small for this file
    ticket = k.render_jpeg_begin()
    hip.solr_hip_jpeg_stream_stats(stats)
    issued = stats[0]
    assert k.render_jpeg_end(ticket, room=64) == want
    hip.solr_hip_jpeg_stream_stats(stats)
    assert stats[0] == issued
    # bad arguments: refused with the error set, nothing launched, no ticket
    for quality, h, v in ((0, 2, 2), (101, 2, 2), (85, 1, 2), (85, 3, 1)):
        assert hip.solr_hip_frame_to_jpeg_async(quality, h, v, 0) == -1 and hip.solr_hip_last_error(None, 0) != 0
        hip.solr_hip_clear_error()
        assert k.L.SolRx_RenderJpegBegin(0.0, quality, h, v, 0) == -1
    hip.solr_hip_jpeg_stream_stats(stats)
    assert stats[0] == issued
    k.check(0, "refused begins")
    k.finalize()


def test_a_strip_is_declined_by_the_engine_and_delivered_by_the_host_road(solr):
    hip = solr.hip_lib()
    k = solr.Kernel(engine="hip")
    width, height = 40, 24
    solr.scenes.cornell(k, width=width, height=height, iterations=1)
    want = {optimise: k.render_jpeg(optimise=optimise) for optimise in MODES}
    stats = (C.c_ulonglong * 4)()
    hip.solr_hip_jpeg_stream_stats(stats)
    issued = stats[0]
    try:
        hip.solr_hip_set_strip(0, height)                  # a strip - of every row, so that the host road has the frame
        k.render()
        assert hip.solr_hip_jpeg_stream_offered() == 0
        assert hip.solr_hip_frame_to_jpeg_async(85, 2, 2, 0) == -1 and hip.solr_hip_last_error(None, 0) == 0
        for optimise in MODES:
            ticket = k.render_jpeg_begin(optimise=optimise)
            assert k.render_jpeg_end(ticket) == want[optimise]
        hip.solr_hip_jpeg_stream_stats(stats)
        assert stats[0] == issued, "the engine handed out a ticket for a strip"
    finally:
        hip.solr_hip_set_strip(0, -1)
    assert hip.solr_hip_jpeg_stream_offered() == 1
    assert k.render_jpeg_end(k.render_jpeg_begin()) == want[False]
    hip.solr_hip_jpeg_stream_stats(stats)
    assert stats[0] == issued + 1
    k.check(0, "strips")
    k.finalize()
