"""The entropy stage of the JPEG writer on the device (sol-r_amd/csrc/solr_jpeg_entropy.hip): solr_hip_jpeg_blocks_to_scan,
solr_hip_rgb_to_jpeg_scan and - through Kernel.render_jpeg - solr_hip_frame_to_jpeg_scan.

The kernels call the functions of csrc/jpeg_entropy.h that the host-only engine runs in loops, and tests/test_jpeg_entropy.py
holds those loops to the one-pass writer, to the fixture generator's coder and to jpge's files; here the device is held to
the host-only engine's bytes on the synthetic blocks of tests/jpeg_entropy_cases.py and on the fixtures' blocks, to jpge's
files from the fixtures' pixels, and a rendered frame's file to encode_jpeg of the same frame and to a screenshot.  Every
comparison is of every byte: no tolerance, no excluded case, no excluded byte."""
import ctypes as C

import numpy as np
import pytest

from test_jpeg_encoder import BAD_ARGUMENTS, NAMES, case
from test_jpeg_entropy import CASE_NAMES, HEADER_BYTES, by_name
from test_jpeg_encoder_gpu import source_of

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A


@pytest.fixture
def host(solr):
    """(per test: the engine is a singleton, and the tests below that render select the HIP engine)"""
    return solr.Kernel(engine="host-only")


def host_scan(host, blocks, width, height, sampling, quality=85):
    file = host.jpeg_from_coefficients(blocks, width, height, quality, sampling)
    assert file[HEADER_BYTES - 14:HEADER_BYTES - 12] == b"\xff\xda" and file[-2:] == b"\xff\xd9"
    return file[HEADER_BYTES:-2]


def assert_same_scan(got, want, what):
    if got == want:
        return
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    raise AssertionError("%s: the segment differs from the host-only engine's (%d bytes against %d), first at byte %d" % (
        what, len(got), len(want), first))


def device_scan(solr, blocks, width, height, sampling, quality=85):
    """solr_hip_jpeg_blocks_to_scan into a buffer that is exactly as large as the segment, a sentinel behind it"""
    hip = solr.hip_lib()
    hip.solr_hip_clear_error()
    blocks = np.ascontiguousarray(blocks, np.int16)
    source = source_of(solr, width, height, sampling, quality)
    size = C.c_long(0)
    none = np.full(16, SENTINEL, np.uint8)
    coded = hip.solr_hip_jpeg_coded_blocks()
    # capacity 0: the size comes back, nothing is written, no error
    assert hip.solr_hip_jpeg_blocks_to_scan(C.byref(source), blocks.ctypes.data, len(blocks), none.ctypes.data, 0,
                                            C.byref(size)) == -1
    assert size.value > 0 and (none == SENTINEL).all() and hip.solr_hip_last_error(None, 0) == 0
    assert hip.solr_hip_jpeg_coded_blocks() == coded
    out = np.full(size.value + 64, SENTINEL, np.uint8)
    needed = size.value
    assert hip.solr_hip_jpeg_blocks_to_scan(C.byref(source), blocks.ctypes.data, len(blocks), out.ctypes.data, needed,
                                            C.byref(size)) == 0
    assert size.value == needed and (out[needed:] == SENTINEL).all(), "bytes behind the segment were written"
    assert hip.solr_hip_jpeg_coded_blocks() - coded == len(blocks), "the entropy stage did not run on the device"
    assert hip.solr_hip_last_error(None, 0) == 0
    return out[:needed].tobytes()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_kernels_give_the_host_only_engines_segment_on_the_synthetic_cases(solr, host, name):
    c = by_name(name)
    want = host_scan(host, c["blocks"], c["width"], c["height"], c["sampling"])
    assert_same_scan(device_scan(solr, c["blocks"], c["width"], c["height"], c["sampling"]), want, name)


@pytest.mark.parametrize("name", NAMES)
def test_the_kernels_give_jpges_segment_on_the_fixtures_blocks(solr, host, name):
    _, width, height, sampling, quality, _, _, file, blocks = case(name)
    want = host_scan(host, blocks, width, height, sampling, quality)
    assert want == file[HEADER_BYTES:-2]
    assert_same_scan(device_scan(solr, blocks, width, height, sampling, quality), want, name)


def pixels_to_scan(solr, pixels, sampling, quality, turned=0, swap=0, room=None):
    hip = solr.hip_lib()
    hip.solr_hip_clear_error()
    pixels = np.ascontiguousarray(pixels, np.uint8)
    height, width, _ = pixels.shape
    source = source_of(solr, width, height, sampling, quality, turned, swap)
    out = np.full(room or width * height * 3 + 4096, SENTINEL, np.uint8)
    size = C.c_long(0)
    encoded, coded = hip.solr_hip_jpeg_encoded_blocks(), hip.solr_hip_jpeg_coded_blocks()
    assert hip.solr_hip_rgb_to_jpeg_scan(C.byref(source), pixels.ctypes.data, out.ctypes.data, len(out), C.byref(size)) == 0
    assert hip.solr_hip_last_error(None, 0) == 0 and (out[size.value:] == SENTINEL).all()
    nb_blocks = -(-width // (8 * sampling[0])) * -(-height // (8 * sampling[1])) * (sampling[0] * sampling[1] + 2)
    assert hip.solr_hip_jpeg_encoded_blocks() - encoded == nb_blocks == hip.solr_hip_jpeg_coded_blocks() - coded
    return out[:size.value].tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_pixels_to_segment_on_the_device_is_jpges_file_between_header_and_eoi(solr, name):
    pixels, _, _, sampling, quality, turned, swap, want, _ = case(name)
    assert_same_scan(pixels_to_scan(solr, pixels, sampling, quality, turned, swap), want[HEADER_BYTES:-2], name)


def test_a_1080p_frame_of_noise_at_quality_100(solr, host):
    """the one case of its size: 48 960 blocks, a stream of several megabytes, thousands of stuffing chunks"""
    pixels = np.random.RandomState(1080).randint(0, 256, (1080, 1920, 3)).astype(np.uint8)
    got = pixels_to_scan(solr, pixels, (2, 2), 100)
    blocks = np.zeros((120 * 68 * 6, 64), np.int16)
    assert host.L.SolRx_JpegCoefficients(pixels.ctypes.data, 1920, 1080, 100, 2, 2, 0, 0, blocks.ctypes.data,
                                         len(blocks)) == 0
    assert_same_scan(got, host_scan(host, blocks, 1920, 1080, (2, 2), 100), "1920 x 1080 noise")


OUTSIDE = [(0, 0, 2048), (3, 0, 1024), (1, 1, 1024), (5, 63, -1024)]


@pytest.mark.parametrize("block, position, value", OUTSIDE)
def test_a_block_outside_the_domain_is_refused_with_the_buffer_untouched(solr, block, position, value):
    hip = solr.hip_lib()
    hip.solr_hip_clear_error()
    blocks = np.zeros((6, 64), np.int16)
    blocks[0, 0] = -1024
    blocks[block, position] = value
    out = np.full(4096, SENTINEL, np.uint8)
    size = C.c_long(0)
    source = source_of(solr, 16, 8, (1, 1), 85)
    encoded, coded = hip.solr_hip_jpeg_encoded_blocks(), hip.solr_hip_jpeg_coded_blocks()
    assert hip.solr_hip_jpeg_blocks_to_scan(C.byref(source), blocks.ctypes.data, 6, out.ctypes.data, len(out),
                                            C.byref(size)) == -1
    message = C.create_string_buffer(512)
    assert hip.solr_hip_last_error(message, 512) != 0 and b"solr_hip_jpeg_blocks_to_scan" in message.value
    assert (out == SENTINEL).all()
    assert (hip.solr_hip_jpeg_encoded_blocks(), hip.solr_hip_jpeg_coded_blocks()) == (encoded, coded)
    hip.solr_hip_clear_error()


BAD = BAD_ARGUMENTS + [dict(null="input"), dict(null="scan"), dict(null="size"), dict(null="source"), dict(capacity=-1)]
REFUSALS = [("blocks", bad) for bad in BAD + [dict(blocks=5)]] + [("rgb", bad) for bad in BAD]


@pytest.mark.parametrize("entry, bad", REFUSALS,
                         ids=lambda v: v if isinstance(v, str) else "_".join("%s=%s" % kv for kv in v.items()))
def test_bad_arguments_are_refused_with_nothing_launched(solr, entry, bad):
    hip = solr.hip_lib()
    hip.solr_hip_clear_error()
    a = dict(width=8, height=8, quality=85, sampling=(2, 2), blocks=6, null=None, capacity=4096)
    a.update(bad)
    pixels = np.zeros((8, 8, 3), np.uint8)
    blocks = np.zeros((6, 64), np.int16)
    out = np.full(4096, SENTINEL, np.uint8)
    size = C.c_long(77)
    source = None if a["null"] == "source" else C.byref(source_of(solr, a["width"], a["height"], a["sampling"], a["quality"]))
    scan = None if a["null"] == "scan" else out.ctypes.data
    size_at = None if a["null"] == "size" else C.byref(size)
    encoded, coded = hip.solr_hip_jpeg_encoded_blocks(), hip.solr_hip_jpeg_coded_blocks()
    if entry == "blocks":
        status = hip.solr_hip_jpeg_blocks_to_scan(source, None if a["null"] == "input" else blocks.ctypes.data, a["blocks"],
                                                  scan, a["capacity"], size_at)
    else:
        status = hip.solr_hip_rgb_to_jpeg_scan(source, None if a["null"] == "input" else pixels.ctypes.data, scan,
                                               a["capacity"], size_at)
    message = C.create_string_buffer(512)
    assert status == -1 and hip.solr_hip_last_error(message, 512) != 0
    assert (b"solr_hip_jpeg_blocks_to_scan" if entry == "blocks" else b"solr_hip_rgb_to_jpeg_scan") in message.value
    assert (out == SENTINEL).all() and size.value == 77
    assert (hip.solr_hip_jpeg_encoded_blocks(), hip.solr_hip_jpeg_coded_blocks()) == (encoded, coded)
    hip.solr_hip_clear_error()


def host_bitmap(k, nb_bytes):
    ptr = k.L.SolRx_GetBitmap()
    assert ptr
    return np.frombuffer((C.c_ubyte * nb_bytes).from_address(ptr), np.uint8)


@pytest.mark.parametrize("frame_buffer, width, height, flights", [("ftRGB", 40, 24, 1), ("ftRGB", 37, 21, 1),
                                                                  ("ftBGR", 32, 32, 1), ("ftRGB", 40, 24, 3)])
def test_render_jpeg_is_the_file_of_the_frame(solr, tmp_path, frame_buffer, width, height, flights):
    """(ftBGR at 32 x 32 only: at other shapes such a frame is not a function of the scene, tests/test_jpeg_encoder_gpu.py)"""
    hip = solr.hip_lib()
    hip.solr_hip_clear_error()
    fb = getattr(solr, frame_buffer)
    k = solr.Kernel(engine="hip")
    solr.scenes.cornell(k, width=width, height=height, iterations=2, frameBufferType=fb)
    before = k.render()
    assert before.any()
    by_hand = str(tmp_path / "by_hand.jpg")
    k.encode_jpeg(by_hand, before, quality=85, sampling=(2, 2), turned=True, swap_red_blue=fb != solr.ftRGB)
    want = open(by_hand, "rb").read()

    bitmap = host_bitmap(k, width * height * 3)             # (brings the host bitmap up to date first)
    bitmap[:] = SENTINEL
    k.L.SolRx_SetFramesInFlight(flights)
    encoded, coded = hip.solr_hip_jpeg_encoded_blocks(), hip.solr_hip_jpeg_coded_blocks()
    got = k.render_jpeg(quality=85, sampling=(2, 2))
    nb_blocks = -(-width // 16) * -(-height // 16) * 6
    assert hip.solr_hip_jpeg_encoded_blocks() - encoded == nb_blocks == hip.solr_hip_jpeg_coded_blocks() - coded
    what = "render_jpeg %dx%d %s, %d in flight" % (width, height, frame_buffer, flights)
    assert got[:2] == b"\xff\xd8" and got[-2:] == b"\xff\xd9" and got == want, what + ": not encode_jpeg of render()"
    if flights == 1:
        # the device route: the frame never came to the host as pixels
        assert (host_bitmap(k, width * height * 3) == SENTINEL).all(), what + ": the host bitmap was refreshed"
    k.L.SolRx_SetFramesInFlight(1)
    assert np.array_equal(k.render(), before), what + ": the frame rendered afterwards is not the one rendered before"

    shot = str(tmp_path / "shot.jpg")
    k.screenshot(shot, width, height, 1)
    assert open(shot, "rb").read() == want, what + ": not a one-pass screenshot of that size"
    other = k.render_jpeg(quality=50, sampling=(1, 1))
    k.encode_jpeg(by_hand, before, quality=50, sampling=(1, 1), turned=True, swap_red_blue=fb != solr.ftRGB)
    assert other == open(by_hand, "rb").read(), what + " at quality 50, 1x1"
    k.check(0, "render_jpeg")
    k.finalize()


def test_render_jpeg_refuses_what_the_encoder_refuses(solr):
    hip = solr.hip_lib()
    hip.solr_hip_clear_error()
    k = solr.Kernel(engine="hip")
    solr.scenes.cornell(k, width=32, height=24, iterations=1)
    first = k.render()
    out = np.full(65536, SENTINEL, np.uint8)
    size = C.c_long(77)
    encoded, coded = hip.solr_hip_jpeg_encoded_blocks(), hip.solr_hip_jpeg_coded_blocks()
    for quality, h, v in ((0, 2, 2), (101, 2, 2), (85, 1, 2), (85, 3, 1)):
        assert k.L.SolRx_RenderJpeg(0.0, quality, h, v, out.ctypes.data, len(out), C.byref(size)) == -1
        assert size.value == 0 and (out == SENTINEL).all()
    assert (hip.solr_hip_jpeg_encoded_blocks(), hip.solr_hip_jpeg_coded_blocks()) == (encoded, coded)
    k.check(0, "refused render_jpeg calls")
    # a buffer too small: the size comes back, nothing is written
    assert k.L.SolRx_RenderJpeg(0.0, 85, 2, 2, out.ctypes.data, 100, C.byref(size)) == -1
    assert size.value > 100 and (out == SENTINEL).all()
    assert k.L.SolRx_RenderJpeg(0.0, 85, 2, 2, out.ctypes.data, size.value, C.byref(size)) == 0
    assert out[:2].tobytes() == b"\xff\xd8" and out[size.value - 2:size.value].tobytes() == b"\xff\xd9"
    assert np.array_equal(k.render(), first)
    k.check(0, "render_jpeg")
    k.finalize()
