"""The JPEG screenshot writer on the device (k_jpegCoefficients, csrc/solr_jpeg_encode.hip) and SolR_GenerateScreenshot on
the HIP engine: see tests/test_jpeg_encoder.py for the fixture set.  Every picture goes two ways:

    solr_hip_rgb_to_jpeg_blocks   the picture straight into the kernel: the blocks must be jpge's, every coefficient
    encode_jpeg                   the picture through the kernel and the host's Huffman coder: the file must be jpge's

Where only the second fails the coder or the hook is wrong, where both fail the kernel.  The engine's counter of encoded
blocks must advance by exactly the picture's block count: the kernel ran, not the host's loop.  Screenshots are held to
the encoding of a hand-run loop of frames, for both frame-buffer types and with frames in flight (for ftBGR, whose frames
are not a function of the scene at these sizes, see the test)."""
import ctypes as C
import os

import numpy as np
import pytest

from test_jpeg_encoder import BAD_ARGUMENTS, NAMES, assert_same_blocks, assert_same_file, case

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A


def source_of(solr, width, height, sampling, quality, turned=0, swap=0):
    s = solr.JpegSource()
    s.width, s.height, s.lumaH, s.lumaV, s.quality, s.turned, s.swapRedBlue = (width, height, sampling[0], sampling[1],
                                                                                quality, turned, swap)
    return s


@pytest.mark.parametrize("name", NAMES)
def test_the_kernel_gives_jpges_blocks(solr, name):
    hip = solr.hip_lib()
    hip.solr_hip_clear_error()
    pixels, width, height, sampling, quality, turned, swap, _, blocks = case(name)
    pixels = np.ascontiguousarray(pixels)
    got = np.full(blocks.shape, SENTINEL, np.int16)
    before = hip.solr_hip_jpeg_encoded_blocks()
    source = source_of(solr, width, height, sampling, quality, turned, swap)
    assert hip.solr_hip_rgb_to_jpeg_blocks(C.byref(source), pixels.ctypes.data, got.ctypes.data, len(got)) == 0
    assert hip.solr_hip_jpeg_encoded_blocks() - before == len(blocks), "the pixel stage did not run on the device"
    assert_same_blocks(got, blocks, name)
    assert hip.solr_hip_last_error(None, 0) == 0


@pytest.fixture(scope="module")
def engine(solr):
    k = solr.Kernel(engine="hip")
    yield k
    k.finalize()


@pytest.mark.parametrize("name", NAMES)
def test_encode_jpeg_on_the_hip_engine_writes_jpges_bytes(solr, engine, tmp_path, name):
    hip = solr.hip_lib()
    hip.solr_hip_clear_error()
    pixels, _, _, sampling, quality, turned, swap, want, blocks = case(name)
    path = str(tmp_path / "out.jpg")
    before = hip.solr_hip_jpeg_encoded_blocks()
    engine.encode_jpeg(path, pixels, quality=quality, sampling=sampling, turned=bool(turned), swap_red_blue=bool(swap))
    assert hip.solr_hip_jpeg_encoded_blocks() - before == len(blocks), "the pixel stage did not run on the device"
    assert_same_file(open(path, "rb").read(), want, name)
    assert hip.solr_hip_last_error(None, 0) == 0


@pytest.mark.parametrize("bad", BAD_ARGUMENTS + [dict(blocks=5), dict(null="rgb"), dict(null="coefficients"),
                                                 dict(null="source")],
                         ids=lambda b: "_".join("%s=%s" % kv for kv in b.items()))
def test_bad_arguments_are_refused_with_nothing_launched(solr, bad):
    hip = solr.hip_lib()
    hip.solr_hip_clear_error()
    a = dict(width=8, height=8, quality=85, sampling=(2, 2), blocks=6, null=None)
    a.update(bad)
    pixels = np.zeros((8, 8, 3), np.uint8)
    out = np.full((6, 64), SENTINEL, np.int16)
    source = source_of(solr, a["width"], a["height"], a["sampling"], a["quality"])
    before = hip.solr_hip_jpeg_encoded_blocks()
    status = hip.solr_hip_rgb_to_jpeg_blocks(None if a["null"] == "source" else C.byref(source),
                                             None if a["null"] == "rgb" else pixels.ctypes.data,
                                             None if a["null"] == "coefficients" else out.ctypes.data, a["blocks"])
    message = C.create_string_buffer(512)
    assert status == -1 and hip.solr_hip_last_error(message, 512) != 0
    assert b"solr_hip_rgb_to_jpeg_blocks" in message.value
    assert hip.solr_hip_jpeg_encoded_blocks() == before and (out == np.int16(SENTINEL)).all()
    hip.solr_hip_clear_error()


OLD_SIZE = (32, 32)      # square: an ftBGR frame is then a function of the scene (below), so before == after can be asked


def bgr_writers(width, height):
    """Which pixels write position i of an ftBGR bitmap.  The reference's makeColor (GS:144-154, csrc/rt_device.h) puts
    pixel `index` at (index / height + 1) * height - index % width - 1, blue first.  On a square frame that mirrors every
    row; on any other frame some positions are written by two pixels - whichever wave stores last wins, so the frame is
    not a function of the scene there - and as many by none (they keep what the buffer held).  Returns the position of
    every pixel and the number of writers of every position."""
    index = np.arange(width * height)
    position = (index // height + 1) * height - index % width - 1
    assert position.min() >= 0 and position.max() < width * height
    return position, np.bincount(position, minlength=width * height)


def delivered_frame(k, width, height):
    ptr = k.L.SolRx_GetBitmap()
    assert ptr
    return np.frombuffer((C.c_ubyte * (width * height * 3)).from_address(ptr), np.uint8).reshape(height, width, 3).copy()


@pytest.mark.parametrize("frame_buffer", ["ftRGB", "ftBGR"])
@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("width, height, flights", [(40, 24, 1), (37, 21, 3)])
def test_a_screenshot_is_the_encoding_of_the_last_frame_of_a_hand_run_loop(solr, tmp_path, width, height, flights,
                                                                           passes, frame_buffer):
    """ftRGB: the file is encode_jpeg of the reordered last image of a hand-run loop of frames, every byte.

    ftBGR at these sizes: the reference's BGR indexing lets two pixels write 384 of the 960 positions of a 40 x 24 frame
    (336 of 777 at 37 x 21) and which one lands last differs from run to run (seen on an MI355X: the file of one run 1141
    bytes, of the next 1145), so two renderings of the same frame need not be the same bytes and neither need their files.
    What is a function of the scene is held exactly all the same: the file is encode_jpeg of the frame the screenshot
    delivered; that frame equals the hand-run loop's at every position with one writer, and at a position with two it holds
    the colour of one of the two, taken from the same loop rendered as ftRGB."""
    hip = solr.hip_lib()
    hip.solr_hip_clear_error()
    fb = getattr(solr, frame_buffer)
    k = solr.Kernel(engine="hip")
    solr.scenes.cornell(k, width=OLD_SIZE[0], height=OLD_SIZE[1], iterations=2, frameBufferType=fb)
    before = k.render()
    assert before.any()
    k.L.SolRx_SetFramesInFlight(flights)
    shot = str(tmp_path / "shot.jpg")
    encoded = hip.solr_hip_jpeg_encoded_blocks()
    k.screenshot(shot, width, height, passes)
    assert hip.solr_hip_jpeg_encoded_blocks() - encoded == -(-width // 16) * -(-height // 16) * 6
    frame = delivered_frame(k, width, height)
    k.L.SolRx_SetFramesInFlight(1)
    after = k.render()
    assert np.array_equal(before, after), "the frame rendered after the screenshot is not the one rendered before it"
    got = open(shot, "rb").read()
    assert got[:2] == b"\xff\xd8" and got[-2:] == b"\xff\xd9"
    what = "screenshot %dx%d, %d passes, %s" % (width, height, passes, frame_buffer)

    def loop(frame_buffer_type):
        for i in range(passes):
            last = k.render(width=width, height=height, pathTracingIteration=i, maxPathTracingIterations=passes,
                            frameBufferType=frame_buffer_type)
        return last

    by_hand = str(tmp_path / "by_hand.jpg")
    if fb == solr.ftRGB:
        k.encode_jpeg(by_hand, loop(fb), quality=85, sampling=(2, 2), turned=True, swap_red_blue=False)
        assert_same_file(got, open(by_hand, "rb").read(), what)
    else:
        k.encode_jpeg(by_hand, frame, quality=85, sampling=(2, 2), turned=True, swap_red_blue=True)
        assert_same_file(got, open(by_hand, "rb").read(), what + " (the frame it delivered)")
        position, writers = bgr_writers(width, height)
        frame, again = frame.reshape(-1, 3), loop(fb).reshape(-1, 3)
        colours = loop(solr.ftRGB).reshape(-1, 3)[:, ::-1]           # what every pixel writes, blue first
        once = writers == 1
        assert np.array_equal(frame[once], again[once]), what + ": differs from the hand-run loop where one pixel writes"
        holds_a_writer = np.zeros(width * height, bool)
        holds_a_writer[position[(frame[position] == colours).all(axis=-1)]] = True
        assert holds_a_writer[writers >= 1].all(), what + ": a position holds the colour of none of its writers"
    k.check(0, "a screenshot")
    k.finalize()


def test_a_frame_renders_cleanly_after_all_of_it(solr, tmp_path):
    hip = solr.hip_lib()
    hip.solr_hip_clear_error()
    k = solr.Kernel(engine="hip")
    solr.scenes.cornell(k, width=32, height=24, iterations=1)
    first = k.render()
    k.screenshot(str(tmp_path / "shot.jpg"), 17, 16, 2)
    k.encode_jpeg(str(tmp_path / "noise.jpg"), case("noise_37x21__420_q85")[0])
    again = k.render()
    k.check(0, "a frame after the screenshots")
    assert first.any() and np.array_equal(first, again)
    k.finalize()
