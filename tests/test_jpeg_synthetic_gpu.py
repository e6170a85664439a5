"""The JPEG pixel stage on the device (k_jpegPixels, csrc/solr_textures.hip) on the files written from synthesised
coefficient blocks: see tests/test_jpeg_synthetic.py for the fixture set and its two tiers.  Every file goes two ways:

    load_texture            the file through the host's Huffman stage and the kernel
    solr_hip_jpeg_to_rgb    the fixture's own coefficient blocks and frame straight into the kernel

and both must give every byte of `expected/` (exact tier: the reference's jpgd) or `wrapped/` (wrap tier: the int64 model
with the engine's wrap semantics).  Where only the first fails the Huffman stage is wrong, where both fail the kernel.
The wrap-tier files are ordinary in-range launches whose arithmetic wraps; a frame is rendered after them all the same."""
import ctypes as C
import os

import numpy as np
import pytest

from test_jpeg_synthetic import EXACT, FIXTURES, NAMES, WRAP, bytes_the_loader_owes, frame_of, path_of

pytestmark = pytest.mark.gpu


def output_blocks(name):
    """8x8 blocks the pixel stage produces for a file: 3, 4 or 12 per MCU (2x2 chroma comes out at full resolution)"""
    width, height, (h, v), _ = frame_of(name)
    return -(-width // (8 * h)) * -(-height // (8 * v)) * {(1, 1): 3, (2, 1): 4, (2, 2): 12}[(h, v)]


def assert_bytes(got, name, route):
    e = bytes_the_loader_owes(name)
    assert got.size == e.size
    got = got.reshape(e.shape)
    assert np.array_equal(got, e), "%s: %d of %d bytes differ from %s, first at %s" % (
        route, (got != e).sum(), e.size, "jpgd" if name in EXACT else "the wrapped model",
        np.argwhere(got != e)[:4].tolist())


def through_the_file(solr, name):
    hip = solr.hip_lib()
    k = solr.Kernel(engine="hip")
    hip.solr_hip_clear_error()
    before = hip.solr_hip_jpeg_blocks()
    assert k.load_texture(0, path_of(name))
    assert hip.solr_hip_jpeg_blocks() - before == output_blocks(name), "the pixel stage did not run on the device"
    assert_bytes(k.flat_scene().textures, name, "load_texture")
    assert hip.solr_hip_last_error(None, 0) == 0


def through_the_blocks(solr, name):
    hip = solr.hip_lib()
    hip.solr_hip_clear_error()
    width, height, (h, v), quant = frame_of(name)
    frame = solr.JpegFrame()
    frame.width, frame.height, frame.lumaH, frame.lumaV = width, height, h, v
    frame.mcusPerRow, frame.mcuRows = -(-width // (8 * h)), -(-height // (8 * v))
    for c in range(3):
        for i in range(64):
            frame.quant[c][i] = int(quant[c][i])
    blocks = np.ascontiguousarray(FIXTURES["coefficients/" + name])
    rgb = np.full((height, width, 3), 0xEE, np.uint8)
    before = hip.solr_hip_jpeg_blocks()
    assert hip.solr_hip_jpeg_to_rgb(C.byref(frame), blocks.ctypes.data, len(blocks), rgb.ctypes.data) == 0
    assert hip.solr_hip_jpeg_blocks() - before == output_blocks(name)
    assert_bytes(rgb, name, "solr_hip_jpeg_to_rgb")
    assert hip.solr_hip_last_error(None, 0) == 0


@pytest.mark.parametrize("name", EXACT)
def test_an_exact_tier_file_is_decoded_to_the_reference_decoders_bytes(solr, name):
    through_the_blocks(solr, name)
    through_the_file(solr, name)


@pytest.mark.parametrize("name", WRAP)
def test_a_wrap_tier_file_is_decoded_to_the_wrapped_models_bytes(solr, name):
    through_the_blocks(solr, name)
    through_the_file(solr, name)


def test_the_engine_renders_after_the_wrap_tier_files(solr):
    assert sorted(EXACT + WRAP) == NAMES
    for name in WRAP:
        through_the_blocks(solr, name)
    k = solr.Kernel(engine="hip")
    for slot, name in enumerate(WRAP):
        assert k.load_texture(slot, path_of(name))
    solr.scenes.cornell(k, width=32, height=24, iterations=1)
    k.render()
    k.check(0, "a frame after the wrap-tier files")
    k.finalize()
