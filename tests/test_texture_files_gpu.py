"""Texture files on the HIP engine: the pixel stage of the JPEG loader runs in a kernel (csrc/solr_textures.hip behind
solr_hip_jpeg_to_rgb) and is held to the same arrays as the CPU loop in tests/test_texture_files.py - the reference
decoder's output, every byte equal - and to having actually run: solr_hip_jpeg_blocks() counts the 8x8 blocks the
device produced, so a silent fall-back to the CPU loop fails."""
import ctypes as C
import importlib
import os
import shutil

import numpy as np
import pytest

from helpers import assert_parity, compare_frames, gpu_frame, oracle_frame

pytestmark = pytest.mark.gpu
solr_mod = importlib.import_module("sol-r_amd")

HERE = os.path.dirname(os.path.abspath(__file__))
TEXTURES = os.path.join(HERE, "golden", "textures")
EXPECTED = np.load(os.path.join(HERE, "golden", "texture_files.npz"))
JPEGS = sorted(name for name in EXPECTED.files if name.endswith(".jpg"))
QUAD = os.path.join(TEXTURES, "quad.obj")


def output_blocks(path):
    """8x8 blocks the pixel stage produces for a file, from its frame header: 3, 4 or 12 per MCU (2x2 chroma comes
    out at full resolution)"""
    d = open(path, "rb").read()
    pos = 2
    while d[pos + 1] not in (0xC0, 0xC1):
        pos += 2 + int.from_bytes(d[pos + 2:pos + 4], "big")
    height, width = int.from_bytes(d[pos + 5:pos + 7], "big"), int.from_bytes(d[pos + 7:pos + 9], "big")
    h, v = d[pos + 11] >> 4, d[pos + 11] & 15
    mcus = -(-width // (8 * h)) * -(-height // (8 * v))
    return mcus * {(1, 1): 3, (2, 1): 4, (2, 2): 12}[(h, v)]


def test_block_counts_of_the_fixtures():
    # the three samplings, partial MCUs on both edges, one MCU, many workgroups
    assert {name: output_blocks(os.path.join(TEXTURES, name)) for name in JPEGS} == {
        "0100d.jpg": 4096 * 3, "0220r.jpg": 1024 * 12, "420_31x31_optimized.jpg": 4 * 12, "420_37x21.jpg": 6 * 12,
        "420_40x40_restart2.jpg": 9 * 12, "422_33x9.jpg": 6 * 4, "444_16x16_q100.jpg": 4 * 3, "444_24x17.jpg": 9 * 3,
        "444_8x8_flat.jpg": 3}


@pytest.mark.parametrize("name", JPEGS)
def test_a_jpeg_file_is_decoded_on_the_device_to_the_reference_decoders_bytes(solr, name):
    hip = solr.hip_lib()
    k = solr.Kernel(engine="hip")
    hip.solr_hip_clear_error()
    before = hip.solr_hip_jpeg_blocks()
    path = os.path.join(TEXTURES, name)
    assert k.load_texture(0, path)                        # (before SolR_InitializeKernel: no scene yet)
    assert hip.solr_hip_jpeg_blocks() - before == output_blocks(path), "the pixel stage did not run on the device"
    e = EXPECTED[name]
    got = k.flat_scene().textures
    assert got.size == e.size
    got = got.reshape(e.shape)
    assert np.array_equal(got, e), "%d of %d bytes differ from the reference decoder, first at %s" % (
        (got != e).sum(), e.size, np.argwhere(got != e)[:4].tolist())
    assert hip.solr_hip_last_error(None, 0) == 0


def textured_quad(solr, path=QUAD):
    k = solr.Kernel(engine="hip", deterministic_seed=1)
    solr.scenes.obj_model(k, path, width=64, height=48, iterations=2)
    return k


def test_loading_between_two_frames(solr):
    hip = solr.hip_lib()
    k = textured_quad(solr)
    first = gpu_frame(k)
    before = hip.solr_hip_jpeg_blocks()
    for slot, name in ((1, "0220r.jpg"), (2, "422_33x9.jpg")):
        assert k.load_texture(slot, os.path.join(TEXTURES, name))
    assert hip.solr_hip_jpeg_blocks() - before == 1024 * 12 + 6 * 4
    k.check(0, "loading between frames")
    second = gpu_frame(k)                                 # the atlas is uploaded again, now with three textures
    k.check(0, "the frame after loading")
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    atlas = k.flat_scene().textures
    assert np.array_equal(atlas, np.concatenate([EXPECTED[n].ravel() for n in ("444_24x17.jpg", "0220r.jpg",
                                                                                "422_33x9.jpg")]))
    k.finalize()


MATERIAL_FIELDS = [C.c_double] * 6 + [C.c_int] * 3 + [C.c_double] * 2 + [C.c_int] * 7 + [C.c_double] * 6 + [C.c_int]


def test_the_textured_quad_renders_the_same_three_ways(solr, oracle, tmp_path):
    # 1. the model's map_Kd loaded through the new path, pixels decoded on the device
    k = textured_quad(solr)
    frame = gpu_frame(k)
    pp, ids, rgb = frame
    flat = k.flat_scene()
    quad = np.isin(ids[..., 0], np.flatnonzero(flat.primitives["materialId"] == 0))
    assert quad.mean() > 0.15, "the quad is not in view"
    assert len(np.unique(rgb[quad].reshape(-1, 3), axis=0)) > 40, "the quad does not show its texture"
    # 2. against the oracle
    opp, oids, orgb, _, status = oracle_frame(k, oracle)
    assert status == 0
    assert_parity(compare_frames(pp, ids, rgb, opp, oids, orgb))
    material = [t() for t in MATERIAL_FIELDS]
    assert k.L.SolR_GetMaterial(0, *[C.byref(f) for f in material]) == 0
    assert material[11].value == 0                        # diffuseTextureId
    k.finalize()

    # 3. the same model without its image file, the texture supplied from the reference decoder's array
    for name in ("quad.obj", "quad.mtl"):
        shutil.copyfile(os.path.join(TEXTURES, name), str(tmp_path / name))
    k = textured_quad(solr, str(tmp_path / "quad.obj"))
    assert k.flat_scene().materials[0]["textureIds"][0] == -1
    k.set_texture(0, EXPECTED["444_24x17.jpg"])
    k.L.SolR_SetMaterial(0, *[f.value for f in material])
    supplied = gpu_frame(k)
    k.finalize()
    for a, b in zip(frame, supplied):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def grey_frame(solr, width=8, height=8, h=1, v=1):
    frame = solr.JpegFrame()
    frame.width, frame.height, frame.lumaH, frame.lumaV = width, height, h, v
    frame.mcusPerRow, frame.mcuRows = -(-width // (8 * h)), -(-height // (8 * v))
    for c in range(3):
        for i in range(64):
            frame.quant[c][i] = 1
    blocks = frame.mcusPerRow * frame.mcuRows * (h * v + 2)
    return frame, np.zeros((blocks, 64), np.int16), blocks, np.full((height, width, 3), 7, np.uint8)


def last_error(hip):
    buf = C.create_string_buffer(512)
    return hip.solr_hip_last_error(buf, 512), buf.value.decode()


def test_bad_arguments_are_refused_on_the_host_and_leave_the_engine_usable(solr):
    hip = solr.hip_lib()
    hip.solr_hip_clear_error()
    frame, zeros, blocks, rgb = grey_frame(solr)
    tall, tall_zeros, tall_blocks, _ = grey_frame(solr, h=1, v=2)
    produced = hip.solr_hip_jpeg_blocks()
    cases = [
        ("null", (None, zeros.ctypes.data, blocks, rgb.ctypes.data)),
        ("null", (C.byref(frame), None, blocks, rgb.ctypes.data)),
        ("null", (C.byref(frame), zeros.ctypes.data, blocks, None)),
        ("nbBlocks", (C.byref(frame), zeros.ctypes.data, blocks + 1, rgb.ctypes.data)),
        ("nbBlocks", (C.byref(frame), zeros.ctypes.data, 0, rgb.ctypes.data)),
        ("sampling", (C.byref(tall), tall_zeros.ctypes.data, tall_blocks, rgb.ctypes.data)),
    ]
    for word, args in cases:
        assert hip.solr_hip_jpeg_to_rgb(*args) == -1
        code, text = last_error(hip)
        assert code == -1 and "solr_hip_jpeg_to_rgb" in text and word in text, text
        assert (rgb == 7).all() and hip.solr_hip_jpeg_blocks() == produced     # nothing ran
        hip.solr_hip_clear_error()
    # all coefficients zero: Y = Cb = Cr = 128, which is mid-grey
    assert hip.solr_hip_jpeg_to_rgb(C.byref(frame), zeros.ctypes.data, blocks, rgb.ctypes.data) == 0
    assert (rgb == 128).all() and hip.solr_hip_jpeg_blocks() == produced + 3
    # ... and the engine still renders
    k = solr.Kernel(engine="hip")
    solr.scenes.cornell(k, width=32, height=24, iterations=1)
    k.render()
    k.check(0, "a frame after refused calls")
    k.finalize()
