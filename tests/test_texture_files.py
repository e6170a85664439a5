"""Texture files on the host-only engine: SolR_LoadTextureFromFile (GPUKernel::loadTextureFromFile, host/ImageLoader.*)
against the reference's own decoders.

tests/golden/texture_files.npz holds, per file of tests/golden/textures/, what the reference's jpgd / tgad produce for it
(tests/golden/make_texture_fixtures.py; BMP: derived from the file's bytes).  The arithmetic is all integer, so the bar
is the project's usual one: every byte equal - no tolerance, no excluded pixels.  The JPEG pixel stage runs on the CPU
here (csrc/jpeg_pixels.h in a loop); tests/test_texture_files_gpu.py holds the kernel to the same arrays."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TEXTURES = os.path.join(HERE, "golden", "textures")
EXPECTED = np.load(os.path.join(HERE, "golden", "texture_files.npz"))
ACCEPTED = sorted(EXPECTED.files)
REFUSED = ["progressive_24x24.jpg", "gray_19x13.jpg"]
TEXTURE_NONE = -1
# enum TextureType (include/solr_types.h)
DIFFUSE, BUMP, NORMAL, AMBIENT_OCCLUSION, REFLECTIVE, SPECULAR, TRANSPARENT = range(7)


def test_the_fixture_set_is_the_one_the_loader_is_specified_on():
    assert ACCEPTED == sorted(["444_24x17.jpg", "444_16x16_q100.jpg", "444_8x8_flat.jpg", "422_33x9.jpg",
                               "420_37x21.jpg", "420_31x31_optimized.jpg", "420_40x40_restart2.jpg", "0220r.jpg",
                               "0100d.jpg", "rgb_6x5.bmp", "rgb_8x4.bmp", "raw24_7x5.tga", "rle24_7x5.tga",
                               "rle32_9x3.tga"])
    for name in ACCEPTED + REFUSED:
        assert os.path.exists(os.path.join(TEXTURES, name)), name
    assert EXPECTED["0100d.jpg"].shape == (512, 512, 3) and EXPECTED["0220r.jpg"].shape == (512, 512, 3)
    assert EXPECTED["rle32_9x3.tga"].shape == (3, 9, 4)
    # the q100 file is there for the clamps at both ends
    assert EXPECTED["444_16x16_q100.jpg"].min() == 0 and EXPECTED["444_16x16_q100.jpg"].max() == 255
    restart = open(os.path.join(TEXTURES, "420_40x40_restart2.jpg"), "rb").read()
    assert b"\xff\xdd\x00\x04\x00\x02" in restart, "no restart interval of 2 MCUs in the restart fixture"


def fresh(solr):
    k = solr.Kernel(engine="host-only")
    assert nb_textures(k) == 0
    return k


def nb_textures(k):
    n = C.c_int(-1)
    assert k.L.SolR_GetNbTextures(C.byref(n)) == 0
    return n.value


def texture_size(k, slot):
    w, h, d = C.c_int(), C.c_int(), C.c_int()
    assert k.L.SolR_GetTextureSize(slot, C.byref(w), C.byref(h), C.byref(d)) == 0
    return w.value, h.value, d.value


def get_texture(k, slot, shape):
    """SolR_GetTexture hands the pixels out with the first and third channel swapped and leaves a fourth byte alone
    (SolRStub.cpp:351-373 of the reference)"""
    out = np.full(shape, 0xEE, np.uint8)
    assert k.L.SolR_GetTexture(slot, out.ctypes.data) == 0
    return out


def expected_from_get_texture(e):
    swapped = e.copy()
    swapped[..., 0], swapped[..., 2] = e[..., 2], e[..., 0]
    if e.shape[2] == 4:
        swapped[..., 3] = 0xEE
    return swapped


@pytest.mark.parametrize("name", ACCEPTED)
def test_an_accepted_file_loads_to_the_reference_decoders_bytes(solr, name):
    k = fresh(solr)
    e = EXPECTED[name]
    assert k.L.SolR_LoadTextureFromFile(0, os.fsencode(os.path.join(TEXTURES, name))) == 1
    assert nb_textures(k) == 1
    assert texture_size(k, 0) == (e.shape[1], e.shape[0], e.shape[2])
    assert np.array_equal(get_texture(k, 0, e.shape), expected_from_get_texture(e))
    # the bytes themselves, as the device layer is handed them
    atlas = k.flat_scene().textures
    assert atlas.size == e.size and np.array_equal(atlas.reshape(e.shape), e), \
        "%d of %d bytes differ from the reference decoder" % ((atlas.reshape(e.shape) != e).sum(), e.size)
    # (0220r.jpg is a reflection map by its name; type_by_the_rule is below)
    assert k.L.SolRx_GetTextureType(0) == type_by_the_rule(os.path.join(TEXTURES, name))
    assert type_by_the_rule("0220r.jpg") == REFLECTIVE and type_by_the_rule("0100d.jpg") == DIFFUSE


def test_slots_count_up_and_the_atlas_keeps_every_file(solr):
    k = fresh(solr)
    for slot, name in enumerate(ACCEPTED):
        assert k.load_texture(slot, os.path.join(TEXTURES, name)) is True
        assert nb_textures(k) == slot + 1
    atlas = k.flat_scene().textures
    assert np.array_equal(atlas, np.concatenate([EXPECTED[name].ravel() for name in ACCEPTED]))


def type_by_the_rule(path):
    """GPUKernel.cpp:2136-2148 of the reference: substrings of the whole name, the last match winning"""
    kind = DIFFUSE
    for mark, value in (("b.", BUMP), ("n.", NORMAL), ("a.", AMBIENT_OCCLUSION), ("r.", REFLECTIVE), ("s.", SPECULAR),
                        ("t.", TRANSPARENT)):
        if mark in path:
            kind = value
    return kind


@pytest.mark.parametrize("name, kind", [("xd.jpg", DIFFUSE), ("xb.jpg", BUMP), ("xn.jpg", NORMAL),
                                        ("xa.jpg", AMBIENT_OCCLUSION), ("xr.jpg", REFLECTIVE), ("xs.jpg", SPECULAR),
                                        ("xt.jpg", TRANSPARENT), ("xb.n.jpg", NORMAL), ("xt.b.jpg", TRANSPARENT),
                                        ("xs.tga", SPECULAR), ("xr.bmp", REFLECTIVE)])
def test_the_texture_type_follows_the_file_name(solr, tmp_path, name, kind):
    source = {"jpg": "444_8x8_flat.jpg", "tga": "raw24_7x5.tga", "bmp": "rgb_8x4.bmp"}[name[-3:]]
    path = str(tmp_path / name)
    shutil.copyfile(os.path.join(TEXTURES, source), path)
    if type_by_the_rule(str(tmp_path) + "/") == DIFFUSE:   # (a folder name with a mark in it would win or lose by the same rule)
        assert type_by_the_rule(path) == kind
    k = fresh(solr)
    assert k.load_texture(0, path)
    assert k.L.SolRx_GetTextureType(0) == type_by_the_rule(path)
    assert np.array_equal(k.flat_scene().textures, EXPECTED[source].ravel())


def slot_state(k, slot, shape):
    pixels = np.full(shape, 0xEE, np.uint8)
    status = k.L.SolR_GetTexture(slot, pixels.ctypes.data)      # 1 and nothing written for a slot beyond the count
    return nb_textures(k), texture_size(k, slot), status, pixels.tobytes(), k.L.SolRx_GetTextureType(slot)


def assert_refused(k, path):
    """0, and slot 0 (holding the flat fixture), slot 1 (empty) and the count as they were"""
    e = EXPECTED["444_8x8_flat.jpg"]
    before = slot_state(k, 0, e.shape), slot_state(k, 1, e.shape)
    assert k.L.SolR_LoadTextureFromFile(0, os.fsencode(path)) == 0
    assert k.L.SolR_LoadTextureFromFile(1, os.fsencode(path)) == 0
    assert (slot_state(k, 0, e.shape), slot_state(k, 1, e.shape)) == before
    assert np.array_equal(k.flat_scene().textures, e.ravel())


@pytest.fixture
def loaded(solr):
    k = fresh(solr)
    assert k.load_texture(0, os.path.join(TEXTURES, "444_8x8_flat.jpg"))
    return k


@pytest.mark.parametrize("name", REFUSED)
def test_a_refused_file_leaves_the_slot_and_the_count_alone(loaded, name, capfd):
    assert_refused(loaded, os.path.join(TEXTURES, name))
    err = capfd.readouterr().err
    assert name in err and ("progressive" in err if name.startswith("progressive") else "one-component" in err)


def test_names_that_are_not_files_or_not_images(loaded, tmp_path):
    assert loaded.L.SolR_LoadTextureFromFile(1, b"") == 0
    assert loaded.L.SolR_LoadTextureFromFile(1, None) == 0
    assert_refused(loaded, str(tmp_path / "missing.jpg"))
    other = str(tmp_path / "picture.png")
    shutil.copyfile(os.path.join(TEXTURES, "444_8x8_flat.jpg"), other)
    assert_refused(loaded, other)                         # the format goes by the name
    assert loaded.L.SolR_LoadTextureFromFile(-1, os.fsencode(os.path.join(TEXTURES, "444_8x8_flat.jpg"))) == 0
    assert loaded.L.SolR_LoadTextureFromFile(1 << 20, os.fsencode(os.path.join(TEXTURES, "444_8x8_flat.jpg"))) == 0
    assert nb_textures(loaded) == 1


@pytest.mark.parametrize("name", ["444_24x17.jpg", "420_40x40_restart2.jpg", "rle24_7x5.tga", "raw24_7x5.tga",
                                  "rgb_6x5.bmp"])
def test_truncated_files_are_refused(loaded, tmp_path, name):
    data = open(os.path.join(TEXTURES, name), "rb").read()
    # nothing, inside the headers, inside the tables, and at three places of the pixel / entropy-coded data (the last
    # one ten bytes short of the end, where a JPEG file still lacks the end of its last MCUs)
    for cut in sorted({0, 1, 3, 11, 17, 40, 200, len(data) // 3, len(data) // 2, 3 * len(data) // 4, len(data) - 10}):
        if 0 <= cut < len(data) - 2:
            path = str(tmp_path / ("cut%d_%s" % (cut, name[-4:])))
            open(path, "wb").write(data[:cut])
            assert_refused(loaded, path)


def segments(data):
    """(marker, offset of the segment's payload, payload length) up to the start of the scan"""
    pos, out = 2, []
    while True:
        assert data[pos] == 0xFF
        marker, length = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        out.append((marker, pos + 4, length - 2))
        if marker == 0xDA:
            return out
        pos += 2 + length


def test_corrupt_jpeg_files_are_refused(loaded, tmp_path):
    data = bytearray(open(os.path.join(TEXTURES, "444_24x17.jpg"), "rb").read())
    seg = segments(data)
    dht = [s for s in seg if s[0] == 0xC4][0]
    dqt = [s for s in seg if s[0] == 0xDB][0]
    sof = [s for s in seg if s[0] == 0xC0][0]
    sos = [s for s in seg if s[0] == 0xDA][0]

    def variant(tag, edit):
        d = bytearray(data)
        edit(d)
        path = str(tmp_path / (tag + ".jpg"))
        open(path, "wb").write(d)
        return path

    def many_codes(d):            # three codes of one bit: more than there can be
        d[dht[1] + 1] = 3

    def counts_past_the_segment(d):
        for i in range(1, 17):
            d[dht[1] + i] = 255

    def table_number(d):
        d[dht[1]] = 0x07

    def wide_quantisers(d):       # 16-bit tables
        d[dqt[1]] = 0x10

    def twelve_bits(d):
        d[sof[1]] = 12

    def no_size(d):
        d[sof[1] + 1:sof[1] + 5] = b"\0\0\0\0"

    def tall_luma(d):             # 1x2
        d[sof[1] + 7] = 0x12

    def one_component_scan(d):
        d[sos[1]] = 1

    def undefined_table(d):
        d[sos[1] + 2] = 0x33

    def segment_past_the_end(d):
        d[dht[1] - 2:dht[1]] = b"\xff\xff"

    def marker_in_the_scan(d):    # an end-of-image marker where the second MCU row's bits should be
        at = sos[1] + sos[2] + (len(d) - sos[1] - sos[2]) // 2
        d[at:at + 2] = b"\xff\xd9"

    for edit in (many_codes, counts_past_the_segment, table_number, wide_quantisers, twelve_bits, no_size, tall_luma,
                 one_component_scan, undefined_table, segment_past_the_end, marker_in_the_scan):
        assert_refused(loaded, variant(edit.__name__, edit))
    empty = str(tmp_path / "empty.jpg")
    open(empty, "wb").close()
    assert_refused(loaded, empty)
    for ext in (".tga", ".bmp"):
        empty = str(tmp_path / ("empty" + ext))
        open(empty, "wb").close()
        assert_refused(loaded, empty)


def test_bad_tga_and_bmp_headers_are_refused(loaded, tmp_path):
    tga = bytearray(open(os.path.join(TEXTURES, "rle24_7x5.tga"), "rb").read())
    bmp = bytearray(open(os.path.join(TEXTURES, "rgb_6x5.bmp"), "rb").read())

    def write(name, d):
        path = str(tmp_path / name)
        open(path, "wb").write(d)
        return path

    d = bytearray(tga); d[2] = 1                       # colour-mapped
    assert_refused(loaded, write("mapped.tga", d))
    d = bytearray(tga); d[16] = 16                     # 16 bits a pixel
    assert_refused(loaded, write("bits16.tga", d))
    d = bytearray(tga); d[18] = 0xFF                   # a run of 128 pixels in an image of 35
    assert_refused(loaded, write("long_run.tga", d))
    d = bytearray(bmp); d[28] = 32                     # 32 bits a pixel
    assert_refused(loaded, write("bits32.bmp", d))
    d = bytearray(bmp); d[30] = 1                      # run-length compressed
    assert_refused(loaded, write("rle.bmp", d))
    d = bytearray(bmp); d[10:14] = (1 << 20).to_bytes(4, "little")   # pixel data said to begin past the end
    assert_refused(loaded, write("offset.bmp", d))
    d = bytearray(bmp); d[22:26] = (5000).to_bytes(4, "little")      # taller than the file has rows for
    assert_refused(loaded, write("tall.bmp", d))
    d = bytearray(bmp); d[0] = ord("X")
    assert_refused(loaded, write("id.bmp", d))


def test_the_device_entry_point_checks_its_arguments_before_it_touches_a_device(solr):
    """solr_hip_jpeg_to_rgb (include/solr_hip.h): -1 and a message, the library's convention; needs no GPU"""
    hip = solr.hip_lib()
    hip.solr_hip_clear_error()
    frame = solr.JpegFrame()
    frame.width = frame.height = 8
    frame.lumaH = frame.lumaV = frame.mcusPerRow = frame.mcuRows = 1
    zeros, rgb = np.zeros((3, 64), np.int16), np.full((8, 8, 3), 7, np.uint8)
    huge = solr.JpegFrame()
    huge.width, huge.height, huge.lumaH, huge.lumaV, huge.mcusPerRow, huge.mcuRows = 1 << 20, 8, 1, 1, 1 << 17, 1
    for word, args in [("null", (None, zeros.ctypes.data, 3, rgb.ctypes.data)),
                       ("null", (C.byref(frame), None, 3, rgb.ctypes.data)),
                       ("null", (C.byref(frame), zeros.ctypes.data, 3, None)),
                       ("nbBlocks", (C.byref(frame), zeros.ctypes.data, 4, rgb.ctypes.data)),
                       ("size", (C.byref(huge), zeros.ctypes.data, 3 << 17, rgb.ctypes.data))]:
        assert hip.solr_hip_jpeg_to_rgb(*args) == -1
        buf = C.create_string_buffer(512)
        assert hip.solr_hip_last_error(buf, 512) == -1
        assert "solr_hip_jpeg_to_rgb" in buf.value.decode() and word in buf.value.decode()
        hip.solr_hip_clear_error()
    frame.lumaV = frame.mcuRows = 2           # 1x2: not among the samplings the stage implements
    frame.mcuRows = 1
    assert hip.solr_hip_jpeg_to_rgb(C.byref(frame), zeros.ctypes.data, 4, rgb.ctypes.data) == -1
    buf = C.create_string_buffer(512)
    assert hip.solr_hip_last_error(buf, 512) == -1 and "sampling" in buf.value.decode()
    hip.solr_hip_clear_error()
    assert (rgb == 7).all() and hip.solr_hip_last_error(None, 0) == 0


# ---- the OBJ reader's map_Kd (reference: OBJReader.cpp:243-299) -------------------------------------------
QUAD = os.path.join(TEXTURES, "quad.obj")


def test_an_obj_model_brings_its_texture(solr):
    k = solr.Kernel(engine="host-only")
    solr.scenes.obj_model(k, QUAD, width=64, height=48)
    e = EXPECTED["444_24x17.jpg"]
    assert nb_textures(k) == 1 and texture_size(k, 0) == (24, 17, 3)
    diffuse = C.c_int(-7)
    args = [0] + [None] * 11 + [C.byref(diffuse)] + [None] * 13
    assert k.L.SolR_GetMaterial(*args) == 0
    assert diffuse.value == 0
    flat = k.flat_scene()
    m = flat.materials[0]
    assert m["textureIds"][0] == 0 and list(m["textureMapping"]) == [24, 17, TEXTURE_NONE, 3]
    assert m["textureOffset"][0] == 0
    assert np.array_equal(flat.textures.reshape(e.shape), e)
    triangles = flat.primitives[flat.primitives["materialId"] == 0]
    assert len(triangles) == 2 and {tuple(t) for t in triangles["vt0"]} | {tuple(t) for t in triangles["vt1"]} \
        | {tuple(t) for t in triangles["vt2"]} == {(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)}


def test_an_obj_model_whose_image_is_missing_still_loads(solr, tmp_path, capfd):
    for name in ("quad.obj", "quad.mtl"):
        shutil.copyfile(os.path.join(TEXTURES, name), str(tmp_path / name))
    k = solr.Kernel(engine="host-only")
    solr.scenes.obj_model(k, str(tmp_path / "quad.obj"), width=64, height=48)
    assert "444_24x17.jpg" in capfd.readouterr().err
    assert nb_textures(k) == 0
    flat = k.flat_scene()
    assert flat.materials[0]["textureIds"][0] == TEXTURE_NONE
    assert (flat.primitives["materialId"] == 0).sum() == 2
    assert flat.textures.size == 0
