"""The JPEG loader on files written from synthesised coefficient blocks, host-only engine: SolR_LoadTextureFromFile
(host/ImageLoader.cpp for the Huffman stage, csrc/jpeg_pixels.h in a loop for the pixels).

tests/golden/make_jpeg_synthetic_fixtures.py writes tests/golden/textures/synthetic/*.jpg with a small baseline JPEG
writer of its own, from blocks chosen for the paths they reach - every last zigzag position in Y, Cb and Cr (jpgd's
Row<N>, Col<N> and the fifteen P_Q / R_S instantiations), coefficients of +-1023 (the clamps, the largest sums that still
fit), widths with and without the dword store path, pictures of one pixel, 512 MCUs in a row and 256 in a column, ZRL
runs to coefficient 63, blocks without an end-of-block code, DC differences of category 11, restart markers past RST7,
stuffed 0xFF bytes - and keeps in tests/golden/jpeg_synthetic.npz what the reference's jpgd decodes them to.

Two tiers.  EXACT: jpgd built with -fsanitize=signed-integer-overflow reports nothing and an int64 model of the general
transforms keeps every sum within int32 and every 16-bit store untruncated; the loader must give jpgd's bytes
(`expected/`), every one - no tolerance, no excluded pixels.  WRAP (wrap_*): sums pass 32 bits; the loader must give
`wrapped/`, the model's bytes with the engine's documented semantics (sums modulo 2^32, 16-bit stores as casts), again
every byte; `jpgd/` is kept for information ("Texture files").  tests/test_jpeg_synthetic_gpu.py holds the
kernel to the same arrays."""
import ctypes as C
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SYNTHETIC = os.path.join(HERE, "golden", "textures", "synthetic")
FIXTURES = np.load(os.path.join(HERE, "golden", "jpeg_synthetic.npz"))
NAMES = sorted(key[len("frame/"):] for key in FIXTURES.files if key.startswith("frame/"))
EXACT = sorted(key[len("expected/"):] for key in FIXTURES.files if key.startswith("expected/"))
WRAP = sorted(key[len("wrapped/"):] for key in FIXTURES.files if key.startswith("wrapped/"))
SAMPLINGS = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}
TINY = ["tiny_%s_%s" % (s, size) for s in SAMPLINGS for size in ("1x1", "3x1", "4x1", "5x3")]
# the files whose blocks are "moderate": they must leave nearly every decoded byte away from the clamps
MODERATE = sorted(["zag_444", "zag_422", "zag_420", "dwords_444", "dwords_422", "dwords_420", "pair_420_21x9",
                   "row_444_4096x1", "column_420_2x4096", "huffman_zrl_to_63_16x8", "huffman_no_eob_16x8",
                   "huffman_zrl_then_eob_16x8", "huffman_restart_444_32x24", "huffman_restart_420_40x56"] + TINY)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def path_of(name):
    return os.path.join(SYNTHETIC, name + ".jpg")


def frame_of(name):
    """width, height, (luma H, luma V), the three quantisation tables (3, 64)"""
    f = FIXTURES["frame/" + name]
    return int(f[0]), int(f[1]), (int(f[2]), int(f[3])), f[4:].reshape(3, 64)


def bytes_the_loader_owes(name):
    return FIXTURES[("expected/" if name in EXACT else "wrapped/") + name]


def components(name):
    """the blocks of coefficients/<name> by component: Y, Cb, Cr"""
    _, _, (h, v), _ = frame_of(name)
    blocks = FIXTURES["coefficients/" + name]
    per_mcu = h * v + 2
    index = np.arange(len(blocks)) % per_mcu
    return blocks[index < h * v], blocks[index == h * v], blocks[index == h * v + 1]


def last_positions(blocks):
    """the last non-zero zigzag position of every block (0: nothing beyond the DC coefficient)"""
    nonzero = blocks[:, ZIGZAG] != 0
    nonzero[:, 0] = True
    return 63 - np.argmax(nonzero[:, ::-1], axis=1)


def entropy_coded(name):
    """the bytes between the scan header and the end-of-image marker"""
    d = open(path_of(name), "rb").read()
    pos = 2
    while d[pos + 1] != 0xDA:
        pos += 2 + int.from_bytes(d[pos + 2:pos + 4], "big")
    assert d[-2:] == b"\xff\xd9"
    return d[pos + 2 + int.from_bytes(d[pos + 2:pos + 4], "big"):-2]


def test_the_fixture_set_and_its_tiers():
    assert EXACT == sorted(["zag_444", "zag_422", "zag_420", "full_444", "full_422", "full_420", "dwords_444",
                            "dwords_422", "dwords_420", "pair_420_21x9", "row_444_4096x1", "column_420_2x4096",
                            "huffman_zrl_to_63_16x8", "huffman_no_eob_16x8", "huffman_zrl_then_eob_16x8",
                            "huffman_dc_category_11_24x24", "huffman_restart_444_32x24", "huffman_restart_420_40x56",
                            "huffman_stuffing_24x24"] + TINY)
    assert WRAP == ["wrap_420", "wrap_422", "wrap_444", "wrap_444_1x1"]
    assert NAMES == sorted(EXACT + WRAP)
    assert sorted(os.listdir(SYNTHETIC)) == [name + ".jpg" for name in NAMES]
    sizes = {"zag": ((67, 61), (139, 61), (139, 125)), "full": ((37, 39), (77, 39), (77, 79)),
             "dwords": ((20, 9), (36, 9), (36, 20)), "wrap": ((21, 13), (37, 13), (37, 21))}
    for family, three in sizes.items():
        for s, size in zip(("444", "422", "420"), three):
            assert frame_of("%s_%s" % (family, s))[:3] == size + (SAMPLINGS[s],)
    for name in TINY:
        s, size = name.split("_")[1:]
        assert frame_of(name)[:3] == tuple(int(n) for n in size.split("x")) + (SAMPLINGS[s],)
    assert frame_of("pair_420_21x9")[:3] == (21, 9, (2, 2))       # one workgroup of two MCUs, the byte store path
    assert frame_of("row_444_4096x1")[:3] == (4096, 1, (1, 1)) and frame_of("column_420_2x4096")[:3] == (2, 4096, (2, 2))
    total = os.path.getsize(os.path.join(HERE, "golden", "jpeg_synthetic.npz"))
    for name in NAMES:
        width, height, (h, v), quant = frame_of(name)
        assert bytes_the_loader_owes(name).shape == (height, width, 3) and bytes_the_loader_owes(name).dtype == np.uint8
        blocks = FIXTURES["coefficients/" + name]
        assert blocks.dtype == np.int16
        assert blocks.shape == (-(-width // (8 * h)) * -(-height // (8 * v)) * (h * v + 2), 64)
        assert np.abs(blocks).max() <= 1023 and quant.min() >= 1 and quant.max() <= 255
        assert os.path.getsize(path_of(name)) < 64 * 1024
        total += os.path.getsize(path_of(name))
    assert total < 420 * 1024
    # dwords_*: a width that takes the dword store path, is no multiple of the MCU's width, and an odd number of MCUs
    for name in ("dwords_444", "dwords_422", "dwords_420"):
        width, _, (h, _), _ = frame_of(name)
        assert width % 4 == 0 and width % (8 * h) != 0 and -(-width // (8 * h)) % 2 == 1
    # wrap tier: quantisers that push the sums beyond 32 bits; the 1x1 file is where jpgd's Col<1> parts from the
    # general column pass (kept for information: the loader is not held to `jpgd/`)
    for name in WRAP:
        assert FIXTURES["jpgd/" + name].shape == FIXTURES["wrapped/" + name].shape
    assert FIXTURES["jpgd/wrap_444_1x1"].tolist() == [[[76, 255, 28]]]
    assert FIXTURES["wrapped/wrap_444_1x1"].tolist() == [[[0, 48, 225]]]


@pytest.mark.parametrize("name", ["zag_444", "zag_422", "zag_420"])
def test_every_last_zigzag_position_occurs_in_every_component(name):
    for blocks in components(name):
        assert set(last_positions(blocks).tolist()) == set(range(64))
    # ... and in full_*, whose blocks are dense up to their last position
    for blocks in components(name.replace("zag", "full")):
        last = last_positions(blocks)
        assert len(set(last.tolist())) >= 15
        for block, position in zip(blocks, last):
            assert (block[ZIGZAG[1:position + 1]] != 0).all()


@pytest.mark.parametrize("name", MODERATE)
def test_moderate_files_stay_away_from_the_clamps(name):
    e = FIXTURES["expected/" + name]
    assert np.isin(e, (0, 255)).mean() <= 0.05
    _, _, _, quant = frame_of(name)
    assert quant.max() <= 3


def test_the_dense_files_reach_both_clamps():
    for s in SAMPLINGS:
        e = FIXTURES["expected/full_" + s]
        assert e.min() == 0 and e.max() == 255
        assert np.abs(FIXTURES["coefficients/full_" + s]).max() == 1023 and frame_of("full_" + s)[3].max() == 2


def test_what_the_huffman_files_hold():
    blocks = FIXTURES["coefficients/huffman_zrl_to_63_16x8"]
    assert (blocks[:, 63] != 0).all() and (blocks[:, 1:63] == 0).all()          # ZRL, ZRL, ZRL, then a run of 14
    assert (FIXTURES["coefficients/huffman_no_eob_16x8"][:, 1:] != 0).all()
    assert last_positions(FIXTURES["coefficients/huffman_zrl_then_eob_16x8"]).tolist() == [0, 1, 5, 20, 46, 47]
    for component in components("huffman_dc_category_11_24x24"):
        assert component[:, 0].tolist() == [-1023, 1023] * 4 + [-1023]           # differences of 2046: category 11
    for name, mcus in (("huffman_restart_444_32x24", 12), ("huffman_restart_420_40x56", 12)):
        data = open(path_of(name), "rb").read()
        assert b"\xff\xdd\x00\x04\x00\x01" in data, "no restart interval of 1 MCU"
        scan = entropy_coded(name)
        markers = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and scan[i + 1] != 0]
        assert markers == [0xD0 + i % 8 for i in range(mcus - 1)] and 0xD7 in markers[:-1]
    assert entropy_coded("huffman_stuffing_24x24").count(b"\xff\x00") >= 32


def nb_textures(k):
    n = C.c_int(-1)
    assert k.L.SolR_GetNbTextures(C.byref(n)) == 0
    return n.value


@pytest.mark.parametrize("name", NAMES)
def test_a_synthetic_file_loads_to_the_bytes_it_owes(solr, name):
    k = solr.Kernel(engine="host-only")
    assert nb_textures(k) == 0
    e = bytes_the_loader_owes(name)
    assert k.L.SolR_LoadTextureFromFile(0, os.fsencode(path_of(name))) == 1
    assert nb_textures(k) == 1
    w, h, d = C.c_int(), C.c_int(), C.c_int()
    assert k.L.SolR_GetTextureSize(0, C.byref(w), C.byref(h), C.byref(d)) == 0
    assert (w.value, h.value, d.value) == (e.shape[1], e.shape[0], 3)
    got = k.flat_scene().textures
    assert got.size == e.size
    got = got.reshape(e.shape)
    assert np.array_equal(got, e), "%d of %d bytes differ from %s, first at %s" % (
        (got != e).sum(), e.size, "jpgd" if name in EXACT else "the wrapped model", np.argwhere(got != e)[:4].tolist())
