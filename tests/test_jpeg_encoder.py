"""The JPEG screenshot writer on the host-only engine: csrc/jpeg_encode.h in a loop for the pixel stage
(GPUKernel::jpegCoefficients), host/JpegWriter.cpp for the entropy stage, SolR_GenerateScreenshot on top.

tests/golden/make_jpeg_encoder_fixtures.py ran the reference's own encoder, solr/images/jpge.cpp, on small pictures chosen
for the paths they reach - one-pixel pictures, one column or one row into a second MCU, 256 MCUs in a row and in a column,
full-range noise, ramps, constant pictures (every block only an end-of-block), checkerboards of 0 / 255 (the largest AC,
alternating DC), pure red, green and blue (the chroma clamp), a last column and row that differ sharply (the edge rule),
the three samplings, qualities 1, 49, 50, 85 and 100, and the turned / red-blue-swapped reading of a screenshot - and keeps
in tests/golden/jpeg_encoder.npz the pictures, jpge's files and the coefficient blocks those files carry (the generator
proves that they are jpge's: an int64 model of the pixel stage followed by a baseline coder reproduces every file).

Every comparison is of every byte: no tolerance, no excluded case.  tests/test_jpeg_encoder_gpu.py holds the kernel and the
HIP engine's screenshots to the same arrays; the host-only engine renders nothing, so here SolR_GenerateScreenshot is only
held to its signature, its return value and to leaving no file and the scene settings alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURES = np.load(os.path.join(HERE, "golden", "jpeg_encoder.npz"))
NAMES = sorted(key[len("file/"):] for key in FIXTURES.files if key.startswith("file/"))


def case(name):
    """pixels (H, W, 3), width, height, (luma H, luma V), quality, turned, swapRedBlue, jpge's file, jpge's blocks"""
    width, height, h, v, quality, turned, swap = (int(x) for x in FIXTURES["params/" + name])
    pixels = FIXTURES["pixels/" + name.split("__")[0]]
    assert pixels.shape == (height, width, 3)
    return pixels, width, height, (h, v), quality, turned, swap, FIXTURES["file/" + name].tobytes(), \
        FIXTURES["blocks/" + name]


def headers_end(data):
    """the offset just behind the SOS segment: where the entropy-coded bytes begin"""
    at = data.find(b"\xff\xda")
    return len(data) if at < 0 else at + 2 + int.from_bytes(data[at + 2:at + 4], "big")


def assert_same_file(got, want, what):
    if got == want:
        return
    end = headers_end(want)
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    raise AssertionError("%s: the file differs from jpge's (%d bytes against %d): the headers up to SOS %s, first "
                         "difference at offset %d (the scan begins at %d)" % (
                             what, len(got), len(want), "agree" if got[:end] == want[:end] else "DIFFER", first, end))


def reordered(pixels, turned, swap):
    """what a screenshot hands the encoder: destination pixel p takes source pixel N - p (N itself clamped to N - 1),
    first and third channel swapped unless the frame buffer is ftRGB"""
    height, width, _ = pixels.shape
    flat = pixels.reshape(-1, 3)
    if turned:
        n = len(flat)
        flat = flat[np.minimum(n - np.arange(n), n - 1)]
    if swap:
        flat = flat[:, ::-1]
    return np.ascontiguousarray(flat.reshape(height, width, 3))


def coefficients_of(k, name):
    pixels, width, height, (h, v), quality, turned, swap, _, blocks = case(name)
    got = np.full(blocks.shape, 0x5A5A, np.int16)
    pixels = np.ascontiguousarray(pixels)
    assert k.L.SolRx_JpegCoefficients(pixels.ctypes.data, width, height, quality, h, v, turned, swap, got.ctypes.data,
                                      len(got)) == 0
    return got


def assert_same_blocks(got, want, name):
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    raise AssertionError("%s: %d of %d coefficients differ from jpge's, first at (block, zigzag position) %s: %s against "
                         "%s" % (name, len(bad), want.size, bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.fixture(scope="module")
def host(solr):
    k = solr.Kernel(engine="host-only")
    yield k
    k.finalize()


def test_the_fixture_set_is_the_one_the_issue_asks_for():
    sizes, contents, samplings, qualities = set(), set(), set(), set()
    at_85_420 = set()
    for name in NAMES:
        picture, rest = name.split("__")
        content, size = picture.rsplit("_", 1)
        s, q = rest.split("_")[:2]
        sizes.add(size), contents.add(content), samplings.add(s), qualities.add(q)
        if (s, q) == ("420", "q85"):
            at_85_420.update((size, content))
    assert sizes == {"1x1", "4x1", "17x16", "16x17", "37x21", "40x40", "4096x1", "2x4096"}
    assert contents == {"noise", "ramp", "constant", "checker1", "checker8", "red", "green", "blue", "edge"}
    assert samplings == {"444", "422", "420"} and qualities == {"q1", "q49", "q50", "q85", "q100"}
    assert at_85_420 == sizes | contents
    assert any(n.endswith("_turned") for n in NAMES) and any(n.endswith("_turned_bgr") for n in NAMES)
    assert os.path.getsize(os.path.join(HERE, "golden", "jpeg_encoder.npz")) <= \
        os.path.getsize(os.path.join(HERE, "golden", "jpeg_synthetic.npz")) <= 256 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_encode_jpeg_writes_jpges_bytes(host, tmp_path, name):
    pixels, _, _, sampling, quality, turned, swap, want, _ = case(name)
    path = str(tmp_path / "out.jpg")
    host.encode_jpeg(path, pixels, quality=quality, sampling=sampling, turned=bool(turned), swap_red_blue=bool(swap))
    assert_same_file(open(path, "rb").read(), want, name)


@pytest.mark.parametrize("name", NAMES)
def test_the_host_loop_gives_jpges_blocks(host, name):
    assert_same_blocks(coefficients_of(host, name), case(name)[8], name)


@pytest.mark.parametrize("name", NAMES)
def test_the_writer_alone_gives_jpges_file(host, tmp_path, name):
    _, width, height, (h, v), quality, _, _, want, blocks = case(name)
    path = str(tmp_path / "out.jpg")
    blocks = np.ascontiguousarray(blocks)
    assert host.L.SolRx_JpegFromCoefficients(os.fsencode(path), blocks.ctypes.data, len(blocks), width, height, quality,
                                             h, v) == 0
    assert_same_file(open(path, "rb").read(), want, name)


def test_the_turned_fixtures_are_the_plain_encoding_of_the_reordered_pixels(host, tmp_path):
    """the two flags against numpy: encoding with turned / swap_red_blue is encoding the reordered picture without"""
    for name in NAMES:
        pixels, _, _, sampling, quality, turned, swap, want, _ = case(name)
        if not (turned or swap):
            continue
        path = str(tmp_path / "out.jpg")
        host.encode_jpeg(path, reordered(pixels, turned, swap), quality=quality, sampling=sampling)
        assert_same_file(open(path, "rb").read(), want, name + " (reordered in numpy)")


def test_quantisation_by_multiplication_is_exact(host):
    """jpe::quantise divides by multiplying with a reciprocal: every quantiser 1 ... 255 and every magnitude the DCT can
    produce, 0 ... 16 384 + 127 once q >> 1 is added, both signs, against plain integer division"""
    top = 16384 + 127
    for q in range(1, 256):
        count = top - (q >> 1) + 1                 # |value| + (q >> 1) runs up to 16 511
        values = np.arange(count, dtype=np.int64)
        magnitude = values + (q >> 1)
        assert magnitude[-1] == top
        want = np.where(magnitude < q, 0, magnitude // q)
        for negative in (0, 1):
            got = np.full(count, 0x5A5A, np.int16)
            assert host.L.SolRx_JpegQuantise(q, 0, count, negative, got.ctypes.data) == 0
            assert np.array_equal(got, -want if negative else want), (q, negative)
    out = np.zeros(4, np.int16)
    assert host.L.SolRx_JpegQuantise(0, 0, 1, 0, out.ctypes.data) == -1
    assert host.L.SolRx_JpegQuantise(256, 0, 1, 0, out.ctypes.data) == -1
    assert host.L.SolRx_JpegQuantise(1, top, 2, 0, out.ctypes.data) == -1


BAD_ARGUMENTS = [dict(quality=0), dict(quality=101), dict(quality=-3), dict(sampling=(1, 2)), dict(sampling=(3, 1)),
                 dict(sampling=(0, 0)), dict(width=0), dict(height=0), dict(width=-1), dict(width=16385),
                 dict(height=16385), dict(width=16384, height=8192)]


@pytest.mark.parametrize("bad", BAD_ARGUMENTS, ids=lambda b: "_".join("%s=%s" % kv for kv in b.items()))
def test_bad_arguments_return_minus_one_and_write_nothing(host, tmp_path, bad):
    pixels = np.zeros((8, 8, 3), np.uint8)            # (never read: the sizes are refused first)
    a = dict(width=8, height=8, quality=85, sampling=(2, 2))
    a.update(bad)
    path = str(tmp_path / "out.jpg")
    assert host.L.SolRx_EncodeJpeg(os.fsencode(path), pixels.ctypes.data, a["width"], a["height"], a["quality"],
                                   a["sampling"][0], a["sampling"][1], 0, 0) == -1
    assert not os.path.exists(path)


def test_null_arguments_and_unwritable_paths(host, tmp_path):
    pixels = np.zeros((8, 8, 3), np.uint8)
    assert host.L.SolRx_EncodeJpeg(None, pixels.ctypes.data, 8, 8, 85, 2, 2, 0, 0) == -1
    assert host.L.SolRx_EncodeJpeg(os.fsencode(str(tmp_path / "out.jpg")), None, 8, 8, 85, 2, 2, 0, 0) == -1
    assert host.L.SolRx_EncodeJpeg(os.fsencode(str(tmp_path / "no" / "such" / "out.jpg")), pixels.ctypes.data, 8, 8, 85,
                                   2, 2, 0, 0) == -1
    assert not list(tmp_path.iterdir())


def test_generate_screenshot_has_the_references_signature():
    """SolR_GenerateScreenshot(char *filename, int width, int height, int quality) returning int: solr/SolRStub.h:62 of
    the reference, restated here so that the test needs no other tree"""
    text = open(os.path.join(ROOT, "sol-r_amd", "host", "SolRStub.h")).read()
    found = re.search(r"\bint\s+SolR_GenerateScreenshot\s*\(([^)]*)\)\s*;", text)
    assert found, "SolRStub.h does not declare SolR_GenerateScreenshot"
    parameters = [re.sub(r"\s+", " ", p.strip()) for p in found.group(1).split(",")]
    assert parameters == ["char *filename", "int width", "int height", "int quality"]


def test_generate_screenshot_returns_zero_and_an_engine_that_cannot_render_writes_nothing(solr, tmp_path):
    """the reference's call returns 0 whatever happens; the host-only engine fails every pass, so no file appears, the
    failure is on record, and the scene settings are the ones from before the call"""
    k = solr.Kernel(engine="host-only")
    solr.scenes.cornell(k, width=40, height=24, iterations=2)
    before = k.frame_parameters()[0]
    path = str(tmp_path / "shot.jpg")
    assert k.L.SolR_GenerateScreenshot(os.fsencode(path), 37, 21, 3) == 0
    assert not os.path.exists(path)
    assert k.L.SolRx_LastError(None, 0) != 0
    with pytest.raises(solr.SolrError):
        k.screenshot(path, 37, 21, 1)
    assert not os.path.exists(path)
    after = k.frame_parameters()[0]
    assert bytes(before) == bytes(after)
    k.finalize()
