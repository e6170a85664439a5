"""The optimised Huffman tables of the JPEG writer on the host (sol-r_amd/csrc/jpeg_entropy.h: blockCensus, optimiseTable;
host/JpegWriter.cpp: encode, header and scan in their optimised mode) - the reference encoder's two-pass mode,
solr/images/jpge.cpp with params::m_two_pass_flag.

Held to jpge's own tables and files (tests/golden/jpeg_two_pass.npz: optimize_huffman_table driven on chosen histograms,
and its two-pass file for each of the 90 cases of jpeg_encoder.npz) and to three things in tests/jpeg_two_pass_cases.py
that share nothing with the header: a census from the text of annex F, a reader that decodes a file with the file's own
DHT segments, and a restatement of the table builder whose wrong variants the fixtures must tell apart.  Every comparison
is of every byte.  With the option off nothing changes: tests/test_jpeg_entropy.py and tests/test_jpeg_encoder.py hold
that, unedited."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import jpeg_entropy_cases as JC
import jpeg_two_pass_cases as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FILES = T.file_names()
TABLES = T.table_names()
SYNTHETIC = JC.cases()


@pytest.fixture(scope="module")
def host(solr):
    k = solr.Kernel(engine="host-only")
    yield k
    k.finalize()


def optimise_table(k, counts):
    counts = np.ascontiguousarray(counts, np.uint32)
    bits = np.full(16, 0x5A, np.uint8)
    values = np.full(256, 0x5A, np.uint8)
    n = k.L.SolRx_JpegOptimiseTable(counts.ctypes.data, len(counts), bits.ctypes.data, values.ctypes.data)
    assert 0 <= n <= len(counts) and (values[n:] == 0x5A).all()
    return bits.tolist(), values[:n].tolist()


def host_census(k, blocks, luma_blocks):
    blocks = np.ascontiguousarray(blocks, np.int16)
    counts = np.full(536, 0x5A5A5A5A, np.uint32)
    assert k.L.SolRx_JpegCensus(blocks.ctypes.data, len(blocks), luma_blocks, counts.ctypes.data) == 0
    return counts


def test_the_fixtures_are_the_ones_the_issue_asks_for():
    one, _ = T.fixtures()
    assert len(FILES) == 90 and FILES == sorted(k[5:] for k in one.files if k.startswith("file/"))
    assert {"one_symbol_dc", "one_symbol_ac", "two_symbols", "dc_all_ones", "all_256_equal", "runs_of_ties", "limit_18",
            "limit_22", "powers_of_two_27", "random_dc", "random_sparse", "random_dense"} <= set(TABLES)
    assert {len(T.table(name)[0]) for name in TABLES} == {12, 256}
    assert T.table("one_symbol_ac")[1].tolist() == [1] + [0] * 15
    assert T.table("all_256_equal")[1].tolist() == [0] * 7 + [255, 1] + [0] * 7
    assert T.table("limit_18")[1].tolist() == [1] * 13 + [0, 2, 3] and int(T.table("limit_18")[0].sum()) == 10944
    assert T.table("limit_22")[1].tolist() == [1] * 12 + [0, 1, 2, 7]
    assert int(T.table("powers_of_two_27")[0].max()) > 1 << 24


@pytest.mark.parametrize("name", TABLES)
def test_the_table_builder_gives_jpges_table(host, name):
    counts, bits, values = T.table(name)
    assert optimise_table(host, counts) == (bits.tolist(), values.tolist())


def test_the_table_builder_refuses_bad_arguments(host):
    counts, bits, values = np.ones(12, np.uint32), np.zeros(16, np.uint8), np.zeros(256, np.uint8)
    call = host.L.SolRx_JpegOptimiseTable
    assert call(None, 12, bits.ctypes.data, values.ctypes.data) == -1
    assert call(counts.ctypes.data, 12, None, values.ctypes.data) == -1
    assert call(counts.ctypes.data, 12, bits.ctypes.data, None) == -1
    assert call(counts.ctypes.data, 0, bits.ctypes.data, values.ctypes.data) == -1
    assert call(counts.ctypes.data, 257, bits.ctypes.data, values.ctypes.data) == -1
    # no symbol at all: no code
    assert optimise_table(host, np.zeros(256, np.uint32)) == ([0] * 16, [])


@pytest.mark.parametrize("name", TABLES)
def test_the_python_restatement_gives_jpges_table_too(name):
    """(what the wrong variants below are variants OF)"""
    counts, bits, values = T.table(name)
    assert T.model_tables(counts) == (bits.tolist(), values.tolist())


@pytest.mark.parametrize("variant", T.VARIANTS)
def test_the_fixtures_tell_a_wrong_restatement_from_the_right_one(host, variant):
    """the builder with ONE statement restated wrongly differs, on at least one histogram of the table tier, from jpge's
    table - which the tests above hold the header's builder to"""
    caught = []
    for name in TABLES:
        counts, bits, values = T.table(name)
        if T.model_tables(counts, variant) != (bits.tolist(), values.tolist()):
            caught.append(name)
    assert caught, "no histogram tells '%s' from the right statement" % variant
    expected = {"ties_reversed": "runs_of_ties", "no_limit": "limit_18", "repair_wrong_length": "limit_repair_choice",
                "dummy_left_in": "one_symbol_dc", "dummy_from_shortest": "dc_all_twelve",
                "values_not_reversed": "two_symbols"}
    assert expected[variant] in caught, caught


@pytest.mark.parametrize("name", FILES)
def test_the_host_writer_gives_jpges_two_pass_file(host, tmp_path, name):
    width, height, sampling, quality, blocks, one, two = T.file_case(name)
    got = host.jpeg_from_coefficients(blocks, width, height, quality, sampling, optimise=True)
    assert got == two, "%s: %d bytes against jpge's %d (the decomposed route)" % (name, len(got), len(two))
    # the bit-buffer coder in its optimised mode (JpegWriter::encode): the same file by another loop
    path = str(tmp_path / "two_pass.jpg")
    assert host.L.SolRx_JpegFromCoefficientsOptimised(os.fsencode(path), blocks.ctypes.data, len(blocks), width, height,
                                                      quality, sampling[0], sampling[1]) == 0
    assert open(path, "rb").read() == two, name + " (JpegWriter::encode)"
    # and with the option off, the bytes of before
    assert host.jpeg_from_coefficients(blocks, width, height, quality, sampling) == one
    assert len(two) < len(one)


@pytest.mark.parametrize("name", FILES)
def test_a_reader_with_the_files_own_tables_gets_the_blocks_back(host, name):
    width, height, sampling, quality, blocks, _, two = T.file_case(name)
    got = host.jpeg_from_coefficients(blocks, width, height, quality, sampling, optimise=True)
    parsed = T.parse(got)
    assert parsed["dht_order"] == [(0, 0), (1, 0), (0, 1), (1, 1)] and (parsed["width"], parsed["height"]) == (width, height)
    assert np.array_equal(T.decode(got), blocks), name
    assert np.array_equal(T.decode(two), blocks), name + " (jpge's file)"
    # the tables in the file are the model's for the census of the blocks
    model = T.model_huffman(T.census(blocks, sampling[0] * sampling[1]))
    assert [parsed["tables"][key] for key in parsed["dht_order"]] == [(b, v) for b, v in model]


@pytest.mark.parametrize("name", [c["name"] for c in SYNTHETIC])
def test_the_synthetic_blocks_survive_the_optimised_route(host, name):
    c = SYNTHETIC[[s["name"] for s in SYNTHETIC].index(name)]
    got = host.jpeg_from_coefficients(c["blocks"], c["width"], c["height"], c["quality"], c["sampling"], optimise=True)
    assert np.array_equal(T.decode(got), c["blocks"]), name
    one = host.jpeg_from_coefficients(c["blocks"], c["width"], c["height"], c["quality"], c["sampling"])
    assert len(got) < len(one)


@pytest.mark.parametrize("name", FILES)
def test_the_census_is_the_numpy_census(host, name):
    _, _, sampling, _, blocks, _, _ = T.file_case(name)
    luma = sampling[0] * sampling[1]
    want = T.census(blocks, luma)
    assert int(want[:24].sum()) == len(blocks)
    assert np.array_equal(host_census(host, blocks, luma), want), name


def test_the_census_of_the_synthetic_blocks_and_of_blocks_outside_the_domain(host):
    for c in SYNTHETIC:
        luma = c["sampling"][0] * c["sampling"][1]
        assert np.array_equal(host_census(host, c["blocks"], luma), T.census(c["blocks"], luma)), c["name"]
    blocks = np.zeros((6, 64), np.int16)
    blocks[4, 7] = 1024
    counts = np.full(536, 0x5A5A5A5A, np.uint32)
    assert host.L.SolRx_JpegCensus(blocks.ctypes.data, 6, 1, counts.ctypes.data) == -1 and (counts == 0x5A5A5A5A).all()
    assert host.L.SolRx_JpegCensus(blocks.ctypes.data, 6, 3, counts.ctypes.data) == -1
    with pytest.raises(Exception):
        host.jpeg_from_coefficients(blocks, 16, 8, 85, (1, 1), optimise=True)


def test_the_limit_engages_in_a_file(host):
    """the 18-symbol histogram as blocks: the luma AC table of the file is the fixture's, with its 16-bit codes"""
    c = T.limit_18_case()
    counts, bits, values = T.table("limit_18")
    assert np.array_equal(T.census(c["blocks"], 4)[T.CENSUS_SLICES["ac_luma"]], counts)
    got = host.jpeg_from_coefficients(c["blocks"], c["width"], c["height"], c["quality"], c["sampling"], optimise=True)
    assert T.parse(got)["tables"][(1, 0)] == (bits.tolist(), values.tolist()) and bits[15] == 3
    assert np.array_equal(T.decode(got), c["blocks"])


def test_the_dense_group_holds_its_tables_longest_codes(host):
    c = T.rare_dense_case()
    got = host.jpeg_from_coefficients(c["blocks"], c["width"], c["height"], c["quality"], c["sampling"], optimise=True)
    for key in ((1, 0), (1, 1)):
        bits, values = T.parse(got)["tables"][key]
        assert sorted(values[-10:]) == list(range(1, 11)), "the (run 0, size s) symbols are not the ten rarest"
    assert np.array_equal(T.decode(got)[c["group"]:c["group"] + 64], c["blocks"][c["group"]:c["group"] + 64])


def test_encode_jpeg_optimised_is_the_two_pass_file_of_the_pixels(host, tmp_path):
    one, two = T.fixtures()
    for name in ("noise_37x21__420_q85", "ramp_40x40__420_q85_turned_bgr", "noise_37x21__444_q100_turned", "edge_2x4096__422_q85"):
        width, height, h, v, quality, turned, bgr = (int(x) for x in one["params/" + name])
        pixels = one["pixels/" + name.split("__")[0]]
        path = str(tmp_path / "out.jpg")
        host.encode_jpeg(path, pixels, quality, (h, v), bool(turned), bool(bgr), optimise=True)
        assert open(path, "rb").read() == two["file/" + name].tobytes(), name
        host.encode_jpeg(path, pixels, quality, (h, v), bool(turned), bool(bgr))
        assert open(path, "rb").read() == one["file/" + name].tobytes(), name + " (option off)"


def test_a_capacity_too_small_reports_the_size_and_writes_nothing(host):
    width, height, sampling, quality, blocks, _, two = T.file_case("noise_37x21__420_q85")
    out = np.full(len(two), 0x5A, np.uint8)
    size = C.c_long(0)
    call = lambda capacity: host.L.SolRx_JpegFileFromCoefficientsOptimised(
        blocks.ctypes.data, len(blocks), width, height, quality, sampling[0], sampling[1], out.ctypes.data, capacity,
        C.byref(size))
    assert call(len(two) - 1) == -1 and size.value == len(two) and (out == 0x5A).all()
    assert call(len(two)) == 0 and size.value == len(two) and out.tobytes() == two


def test_the_header_is_clean_under_the_sanitizers(tmp_path):
    """tests/jpeg_two_pass_check.cpp: census, optimiseTable and the coder with data-borne tables over the table tier, the
    synthetic blocks and the two cases made for the tables, compiled with the address and undefined-behaviour sanitizers
    and run as a program of its own (no device code in it); its buffers are sized exactly"""
    cases = [dict(c) for c in SYNTHETIC] + [T.limit_18_case(), T.rare_dense_case()]
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(TABLES)))
        for name in TABLES:
            counts, bits, values = T.table(name)
            f.write(struct.pack("<ii", len(counts), len(values)))
            f.write(counts.astype("<u4").tobytes() + bits.tobytes() + values.tobytes())
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            luma = c["sampling"][0] * c["sampling"][1]
            f.write(struct.pack("<iiiiq", c["sampling"][0], c["sampling"][1], c["width"], c["height"], len(c["blocks"])))
            f.write(c["blocks"].tobytes())
            f.write(T.census(c["blocks"], luma).astype("<u4").tobytes())
    exe = str(tmp_path / "jpeg_two_pass_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "jpeg_two_pass_check.cpp"),
                    os.path.join(ROOT, "sol-r_amd", "host", "JpegWriter.cpp")], check=True)
    run = subprocess.run([exe, path], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "%d tables, %d cases, %d blocks" % (len(TABLES), len(cases), sum(len(c["blocks"]) for c in cases)) in run.stdout
