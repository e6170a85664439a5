"""The entropy stage of the JPEG writer in its decomposed order (sol-r_amd/csrc/jpeg_entropy.h: bits, prefix sum, emit, count,
stuff) on the host-only engine, which runs the header's functions in loops (JpegWriter::scan): the same functions the HIP
engine's kernels call (tests/test_jpeg_entropy_gpu.py).

Held to three things that share nothing with the header: the one-pass writer (JpegWriter::encode behind
SolRx_JpegFromCoefficients, the bit-buffer coder the screenshots have used so far), the coder of the fixture generator
(write_jpeg of tests/golden/make_jpeg_encoder_fixtures.py, Python), and jpge's own files (tests/golden/jpeg_encoder.npz).
The inputs are the synthetic blocks of tests/jpeg_entropy_cases.py - each made for one edge of the bit stream, the edges
counted there - and the fixtures' blocks.  Every comparison is of every byte: no tolerance, no excluded case."""
import ctypes as C
import importlib.util
import os
import struct
import subprocess

import numpy as np
import pytest

import jpeg_entropy_cases as JC
from test_jpeg_encoder import BAD_ARGUMENTS, NAMES, assert_same_file, case

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = JC.cases()
CASE_NAMES = [c["name"] for c in CASES]
HEADER_BYTES = 623      # SOI 2, APP0 18, two DQT 138, SOF0 19, four DHT 66 + 366, SOS 14


def by_name(name):
    return CASES[CASE_NAMES.index(name)]


@pytest.fixture(scope="module")
def host(solr):
    k = solr.Kernel(engine="host-only")
    yield k
    k.finalize()


@pytest.fixture(scope="module")
def generator():
    spec = importlib.util.spec_from_file_location("make_jpeg_encoder_fixtures",
                                                  os.path.join(HERE, "golden", "make_jpeg_encoder_fixtures.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def one_pass_file(k, tmp_path, c):
    path = str(tmp_path / "one_pass.jpg")
    blocks = c["blocks"]
    assert k.L.SolRx_JpegFromCoefficients(os.fsencode(path), blocks.ctypes.data, len(blocks), c["width"], c["height"],
                                          c["quality"], c["sampling"][0], c["sampling"][1]) == 0
    return open(path, "rb").read()


def test_the_cases_are_the_ones_the_issue_asks_for():
    assert len(CASES) < 40 and max(len(c["blocks"]) for c in CASES) <= 4096
    assert len(set(CASE_NAMES)) == len(CASES)
    for c in CASES:
        assert c["reached"] and all(count > 0 for count in c["reached"].values()), (c["name"], c["reached"])
    assert {c["sampling"] for c in CASES} == {(1, 1), (2, 1), (2, 2)}
    tails = {(8 - c["edges"]["tail_bits"]) % 8 for c in CASES}
    assert tails == set(range(8))
    assert by_name("densest_sparsest")["edges"]["longest_block"] == 1658
    assert by_name("ff_run")["edges"]["ff_longest_run"] == 3
    assert max(c["edges"]["longest_block"] for c in CASES) <= 1660


def test_the_models_tables_are_the_fixture_generators(generator):
    """typed in twice, from the standard: they agree"""
    for mine, theirs in ((JC._DC_LUMA, generator.DC_LUMA), (JC._DC_CHROMA, generator.DC_CHROMA),
                         (JC._AC_LUMA, generator.AC_LUMA), (JC._AC_CHROMA, generator.AC_CHROMA)):
        assert (list(mine[0]), list(mine[1])) == (list(theirs[0]), list(theirs[1]))


def test_the_granularities_are_the_ones_the_cases_were_put_around(host):
    got = (C.c_int * 2)()
    host.L.SolRx_JpegEntropyGranularity(got)
    assert list(got) == [64, 256]
    blocks_per_group, chunk = got
    counts = {len(c["blocks"]) for c in CASES}
    # (65 is no multiple of 3, 4 or 6 blocks per MCU: 66 stands in, and 129 is 2c + 1)
    assert {blocks_per_group - 1, blocks_per_group, blocks_per_group + 2, 2 * blocks_per_group - 2, 2 * blocks_per_group,
            2 * blocks_per_group + 1} <= counts
    lengths = {c["edges"]["unstuffed_bytes"] for c in CASES}
    assert {chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1} <= lengths


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_decomposed_stage_gives_the_one_pass_writers_file(host, generator, tmp_path, name):
    c = by_name(name)
    got = host.jpeg_from_coefficients(c["blocks"], c["width"], c["height"], c["quality"], c["sampling"])
    assert_same_file(got, one_pass_file(host, tmp_path, c), name + " (JpegWriter::encode)")
    assert_same_file(got, generator.write_jpeg(c["width"], c["height"], c["sampling"], c["quality"], c["blocks"]),
                     name + " (write_jpeg)")
    scan, _, _ = JC.model_scan(c["blocks"], c["sampling"])
    assert got[HEADER_BYTES - 14:HEADER_BYTES - 12] == b"\xff\xda" and got[HEADER_BYTES:-2] == scan and \
        got[-2:] == b"\xff\xd9", name + " (the text model)"


@pytest.mark.parametrize("name", NAMES)
def test_the_fixtures_blocks_give_jpges_files_through_the_new_route(host, name):
    _, width, height, sampling, quality, _, _, want, blocks = case(name)
    assert_same_file(host.jpeg_from_coefficients(blocks, width, height, quality, sampling), want, name)


def test_the_prefix_sums_are_64_bits_wide(host):
    """lengths whose total passes 2^32 - as the 1.5 M blocks of a 2^26-pixel picture can - against numpy's uint64; a sum
    kept in 32 bits (the wrong restatement "offsets_in_32_bits") wraps and is told apart"""
    rng = np.random.RandomState(3)
    lengths = rng.randint(1600, 1661, 3 * 1000 * 1000).astype(np.uint32)
    got = np.full(len(lengths) + 1, 0x5A5A5A5A5A5A5A5A, np.uint64)
    host.L.SolRx_JpegEntropyPrefix(lengths.ctypes.data, len(lengths), got.ctypes.data)
    want = np.concatenate(([0], np.cumsum(lengths.astype(np.uint64))))
    assert want[-1] > 1 << 32 and np.array_equal(got, want)
    wrapped = np.concatenate(([0], np.cumsum(lengths, dtype=np.uint32))).astype(np.uint64)
    assert not np.array_equal(got, wrapped)
    big = np.full(8, 0xFFFFFFFF, np.uint32)
    got = np.zeros(9, np.uint64)
    host.L.SolRx_JpegEntropyPrefix(big.ctypes.data, 8, got.ctypes.data)
    assert got.tolist() == [i * 0xFFFFFFFF for i in range(9)]


def test_a_blocks_bits_and_its_bound(host):
    bits = lambda block, previous=0, chroma=0: host.L.SolRx_JpegBlockBits(
        np.ascontiguousarray(block, np.int16).ctypes.data, previous, chroma)
    zero = np.zeros(64, np.int16)
    assert bits(zero) == 2 + 4 and bits(zero, chroma=1) == 2 + 2
    densest = by_name("densest_sparsest")["blocks"][3]
    assert bits(densest) == 20 + 63 * 26 == 1658
    for c in CASES[:12]:
        _, offsets, _ = JC.model_scan(c["blocks"], c["sampling"])
        luma = c["sampling"][0] * c["sampling"][1]
        last = {}
        for i, block in enumerate(c["blocks"]):
            within = i % (luma + 2)
            component = 0 if within < luma else within - luma + 1
            assert bits(block, last.get(component, 0), component > 0) == offsets[i + 1] - offsets[i], (c["name"], i)
            last[component] = int(block[0])


OUTSIDE = [("dc_2048", 0, 2048, 0), ("dc_minus_2048", 0, -2048, 0), ("ac_1024", 1, 1024, 0), ("ac_minus_1024", 63, -1024, 0),
           ("dc_difference_2048", 0, 1024, 3)]


@pytest.mark.parametrize("what, position, value, block", OUTSIDE, ids=[o[0] for o in OUTSIDE])
def test_blocks_outside_the_domain_are_refused_with_nothing_written(host, what, position, value, block):
    blocks = np.zeros((6, 64), np.int16)
    blocks[0, 0] = -1024
    blocks[block, position] = value
    assert host.L.SolRx_JpegBlockBits(blocks[block].ctypes.data, int(blocks[0, 0]) if block else 0, 0) == -1
    out = np.full(4096, 0x5A, np.uint8)
    size = C.c_long(77)
    assert host.L.SolRx_JpegFileFromCoefficients(blocks.ctypes.data, 6, 16, 8, 85, 1, 1, out.ctypes.data, len(out),
                                                 C.byref(size)) == -1
    assert size.value == 0 and (out == 0x5A).all()
    with pytest.raises(Exception):
        host.jpeg_from_coefficients(blocks, 16, 8, 85, (1, 1))
    blocks[block, position] = value - 1 if value > 0 else value + 1          # the largest value inside
    assert len(host.jpeg_from_coefficients(blocks, 16, 8, 85, (1, 1))) > HEADER_BYTES


@pytest.mark.parametrize("bad", BAD_ARGUMENTS + [dict(blocks=5), dict(null="coefficients"), dict(null="file"),
                                                 dict(null="size"), dict(capacity=-1)],
                         ids=lambda b: "_".join("%s=%s" % kv for kv in b.items()))
def test_bad_arguments_are_refused_with_nothing_written(host, bad):
    a = dict(width=8, height=8, quality=85, sampling=(2, 2), blocks=6, null=None, capacity=4096)
    a.update(bad)
    blocks = np.zeros((6, 64), np.int16)
    out = np.full(4096, 0x5A, np.uint8)
    size = C.c_long(77)
    status = host.L.SolRx_JpegFileFromCoefficients(None if a["null"] == "coefficients" else blocks.ctypes.data, a["blocks"],
                                                   a["width"], a["height"], a["quality"], a["sampling"][0],
                                                   a["sampling"][1], None if a["null"] == "file" else out.ctypes.data,
                                                   a["capacity"], None if a["null"] == "size" else C.byref(size))
    assert status == -1 and (out == 0x5A).all() and size.value == (77 if a["null"] == "size" else 0)


def test_a_capacity_too_small_reports_the_size_and_writes_nothing(host):
    c = by_name("zero_runs")
    want = host.jpeg_from_coefficients(c["blocks"], c["width"], c["height"], c["quality"], c["sampling"])
    out = np.full(len(want), 0x5A, np.uint8)
    size = C.c_long(0)
    call = lambda capacity: host.L.SolRx_JpegFileFromCoefficients(
        c["blocks"].ctypes.data, len(c["blocks"]), c["width"], c["height"], c["quality"], c["sampling"][0],
        c["sampling"][1], out.ctypes.data, capacity, C.byref(size))
    assert call(len(want) - 1) == -1 and size.value == len(want) and (out == 0x5A).all()
    assert call(len(want)) == 0 and size.value == len(want) and out.tobytes() == want


@pytest.mark.parametrize("variant", JC.VARIANTS)
def test_the_cases_tell_a_wrong_restatement_from_the_right_one(host, variant):
    """a model with ONE statement restated wrongly differs, on at least one case, from the bytes the stage gives (which
    the tests above hold to the model restated rightly)"""
    caught = []
    for c in CASES:
        right, right_offsets, _ = JC.model_scan(c["blocks"], c["sampling"])
        try:
            wrong, wrong_offsets, _ = JC.model_scan(c["blocks"], c["sampling"], variant)
        except KeyError:                    # the wrong statement asks the tables for a category they do not have
            wrong, wrong_offsets = None, None
        if wrong != right or wrong_offsets != right_offsets:
            caught.append(c["name"])
    if variant == "offsets_in_32_bits":
        # no stream of 4096 blocks reaches 2^32 bits: this one is caught where the offsets are made
        # (test_the_prefix_sums_are_64_bits_wide), on lengths the model wraps and the header does not
        lengths = np.full(3 * 1000 * 1000, 1660, np.uint32)
        got = np.zeros(len(lengths) + 1, np.uint64)
        host.L.SolRx_JpegEntropyPrefix(lengths.ctypes.data, len(lengths), got.ctypes.data)
        assert not caught and int(got[-1]) != int(got[-1]) & 0xFFFFFFFF
        return
    assert caught, "no case tells '%s' from the right statement" % variant
    expected = {"eob_always": "last_position", "zrl_at_15": "zero_runs", "tail_byte_not_stuffed": "last_byte_ff",
                "stuffing_counted_per_word": "ff_run", "dc_from_any_component": "dc_predecessors"}
    if variant in expected:
        assert expected[variant] in caught


def test_the_header_is_clean_under_the_sanitizers(host, tmp_path):
    """tests/jpeg_entropy_check.cpp: the header's loops on every synthetic case, compiled with the address and
    undefined-behaviour sanitizers and run as a program of its own (no device code in it); its buffers are sized exactly"""
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(CASES)))
        for c in CASES:
            scan, _, _ = JC.model_scan(c["blocks"], c["sampling"])
            f.write(struct.pack("<iiiiqq", c["sampling"][0], c["sampling"][1], c["width"], c["height"], len(c["blocks"]),
                                len(scan)))
            f.write(c["blocks"].tobytes())
            f.write(scan)
    exe = str(tmp_path / "jpeg_entropy_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "jpeg_entropy_check.cpp"),
                    os.path.join(ROOT, "sol-r_amd", "host", "JpegWriter.cpp")], check=True)
    run = subprocess.run([exe, path], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "%d cases, %d blocks" % (len(CASES), sum(len(c["blocks"]) for c in CASES)) in run.stdout
