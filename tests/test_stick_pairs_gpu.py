"""The stick search on the device (sol-r_amd/csrc/solr_sticks.hip; needs the MI355X: `pytest -m gpu`): the cases of
tests/test_stick_pairs.py through solr_hip_stick_pairs, start and partners word for word against the numpy model
(tests/stick_pair_cases.py) and against the host-only engine; the counter of pairs examined, which tells which route ran;
the arguments refused before a device is touched; the total the entry declines; and the PDB reader with the HIP engine -
the primitives the host-only engine leaves, and the searches served where the geometry type has sticks."""
import numpy as np
import pytest

import stick_pair_cases as S
from test_scene_files import PDB
from test_stick_pairs import CASES, assert_csr_invariants, assert_same_pairs, bad_calls, call_pairs, expected, recorded

pytestmark = pytest.mark.gpu
f4 = np.float32


@pytest.fixture(scope="module")
def hip(solr, have_gpu):
    assert have_gpu, "no GPU: the device route of the stick search cannot be tested here"
    lib = solr.hip_lib()
    lib.solr_hip_clear_error()
    return lib


def no_error(hip):
    return hip.solr_hip_last_error(None, 0) == 0


def counted(hip, tests, call):
    """call(), which must examine `tests` ordered pairs on the device"""
    before = hip.solr_hip_stick_pair_tests()
    result = call()
    assert hip.solr_hip_stick_pair_tests() - before == tests
    return result


@pytest.mark.parametrize("case", sorted(CASES))
def test_pairs_are_the_models_and_the_host_engines(solr, hip, case):
    n = len(CASES[case][0])
    want = expected(case)
    # sized with capacity 0, a pass to count; then the call itself, a pass to count and - where there are pairs - one to store
    passes = (2 if n else 0) + (1 if len(want[1]) else 0)
    got = counted(hip, passes * n * n, lambda: call_pairs(hip.solr_hip_stick_pairs, case))
    assert_same_pairs(got, want, "solr_hip_stick_pairs " + case)
    assert_csr_invariants(got[1], got[2], n)
    host = solr.Kernel(engine="host-only")
    start, partners = host.stick_pairs(*CASES[case])
    assert np.array_equal(got[1], start) and np.array_equal(got[2], partners)
    assert no_error(hip)


def test_a_full_call_examines_every_ordered_pair_twice(hip):
    want = expected("n513")
    total = len(want[1])
    got = counted(hip, 2 * 513 * 513, lambda: call_pairs(hip.solr_hip_stick_pairs, "n513", total))
    assert_same_pairs(got, want, "n513")


def test_capacity_below_the_count_writes_only_that_many(hip):
    want = expected("mixed-two-reaches")
    total = len(want[1])
    for capacity in (0, total - 1, total):
        got = counted(hip, (2 if capacity else 1) * 257 * 257,
                      lambda: call_pairs(hip.solr_hip_stick_pairs, "mixed-two-reaches", capacity))
        assert_same_pairs(got, want, "capacity %d" % capacity)


def test_bad_arguments_are_refused_before_a_device_is_touched(solr, hip):
    import ctypes as C
    before = hip.solr_hip_stick_pair_tests()
    for name, call in bad_calls(hip.solr_hip_stick_pairs):
        assert call() == -1, name
        message = C.create_string_buffer(512)
        assert hip.solr_hip_last_error(message, 512) != 0, name
        assert b"solr_hip_stick_pairs" in message.value, (name, message.value)
        hip.solr_hip_clear_error()
    assert hip.solr_hip_stick_pair_tests() == before


def test_more_pairs_than_the_entry_indexes_are_declined(hip):
    """46 342 atoms at one place are each other's partners: 46 342 x 46 341 pairs, 1 414 more than 2^31 - 1.  Declined: -1,
    no error pending, start written, one pass made"""
    n = 46342
    assert n * (n - 1) > 2 ** 31 - 1 >= (n - 1) * (n - 2)
    atoms = np.zeros((n, 4), f4)
    atoms[:, :3] = (3.0, -1.0, 2.0)
    backbone = np.zeros(n, np.uint8)
    start, partners = np.zeros(n + 1, np.int64), np.full(16, -9, np.int32)
    got = counted(hip, n * n, lambda: hip.solr_hip_stick_pairs(atoms.ctypes.data, backbone.ctypes.data, n, 1.7, 3.4,
                                                               start.ctypes.data, partners.ctypes.data, 16))
    assert got == -1 and no_error(hip)
    assert np.array_equal(start, np.arange(n + 1, dtype=np.int64) * (n - 1)) and (partners == -9).all()


def served(k, call):
    before = k.stick_searches()
    result = call()
    after = k.stick_searches()
    return result, (after[0] - before[0], after[1] - before[1])


@pytest.mark.parametrize("geometry_type", range(6))
def test_the_reader_leaves_the_host_engines_primitives(solr, hip, geometry_type):
    k = solr.Kernel(engine="hip")
    before = k.set_stick_device_from(0)          # 1BNA's 486 atoms are fewer than the engine sends to the device by itself
    try:
        got, searches = served(k, lambda: recorded(solr, "hip", PDB, geometry_type))
    finally:
        assert k.set_stick_device_from(before) == 0
    assert searches == ((1, 0) if geometry_type in (2, 3, 5) else (0, 0))
    want = recorded(solr, "host-only", PDB, geometry_type)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert no_error(hip)


def test_a_small_molecule_takes_the_loops_by_default(solr, hip):
    k = solr.Kernel(engine="hip")
    assert 486 < k.set_stick_device_from(0) < 4099
    k.set_stick_device_from(486)
    _, searches = served(k, lambda: k.stick_pairs(*CASES["n511"]))
    assert searches == (1, 0)
    _, searches = served(k, lambda: k.stick_pairs(*CASES["n257"]))
    assert searches == (0, 1)
    assert k.set_stick_device_from(0) == 486


def write_pdb(path, positions):
    """ATOM lines with every field where the reader cuts it (sol-r_amd/host/PDBReader.h): atom codes of one and of two
    letters, two chains, residues of seven atoms"""
    with open(path, "w") as out:
        for i, (x, y, z) in enumerate(positions):
            line = [" "] * 80

            def put(at, text):
                line[at:at + len(text)] = text

            put(0, "ATOM")
            put(7, "%4d" % ((i + 1) % 10000))
            put(13, "CNO"[i % 3] + "A" * (i % 2))
            put(17, "ALA")
            put(21, "AB"[(i // 700) % 2])
            put(23, "%3d" % ((i // 7) % 1000))
            put(30, "%8.3f" % x)
            put(38, "%8.3f" % y)
            put(46, "%8.3f" % z)
            put(76, " " + "CNO"[i % 3])
            out.write("".join(line) + "\n")


@pytest.mark.parametrize("geometry_type", [3, 5])
def test_a_molecule_of_4099_atoms_loads_alike_on_both_engines(solr, hip, tmp_path, geometry_type):
    """more than a tile of atoms, the last tile part-filled, through the reader: type 3 keys half the residues by serial
    number and has atoms of both flags, type 5 keys by position and doubles the reach"""
    path = str(tmp_path / "synthetic.pdb")
    write_pdb(path, np.round(S.cloud(4099, 5).astype(np.float64), 3))
    k = solr.Kernel(engine="hip")
    got, searches = served(k, lambda: recorded(solr, "hip", path, geometry_type))
    assert searches == (1, 0)
    want, searches = served(k, lambda: recorded(solr, "host-only", path, geometry_type))
    assert searches == (0, 1)
    assert len(got) > 4099 and got.shape == want.shape and np.array_equal(got, want)
    assert no_error(hip)
