"""The stick search of the PDB reader (sol-r_amd/csrc/stick_pairs.h) on the CPU: the host-only engine's loops held to the
numpy float32 model (tests/stick_pair_cases.py) on every case of the generator, start and partners as integers; the
threshold on the squared sum held to the root, float by float, around both reaches; and the reader, which now asks the
engine for the pairs, held to what it left before - to a restatement of its old nested loop, and to a recording of the
primitives the loader left before the search was moved (tests/golden/pdb_sticks_1bna.npz: `recorded()` below, run at the
commit before, for 1BNA.pdb and every geometry type).  tests/test_stick_pairs_gpu.py runs the same cases through the
kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import stick_pair_cases as S
from test_scene_files import PDB, _element_tables, parse_pdb

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pdb_sticks_1bna.npz")
CASES = S.cases()
f4 = np.float32
RECORDED = ("type", "p0", "p1", "p2", "size", "materialId", "vt0", "vt1", "vt2")

_EXPECTED = {}


def expected(case):
    """the model's (start, partners) of a case, computed once and shared (also with the GPU tests)"""
    if case not in _EXPECTED:
        start, partners = S.model(*CASES[case])
        start.setflags(write=False)
        partners.setflags(write=False)
        _EXPECTED[case] = (start, partners)
    return _EXPECTED[case]


# ---- calls (shared with the GPU tests: `fn` is the entry point of either library) ------------------------------------------
def records(case):
    positions, flags, reach = CASES[case]
    atoms = np.zeros((max(len(positions), 1), 4), f4)
    atoms[:len(positions), :3] = positions
    atoms[:, 3] = f4(np.nan)                        # the spare word is nobody's business
    backbone = np.zeros(max(len(positions), 1), np.uint8)
    backbone[:len(positions)] = np.where(flags, 0x80, 0)     # a truth value, not a 1
    return atoms, backbone, len(positions), reach


def call_pairs(fn, case, capacity=None):
    """fn(...) with room for `capacity` partners (None: sized with capacity 0 first): (total, start, partners with a canary
    behind the room)"""
    atoms, backbone, n, reach = records(case)
    start = np.full(n + 1, -7, np.int64)
    if capacity is None:
        capacity = fn(atoms.ctypes.data, backbone.ctypes.data, n, reach[0], reach[1], start.ctypes.data, None, 0)
        assert capacity >= 0
        start[:] = -7
    partners = np.full(capacity + 4, -9, np.int32)
    total = fn(atoms.ctypes.data, backbone.ctypes.data, n, reach[0], reach[1], start.ctypes.data, partners.ctypes.data,
               capacity)
    assert (partners[capacity:] == -9).all(), "partners written beyond the capacity"
    return total, start, partners[:capacity]


def assert_same_pairs(got, want, what):
    total, start, partners = got
    assert total == want[0][-1] == len(want[1]), "%s: %d pairs, the model has %d" % (what, total, len(want[1]))
    assert start.dtype == np.int64 and partners.dtype == np.int32
    assert np.array_equal(start, want[0]), "%s: start differs first at atom %d" % (what, np.argmax(start != want[0]))
    assert np.array_equal(partners, want[1][:len(partners)]), \
        "%s: partners differ first at place %d" % (what, np.argmax(partners != want[1][:len(partners)]))


def assert_csr_invariants(start, partners, n):
    assert len(start) == n + 1 and start[0] == 0 and start[-1] == len(partners) and (np.diff(start) >= 0).all()
    owner = np.repeat(np.arange(n), np.diff(start))
    assert (partners != owner).all(), "an atom is its own partner"
    assert ((partners >= 0) & (partners < max(n, 1))).all()
    same = owner[1:] == owner[:-1]
    assert (partners[1:][same] > partners[:-1][same]).all(), "an atom's partners do not ascend"
    there, back = owner * np.int64(n) + partners, partners * np.int64(n) + owner
    assert np.array_equal(np.sort(there), np.sort(back)), "j is i's partner and i not j's"


@pytest.fixture(scope="module")
def host(solr):
    k = solr.Kernel(engine="host-only")
    yield k
    k.finalize()


# ---- the cases against the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_pairs_are_the_models(host, case):
    positions, flags, reach = CASES[case]
    start, partners = host.stick_pairs(positions, flags, reach)
    assert_same_pairs((len(partners), start, partners), expected(case), case)
    assert_csr_invariants(start, partners, len(positions))
    assert_same_pairs(call_pairs(host.L.SolRx_StickPairs, case), expected(case), case + " (flags as truth values)")


def test_the_cases_are_what_they_are_named_for():
    assert np.array_equal(np.diff(expected("dense")[0]), np.full(130, 129))
    assert np.array_equal(np.diff(expected("coincident")[0]), [0] * 8 + [1] * 8)
    start, partners = expected("non-finite")
    assert not set(partners) & {3, 6, 9} and all(start[k] == start[k + 1] for k in (3, 6, 9)) and len(partners) == 9 * 8
    # the axis family: of the 9 steps about a reach the four below it bond, the reach itself and the four above do not
    assert np.array_equal(np.diff(expected("axis")[0]), ([1] * 8 + [0] * 10) * 2)
    assert np.nextafter(f4(1.7), f4(0)) < f4(1.7) and np.sqrt(f4(1.7) * f4(1.7)) == f4(1.7)
    # tiles: some atom of the largest case has a partner 256 or more ranks away, and one in the last, part-filled tile
    start, partners = expected("n4099")
    owner = np.repeat(np.arange(4099), np.diff(start))
    assert (np.abs(partners - owner) >= 256).any() and ((partners >= 4096) & (owner < 4096)).any()


@pytest.mark.parametrize("wrong", S.WRONG)
def test_a_wrong_restatement_is_told_apart(wrong):
    """<= for <, self by position, no flag test, the reaches swapped between the flags, a float64 sum: some case differs"""
    told = [case for case in sorted(CASES) if case != "n4099"
            and not all(np.array_equal(a, b) for a, b in zip(S.model(*CASES[case], wrong=wrong), expected(case)))]
    assert told, wrong
    if wrong == "float64_sum":
        assert set(told) == {"shell-1.7", "shell-3.4"}


def test_capacity_below_the_count_writes_only_that_many(host):
    want = expected("mixed-two-reaches")
    total = len(want[1])
    assert total > 8
    for capacity in (0, total - 1, total):
        assert_same_pairs(call_pairs(host.L.SolRx_StickPairs, "mixed-two-reaches", capacity), want, "capacity %d" % capacity)


def test_bad_arguments_are_refused(solr, host):
    for name, call in bad_calls(host.L.SolRx_StickPairs):
        assert call() == -1, name
    with pytest.raises(solr.SolrError):
        host.stick_pairs(np.zeros((2, 3)), [0, 1], reach=(1.7, float("nan")))
    with pytest.raises(ValueError):
        host.stick_pairs(np.zeros((2, 3)), [0])


def bad_calls(fn):
    """(name, call) for every argument the entry refuses; each call must return -1"""
    atoms, backbone, n, reach = records("n63")
    start, partners = np.zeros(n + 1, np.int64), np.zeros(64, np.int32)
    a, b, s, p = atoms.ctypes.data, backbone.ctypes.data, start.ctypes.data, partners.ctypes.data
    calls = [("null atoms", lambda: fn(None, b, n, 1.7, 3.4, s, p, 64)),
             ("null backbone", lambda: fn(a, None, n, 1.7, 3.4, s, p, 64)),
             ("null start", lambda: fn(a, b, n, 1.7, 3.4, None, p, 64)),
             ("null partners with a capacity", lambda: fn(a, b, n, 1.7, 3.4, s, None, 64)),
             ("n -1", lambda: fn(a, b, -1, 1.7, 3.4, s, p, 64)),
             ("n 2500001", lambda: fn(a, b, 2500001, 1.7, 3.4, s, p, 64)),
             ("capacity -1", lambda: fn(a, b, n, 1.7, 3.4, s, p, -1))]
    for bad in (0.0, -1.7, float("nan"), float("inf")):
        calls.append(("plain reach %r" % bad, lambda bad=bad: fn(a, b, n, bad, 3.4, s, p, 64)))
        calls.append(("backbone reach %r" % bad, lambda bad=bad: fn(a, b, n, 1.7, bad, s, p, 64)))
    return calls


# ---- the threshold on the squared sum -------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach", [S.REACH[0], S.REACH[1], f4(1.0), f4(1e-20), f4(3e19), f4(1e30)])
def test_the_threshold_gives_the_roots_verdict_for_every_sum(host, reach):
    """sqrtf is monotone, so one threshold T splits the sums: every float for 2 000 steps about T, and the ends of the range,
    gets the verdict sqrtf(s) < reach from s < T"""
    t = f4(host.L.SolRx_StickSquaredReach(reach))
    around = np.concatenate([S.steps_about(t, 2000), S.steps_about(reach * reach, 2000)]) if np.isfinite(t) else \
        np.array([np.finfo(f4).max, np.inf], f4)
    sums = np.concatenate([around, np.array([0.0, np.finfo(f4).tiny, np.finfo(f4).max, np.inf, np.nan], f4)])
    sums = sums[~(sums < 0)]
    with np.errstate(invalid="ignore", over="ignore"):
        assert np.array_equal(np.sqrt(sums) < reach, sums < t)
    if np.isfinite(t) and t > 0:
        assert np.sqrt(t) >= reach and np.sqrt(np.nextafter(t, f4(0))) < reach


# ---- the reader --------------------------------------------------------------------------------------------------------
def recorded(solr, engine, path, geometry_type):
    """the primitives a loader leaves, in the order they were added, as integers: what the golden file holds"""
    k = solr.Kernel(engine=engine, deterministic_seed=1)
    solr.scenes.pdb_molecule(k, path, width=64, height=48, geometry_type=geometry_type)
    prims = k.flat_scene().primitives
    prims = prims[np.argsort(prims["index"], kind="stable")][:-1]          # (the last one is the scene's lamp)
    nb = len(prims)
    assert np.array_equal(prims["index"], np.arange(nb))
    out = np.concatenate([np.ascontiguousarray(prims[name]).view(np.int32).reshape(nb, -1) for name in RECORDED], axis=1)
    k.finalize()
    return out


def old_loop(solr, geometry_type, scale=200.0, atom_size=100.0, stick_size=10.0):
    """The reader as it was, nested loop and all (sol-r_amd/host/PDBReader.cpp before the search left it; the reference's
    solr/io/PDBReader.cpp:395-690), over the map it builds: (type, p0, p1 or None, size.x, material) per primitive.  This
    statement of the old loop is the tests' alone."""
    colours, radii = _element_tables()
    atoms = parse_pdb(PDB)
    for n, a in enumerate(atoms):
        a["material"] = next(i for i, c in enumerate(colours) if c[0] == a["element"])
        a["w"] = f4(atom_size) if geometry_type == 1 else next(r for name, r in radii if name == a["element"])
        a["backbone"] = len(a["code"]) == 1 or geometry_type in (4, 5)
        a["key"] = a["id"] if (geometry_type == 2 or (geometry_type == 3 and a["residue"] % 2 == 0)) else n + 1
    by_key = {}
    for a in atoms:
        if geometry_type != 5 or a["backbone"]:
            by_key[a["key"]] = a                  # a later atom with the same key replaces the earlier one
    order = [by_key[key] for key in sorted(by_key)]
    pos = np.array([[a["x"], a["y"], a["z"]] for a in atoms], f4)
    mn, mx = pos.min(0), pos.max(0)
    centre = ((mn + mx) / f4(2)).astype(f4)
    s = (f4(scale) / (mx - mn)).astype(f4)
    spread = ((s * f4(2)) * f4(30)).astype(f4)

    def place(p):
        return (spread * (np.array(p, f4) - centre)).astype(f4)

    out = []
    for a in order:
        radius, stick = a["w"], a["w"]
        if geometry_type == 1:
            radius = f4(atom_size)
        elif geometry_type in (2, 5):
            radius = stick = f4(stick_size)
        elif geometry_type == 3:
            radius, stick = f4(a["w"] / f4(2)), f4(f4(stick_size) / f4(2))
        if geometry_type in (2, 3, 5):
            for b in order:
                if b is a or b["backbone"] != a["backbone"]:
                    continue
                ax, ay, az = f4(a["x"] - b["x"]), f4(a["y"] - b["y"]), f4(a["z"] - b["z"])
                distance = np.sqrt(f4(f4(f4(ax * ax) + f4(ay * ay)) + f4(az * az)))
                reach = f4(f4(1.7) * f4(2)) if geometry_type == 5 and b["backbone"] else f4(1.7)
                if distance < reach:
                    half = [f4(f4(a[c] + b[c]) / f4(2)) for c in "xyz"]
                    out.append((solr.ptCylinder, place([a["x"], a["y"], a["z"]]), place(half), f4(s[0] * stick),
                                a["material"] if geometry_type == 2 else 1010))
        radius = stick                              # no models: the atom takes the stick's radius
        material = 11 if geometry_type == 3 else a["material"]
        p = place([a["x"], a["y"], a["z"]])
        if geometry_type == 4 and a["backbone"] and a["chain"] % 2 == 0:
            out.append((solr.ptSphere, p, None, f4(f4(s[0] * radius) * f4(2)), 10))
        out.append((solr.ptSphere, p, None, f4(s[0] * radius), material))
    return out


@pytest.mark.parametrize("geometry_type", range(6))
def test_the_reader_leaves_what_it_left_before(solr, geometry_type):
    got = recorded(solr, "host-only", PDB, geometry_type)
    want = np.load(GOLDEN)["type%d" % geometry_type]
    assert got.shape == want.shape and np.array_equal(got, want), "the primitives differ from the recording"
    # and what the old nested loop over the reader's map would add
    loop = old_loop(solr, geometry_type)
    assert len(loop) == len(got) and (len(got) == 486 if geometry_type in (0, 1) else len(got) > 486)
    columns = np.cumsum([0] + [1, 3, 3, 3, 3, 1, 2, 2, 2])
    field = {name: got[:, columns[k]:columns[k + 1]] for k, name in enumerate(RECORDED)}
    for row, (ptype, p0, p1, size, material) in enumerate(loop):
        assert field["type"][row, 0] == ptype and field["materialId"][row, 0] == material, row
        assert np.array_equal(field["p0"][row], p0.view(np.int32)), row
        assert p1 is None or np.array_equal(field["p1"][row], p1.view(np.int32)), row
        assert field["size"][row, 0] == np.array(size, f4).view(np.int32), row
    assert (field["vt0"] == 0).all() and (field["vt1"] == f4(1).view(np.int32)).all() and (field["vt2"] == 0).all()


def test_the_host_only_engine_counts_its_searches(solr, host):
    before = host.stick_searches()
    host.stick_pairs(*CASES["n63"])
    after = host.stick_searches()
    assert (after[0] - before[0], after[1] - before[1]) == (0, 1)
    for geometry_type, searches in ((0, 0), (1, 0), (4, 0), (3, 1)):
        before = host.stick_searches()
        recorded(solr, "host-only", PDB, geometry_type)
        after = host.stick_searches()
        assert (after[0] - before[0], after[1] - before[1]) == (0, searches), geometry_type


# ---- the stand-alone program under the sanitizers ---------------------------------------------------------------------------
def test_the_header_is_clean_under_the_sanitizers(tmp_path):
    """tests/stick_pairs_check.cpp: the header's loops and the list builder on the generator's edge sizes, compiled with the
    address and undefined-behaviour sanitizers and run as a program of its own (no device code in it)"""
    exe = str(tmp_path / "stick_pairs_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", "-o", exe, os.path.join(HERE, "stick_pairs_check.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "12 sizes, the lists whole and cut short" in run.stdout
