"""(CPU, the oracle alone) The generator of tests/walk_margin_cases.py held to what keeps tests/test_walk_margins_gpu.py
from being vacuous: in every class of every case at least a fifth of the rays hit and at least a fifth miss (shadow cases:
are shadowed, are lit), the edge class has hits and misses on both sides of the edges, a wave composed as pure satisfies its
predicate on all 64 lanes and a wave with a stray on all but one, and the oracle's outputs hold no NaN.

Taken out of the generator because they cannot meet this, not masked where results are compared: origins far beyond the
view distance (64 extents and more away nothing is within the initial bound: every ray misses) - the view distance of 64
extents is a case of its own instead (`panels@64E`, and one step above it); lamps inside an occluder seen only from elsewhere
(every ray shadowed) - half of that class's points lie on the occluder itself, which the walk leaves out.  No class had to
go because the reference's arithmetic ends in NaN: leaves with a NaN coordinate or an infinite size are in the lists of
tests/test_list_copies_gpu.py only, not in the scenes rays are sent through."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import walk_margin_cases as W  # noqa: E402


@pytest.fixture(scope="module")
def solr():
    return importlib.import_module("sol-r_amd")


@pytest.fixture(scope="module")
def outputs(oracle):
    from oracle import probes
    L = oracle.lib()

    def run(case):
        assert L.oracle_get_dialect() == 0
        return probes._oracle_outputs(L, case)
    return run


def _found(case, out):
    return out["hit"] != 0 if case["name"] == "closest" else out["result"] > 0


def _all_cases(solr):
    for name in ("panels", "panels_opaque", "panels_glass", "foreign", "panels@64E", "panels@64E+"):
        for composition, case in W.closest_cases(solr, name).items():
            yield "%s closest %s" % (name, composition), case
    for composition, case in W.deep_cases(solr).items():
        yield "deep closest %s" % composition, case
    for name in ("panels", "panels_opaque", "panels_glass", "deep"):
        for composition, case in W.shadow_cases(solr, name).items():
            yield "%s shadow %s" % (name, composition), case


def test_every_class_of_every_case_hits_and_misses_and_no_output_is_a_nan(solr, outputs):
    cases = 0
    for label, case in _all_cases(solr):
        out = outputs(case)
        for key, value in out.items():
            assert not np.isnan(value).any(), (label, key)
        found = _found(case, out)
        n = len(found)
        assert 1000 <= n <= 7500 or "ragged" in label, (label, n)
        for cls in dict.fromkeys(case["cls"].tolist()):
            mine = case["cls"] == cls
            if mine.sum() >= 64:
                assert 0.2 <= found[mine].mean() <= 0.8, (label, cls, float(found[mine].mean()), int(mine.sum()))
        cases += 1
    assert cases == 4 * 4 + 2 + 4 + 4 * 4


def test_both_sides_of_the_edges_hold_hits_and_misses(solr, outputs):
    for name in ("panels", "foreign"):
        sc = W.scene(solr, name)
        block = W.edge_blocks(sc, np.random.default_rng(31))[0]
        case = dict(name="closest", scene=sc, si=sc.si, origins=block.origins, targets=block.targets, iteration=block.iteration,
                    current=block.current)
        found = outputs(case)["hit"] != 0
        for side in (-1, 0, 1):
            share = found[block.side == side].mean()
            assert 0.1 <= share <= 0.9, (name, side, float(share))
        assert (block.side == 0).sum() >= 200 and (block.side == -1).sum() == (block.side == 1).sum() >= 800
        # every offset of the issue is there: on the edge, one ULP, half a margin, a margin, two margins to either side
        assert len(block.origins) == len(sc.rectangles()) * 8 * 9


def test_the_waves_are_what_they_are_composed_as(solr):
    for label, case in _all_cases(solr):
        if case["name"] != "closest":
            continue
        o, d = case["origins"], W.direction(case)
        vd = float(case["si"].viewDistance)
        n = len(o)
        assert len(case["waves"]) == -(-n // W.WAVE), label
        pure = strays = 0
        for w, (cls, wants, lane) in enumerate(case["waves"]):
            lanes = slice(w * W.WAVE, min((w + 1) * W.WAVE, n))
            if wants is None:
                continue
            assert lanes.stop - lanes.start == W.WAVE
            holds = W.PREDICATES[wants](o[lanes], d[lanes], vd)
            assert W.sure(d[lanes]).all(), (label, w)
            if lane < 0:
                assert holds.all(), (label, w, cls, wants)
                pure += 1
            else:
                assert (~holds).sum() == 1 and not holds[lane], (label, w, cls, wants, lane)
                strays += 1
        if "one_stray" in label:
            assert strays >= 20 and pure == 0, (label, strays, pure)
        elif "pure" in label:
            assert pure >= 20 and strays == 0, (label, pure)
        if "ragged_1" in label:
            assert n % W.WAVE == 1
        if "ragged_63" in label:
            assert n % W.WAVE == 63


def test_the_shadow_waves_with_a_stray_have_one_short_ray(solr):
    for name in ("panels_opaque", "deep"):
        cases = W.shadow_cases(solr, name)
        for composition in ("pure", "one_stray"):
            case = cases[composition]
            d = (case["lamps"] - case["origins"]).astype(np.float32)
            short = ~W.long_ray(d)
            per_wave = [int(short[w:w + W.WAVE].sum()) for w in range(0, len(d) - W.WAVE + 1, W.WAVE)]
            cls = [case["cls"][w] for w in range(0, len(d) - W.WAVE + 1, W.WAVE)]
            for count, c in zip(per_wave, cls):
                if c != "lamp_within_2":
                    assert count == (1 if composition == "one_stray" else 0), (name, composition, c, count)
        for cls in ("one_octant",) + (("one_octant_tiny_components",) if name == "deep" else ()):
            octants = [len(set(W.octant((cases["pure"]["lamps"] - cases["pure"]["origins"])[w:w + W.WAVE]).tolist()))
                       for w in np.flatnonzero(cases["pure"]["cls"] == cls)[::W.WAVE]]
            assert octants and max(octants) == 1, (name, cls, octants)


def test_the_face_class_puts_box_faces_around_the_cut_off(solr):
    """the lamp of every ray of that class lies so that some leaf's box is entered at 1 - 1e-3 ... 1.01 along point -> lamp"""
    sc = W.scene(solr, "panels_glass")
    case = W.shadow_cases(solr, "panels_glass")["pure"]
    mine = np.flatnonzero(case["cls"] == "face_at_the_cut_off")
    leaves = np.flatnonzero(sc.boxes["nbPrimitives"] > 0)
    lo, hi = sc.boxes["min"][leaves].astype(np.float64), sc.boxes["max"][leaves].astype(np.float64)
    got = {p: 0 for p in W.FACE_PARAMETERS}
    for j in mine:
        o, d = case["origins"][j].astype(np.float64), (case["lamps"][j] - case["origins"][j]).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (lo - o) / d, (hi - o) / d
        near, far = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
        entries = near[near <= far]
        want = W.FACE_PARAMETERS[(j - mine[0]) % len(W.FACE_PARAMETERS)]
        if np.abs(entries - want).min() < 2e-5:
            got[want] += 1
    assert all(count >= 0.9 * len(mine) / len(W.FACE_PARAMETERS) for count in got.values()), got
