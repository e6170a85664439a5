"""closestHitWalk and shadowWalk (rt_device.h) on the rays of tests/walk_margin_cases.py - aimed at the margins and
thresholds their short cuts rest on - held, ray by ray and bit for bit, with no element left out and no tolerance,

  1. to themselves with each short cut switched off: the reference's own node list (exactNodes), the reference's leaves
     (solr_hip_set_variant(8): no thin copies), unsorted lists (12), no lamp cut-off (15), no order-free lists (6);
  2. to the oracle's CUDA dialect, on the reference's own node list: the bar tests/test_engine_probes_gpu.py holds the
     engine to on the rays of its fixture;

after asserting (solr_hip_probe_walk_offer) that the walk is offered the short cut the case is about - a case must not pass
because its path was never taken.  Compared: hit, result and colour of every element; the primitive wherever either side
has a hit; hit point, normal and areas wherever both have (what a walk leaves in its in/out locals on a miss is nobody's
business).

`foreign` - leaf boxes of another host's that are smaller than their planes - is the case the thin copy could not be
walked on: a ray through such a box hits the plane beside it, the reference finds that hit, the copy cut with the box does
not.  The engine offers the thin copy only for lists that hold what they name (solr_arena.hip tightListsFor).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_probes as E  # noqa: E402
import walk_margin_cases as W  # noqa: E402

pytestmark = pytest.mark.gpu
i4 = np.int32
REFERENCE_LEAVES, NO_ORDER_FREE, UNSORTED_LISTS, NO_LAMP_CUTOFF = 8, 6, 12, 15
SHADOWS_OPAQUE, SHADOWS_LAMP_CUTOFF = 1, 2


def _rows_differ(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (a.view(i4) != b.view(i4)).reshape(len(a), -1).any(axis=1)


def differing(kind, mine, theirs):
    """per element: does any compared output differ?  (and per output, how many)"""
    n = len(mine["hit" if kind == "closest" else "result"])
    bad, per_key = np.zeros(n, bool), {}
    if kind == "closest":
        found = (mine["hit"] != 0) & (theirs["hit"] != 0)
        for key in ("hit", "primitive", "intersection", "normal", "areas"):
            d = _rows_differ(mine[key], theirs[key])
            if key not in ("hit", "primitive"):
                d &= found
            elif key == "primitive":
                d &= (mine["hit"] != 0) | (theirs["hit"] != 0)
            per_key[key] = int(d.sum())
            bad |= d
    else:
        for key in ("result", "color"):
            d = _rows_differ(mine[key], theirs[key])
            per_key[key] = int(d.sum())
            bad |= d
    return bad, per_key


class Report:
    def __init__(self):
        self.failures = []

    def compare(self, what, case, mine, theirs):
        bad, per_key = differing(case["name"], mine, theirs)
        if bad.any():
            classes = {c: int(bad[case["cls"] == c].sum()) for c in dict.fromkeys(case["cls"].tolist()) if bad[case["cls"] == c].any()}
            self.failures.append("%s: %d of %d rays differ %s, by class %s, first %d" % (what, int(bad.sum()), len(bad), per_key, classes,
                                                                                        int(np.flatnonzero(bad)[0])))
            print("DIFFERS  " + self.failures[-1])

    def done(self):
        assert not self.failures, "\n".join(self.failures)


def _oracle(oracle, case):
    from oracle import probes
    L = oracle.lib()
    assert L.oracle_get_dialect() == 0
    return probes._oracle_outputs(L, case)


def _run(solr, oracle, scene_name, cases, switches, expect, short_ray_lists=-1):
    """every case of a scene under one Resident: variant 0 on the engine's lists against each switch and the reference's list,
    the reference's list against the oracle"""
    hip = solr.hip_lib()
    sc = W.scene(solr, scene_name)
    report = Report()
    with E.Resident(solr, sc.si, sc.boxes, sc.prims, sc.materials, sc.textures, sc.lights, sc.nb_lamps):
        try:
            hip.solr_hip_set_short_ray_lists(short_ray_lists)
            offer = E.walk_offer(hip, sc.si)
            print("%s: %s" % (scene_name, offer))
            expect(offer)
            for composition, case in cases.items():
                what = "%s %s %s (%d rays)" % (scene_name, case["name"], composition, len(case["origins"]))
                base = E.walk_outputs(hip, case)
                for variant in switches:
                    hip.solr_hip_set_variant(variant)
                    out = E.walk_outputs(hip, case)
                    hip.solr_hip_set_variant(0)
                    assert out["features"] == base["features"]
                    report.compare("%s, variant 0 against variant %d" % (what, variant), case, base, out)
                exact = E.walk_outputs(hip, case, exact=1)
                report.compare("%s, the engine's lists against the reference's list" % what, case, base, exact)
                want = _oracle(oracle, case)
                assert not any(np.isnan(v).any() for v in want.values()), what
                report.compare("%s, the reference's list against the oracle" % what, case, exact, want)
                report.compare("%s, the engine's lists against the oracle" % what, case, base, want)
                share = (want["hit"] != 0).mean() if case["name"] == "closest" else (want["result"] > 0).mean()
                assert 0.15 < share < 0.85, (what, share)
                expect(offer, base)
        finally:
            hip.solr_hip_set_variant(0)
            hip.solr_hip_set_short_ray_lists(-1)
    report.done()


@pytest.mark.parametrize("scene_name", ["panels", "panels_opaque", "panels_glass", "panels@64E", "panels@64E+", "foreign"])
def test_closest_hits_on_the_panels(solr, oracle, scene_name):
    def expect(offer, out=None):
        if scene_name == "foreign":
            # recorded, not assumed: its boxes do not hold their planes - no order-free lists, no lamp cut-off, and the walks
            # are not offered the thin copy that was cut with those boxes
            assert offer["nbBoxesFree"] == 0 and not (offer["opaqueShadows"] & SHADOWS_LAMP_CUTOFF) and offer["tightLists"] == 0
        elif scene_name == "panels@64E+":
            assert offer["tightLists"] == 0 and offer["nbBoxesFree"] > 0       # viewDistance one step above 64 extents
        else:
            assert offer["tightLists"] == 1 and offer["nbBoxesFree"] > 0
        assert offer["nbBoxes"] <= 1024
        if out is not None:
            # the lean sphere + plane instantiation (the Cornell box's) where nothing is textured, else the one with everything
            assert out["features"] == (E.F_SPHERE | E.F_PLANE if scene_name == "panels_opaque" else E.EVERYTHING)

    switches = [REFERENCE_LEAVES] + ([NO_ORDER_FREE] if scene_name in ("panels", "panels_opaque") else [])
    _run(solr, oracle, scene_name, W.closest_cases(solr, scene_name), switches, expect)


@pytest.mark.parametrize("short_ray_lists", [-1, 1], ids=["short-rays-in-the-reference-s-order", "short-rays-on-the-order-free-lists"])
def test_closest_hits_on_the_deep_list(solr, oracle, short_ray_lists):
    def expect(offer, out=None):
        assert offer["nbBoxesFree"] > 0 and offer["sortedLists"] == 1 and offer["tightLists"] == 0 and offer["nbBoxes"] > 1024
        assert offer["shortRayLists"] == (1 if short_ray_lists == 1 else 0)
        if out is not None:
            assert out["features"] & E.F_DEEP and out["features"] & E.F_TRI

    cases = W.deep_cases(solr)
    octants = W.same_octant_waves(cases["pure"])
    assert octants[:16].all() and not octants[16:32].any()          # the sorted copy's waves, the generic loop's
    tiny = np.flatnonzero(cases["pure"]["cls"] == "one_octant_tiny_components")
    assert tiny[0] == 32 * W.WAVE and len(tiny) == 8 * W.WAVE and octants[32:40].all()     # ... the sorted copy's again:
    d = W.direction(cases["pure"])[tiny]                                                  # components of +-0 and denormals
    assert ((d == 0) | (np.abs(d) < 1e-29)).any(axis=1).all() and (d == 0).any() and np.signbit(d[d == 0]).any()
    assert W.long_ray(d).all()
    _run(solr, oracle, "deep", cases, [UNSORTED_LISTS, NO_ORDER_FREE], expect, short_ray_lists)


@pytest.mark.parametrize("scene_name", ["panels", "panels_opaque", "panels_glass", "deep"])
def test_shadows_with_the_lamp_at_the_cut_off(solr, oracle, scene_name):
    """panels (a textured plane scales a shadow) and panels_glass keep the reference's order: the lamp's cut-off is the path
    under test; panels_opaque - the textured plane made a wireframe one - and deep take the order-free lists, deep's waves
    of one octant the reversed loop over the sorted copy"""
    def expect(offer, out=None):
        assert offer["opaqueShadows"] & SHADOWS_LAMP_CUTOFF
        assert bool(offer["opaqueShadows"] & SHADOWS_OPAQUE) == (scene_name in ("panels_opaque", "deep"))
        assert offer["nbBoxesFree"] > 0 and offer["tightLists"] == (0 if scene_name == "deep" else 1)
        assert offer["sortedLists"] == 1

    if scene_name == "deep":
        case = W.shadow_cases(solr, scene_name)["pure"]
        mine = np.flatnonzero(case["cls"] == "one_octant_tiny_components")
        d = (case["lamps"] - case["origins"])[mine]
        assert len(mine) % W.WAVE == 0 and mine[0] % W.WAVE == 0 and W.long_ray(d).all()
        assert all(len(set(W.octant(d[w:w + W.WAVE]).tolist())) == 1 for w in range(0, len(mine), W.WAVE))
        assert ((d == 0) | (np.abs(d) < 1e-29)).any(axis=1).all() and np.signbit(d[d == 0]).any()
    switches = [NO_LAMP_CUTOFF, NO_ORDER_FREE] + ([UNSORTED_LISTS] if scene_name == "deep" else [REFERENCE_LEAVES])
    _run(solr, oracle, scene_name, W.shadow_cases(solr, scene_name), switches, expect)
