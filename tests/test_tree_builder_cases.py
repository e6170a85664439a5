"""The host box-grid builder (sol-r_amd/host/GPUKernel.cpp compactBoxes(true)) against the line-by-line model of the
reference's (tests/test_builder_reference_model.py) on the synthetic scenes of tests/tree_builder_cases.py - and each scene
against what it is named after.  The host builder is what the device builder is held to, case by case
(tests/test_tree_build_gpu.py); here it is itself held to the model: the number of nodes, every node's bounds as 32-bit
patterns (the sign of a zero counts), the primitive counts, start indices and skip pointers, the order of the primitives
including its length, and the lights.  No GPU."""
import numpy as np
import pytest

import test_builder_reference_model as M
import tree_builder_cases as K

F = np.float32


@pytest.fixture(scope="module")
def built(solr):
    cache = {}

    def get(name):
        if name not in cache:
            c = K.CASES[name]
            spec = c.spec(solr)
            assert len(spec) <= 3100, "the scenes stay small"
            cache[name] = (spec,) + M._build_both(solr, spec, c.view_distance, move=c.move, capacity=c.capacity,
                                                  movable=c.movable)
        return cache[name]
    return get


def _words(v):
    return [int(x) for x in np.asarray(v, F).view(np.uint32)]


@pytest.mark.parametrize("name", list(K.CASES))
def test_the_host_builder_is_the_model(built, name):
    spec, model, boxes, order, lights = built(name)
    assert len(boxes) == len(model.nodes), (len(boxes), len(model.nodes))
    assert len(order) == len(model.order), (len(order), len(model.order))
    assert order == [M.i32(p) for p in model.order], "primitive order differs"     # (a box key streamed as a primitive
    assert lights == [M.i32(p) for p in model.lamps], "light list differs"          #  is held in an int)
    for i, (b, n) in enumerate(zip(boxes, model.nodes)):
        got = (_words(b["min"]), _words(b["max"]), int(b["nbPrimitives"]), int(b["startIndex"]),
               int(b["indexForNextBox"][0]), int(b["indexForNextBox"][1]))
        want = (_words(n["lo"]), _words(n["hi"]), n["nb"], n["start"], n["skip"], 0)
        assert got == want, "node %d: builder %s, reference model %s" % (i, got, want)


@pytest.mark.parametrize("name", list(K.CASES))
def test_the_case_steers_what_it_is_named_after(solr, built, name):
    spec, model, boxes, order, lights = built(name)
    assert sorted(model.declined) == sorted(K.CASES[name].declined), model.declined
    K.CASES[name].check(solr, spec, model)


def test_the_engine_cases_exist_and_cover_what_they_are_meant_to():
    assert set(K.ENGINE_CASES) <= set(K.CASES) and len(set(K.ENGINE_CASES)) == len(K.ENGINE_CASES) >= 8
    picked = [K.CASES[n] for n in K.ENGINE_CASES]
    assert any(c.declined for c in picked) and any(K.FEW in c.declined for c in picked)
    assert any(c.movable is not None and len(set(c.movable)) == 2 for c in picked)
    assert any(n.startswith("members:") for n in K.ENGINE_CASES)


def test_cast_int_outside_int():
    """what the model defines where the reference leaves the conversion undefined: the host's compiled code"""
    with np.errstate(all="ignore"):
        for v in (F(2.0 ** 31), F(6.4e9), F(-2.0 ** 31) * F(1.5), F(np.inf), F(-np.inf), F(np.nan)):
            assert M.cast_int(v) == -2 ** 31 and not M.fits_int(v)
    assert M.cast_int(F(-2.0 ** 31)) == -2 ** 31 and M.fits_int(F(-2.0 ** 31))
    assert M.cast_int(F(2147483520.0)) == 2147483520 and M.cast_int(F(-0.75)) == 0 and M.cast_int(F(-1.5)) == -1
