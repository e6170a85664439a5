"""The engine's texture tier per element, at the texel edges, against a model that shares nothing with it.

The five pieces of device code that decide a frame's colour - cubeMapping, sphereUVMapping and triangleUVMapping with their
shared fetchTexel, juliaSet and mandelbrotSet, the texel fetch of skyboxMapping, and what planeIntersection takes from them
(sol-r_amd/csrc/rt_device.h) - run here through the probes of include/solr_hip_probes.h on the cases of
tests/texture_mapper_cases.py, and are held

  * to tests/texture_mapper_model.py (plain Python from the reference's text) BIT FOR BIT on every output of every element:
    colour with w, bump normal, specular, attributes, ambient occlusion; for the planes by rays hit, and where they hit the hit
    point, the normal and the shadow intensity (what a test leaves in its outputs on a miss is the caller's locals).  An
    element the model calls ambiguous (a transcendental within its error bound of a binary32 rounding boundary) may take
    either neighbour's result.  The one-texel-wide fractals' NaN colours compare as NaN.  The mapping without columns, which
    the C oracle cannot be given (`x % 0` traps on the host), is compared here;
  * to the C oracle in the same mode (CUDA dialect, transcendentals rounded once) on everything the oracle was given;
  * to themselves across the wave: the case that deals every mapper, fractal lanes, untextured lanes and lanes that miss the
    texture into every wave of 64 returns the bits of the same elements sorted by mapper.

Instantiations.  solr_hip_probe_primitive takes a feature mask: the planes run in the instantiation the renderer would launch
for the resident scene (features = 0: the lean sphere + plane kernel for the untextured planes, the all-features one for the
textured) and in engine_probes.EVERYTHING.  solr_hip_probe_intersection_shader and solr_hip_probe_skybox have the one
all-features instantiation; what each call ran is asserted, so that no case silently runs an untextured row.

Safety.  Every table of every case passes the engine's own rule and every byte index lies inside the atlas: asserted by the
model on the CPU before anything is uploaded (texture_mapper_model.run).  engine_probes raises where the engine refuses an
upload or a probe, and the engine's error state is asserted clear after each case.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_probes as E  # noqa: E402
import texture_mapper_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu
_RAN = {}


@pytest.fixture
def rounded_oracle(solr, oracle):
    with TC.rounded_oracle(oracle) as L:
        yield L


def instantiations(case):
    if case["name"] == "primitive":
        return (("the renderer's instantiation", 0), ("all-features instantiation", E.EVERYTHING))
    return (("all-features instantiation (the probe's only one)", 0),)


def engine(solr, name, features=0):
    """the case through the engine's probe, once per instantiation for the whole module"""
    if (name, features) not in _RAN:
        case = TC.case(name)
        TC.model_outputs(name)                   # (tables and byte indices are asserted on the CPU before the upload)
        hip = solr.hip_lib()
        out = E.engine_outputs(solr, case, features=features)
        buf = C.create_string_buffer(512)
        assert hip.solr_hip_last_error(buf, 512) == 0, (name, buf.value)
        _RAN[name, features] = out
    return _RAN[name, features]


@pytest.mark.parametrize("name", TC.names())
def test_the_engine_equals_the_model_bit_for_bit(solr, name):
    case = TC.case(name)
    model, _, alternatives = TC.model_outputs(name)
    for label, features in instantiations(case):
        out = engine(solr, name, features)
        bad = TC.differing(case, model, alternatives, out)
        assert len(bad) == 0, "%s (%s): %d of %d elements differ from the model; first %d (%s)" % (
            name, label, len(bad), len(case["kind"]), bad[0], case["kind"][bad[0]])
        if case["name"] == "primitive":
            assert 0.1 < out["hit"].mean() < 0.9, name


@pytest.mark.parametrize("name", [n for n in TC.names() if n not in TC.NOT_FOR_THE_ORACLE])
def test_the_engine_equals_the_oracle_in_the_same_mode(solr, rounded_oracle, name):
    case = TC.case(name)
    _, _, alternatives = TC.model_outputs(name)
    theirs = TC.oracle_outputs(rounded_oracle, case)
    for label, features in instantiations(case):
        out = engine(solr, name, features)
        bad = [e for e in TC.differing(case, theirs, {}, out) if int(e) not in alternatives]
        assert len(bad) == 0, "%s (%s): %d of %d elements differ from the oracle; first %d (%s)" % (
            name, label, len(bad), len(case["kind"]), bad[0], case["kind"][bad[0]])


def test_a_wave_of_mixed_mappers_returns_the_bits_of_the_sorted_elements(solr):
    order = TC.mix_order(TC.case("mix_sorted")["kind"])
    sorted_out, mixed_out = engine(solr, "mix_sorted"), engine(solr, "mix_interleaved")
    for key in ("color", "bump", "specular", "advanced", "attributes"):
        same = TC.rows_equal(sorted_out[key][order], mixed_out[key])
        assert same.all(), (key, int((~same).sum()), int(np.flatnonzero(~same)[0]))


def test_the_probes_ran_the_instantiations_they_claim(solr):
    """features = 0 picks the renderer's row for the resident scene: sphere + plane (with either node loop) for the untextured
    planes, everything for the textured ones; the texture probes always run the all-features instantiation"""
    for name in TC.names():
        case = TC.case(name)
        picked = engine(solr, name, 0)["features"]
        if name == "planes_lean":
            assert picked & ~E.F_DEEP == E.F_SPHERE | E.F_PLANE, (name, picked)
        else:
            assert picked == E.EVERYTHING, (name, picked)
        if case["name"] == "primitive":
            assert engine(solr, name, E.EVERYTHING)["features"] == E.EVERYTHING, name
