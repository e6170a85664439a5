"""THE ENGINE against THE REFERENCE'S OWN FUNCTIONS, element for element, with no oracle in between.

tests/golden/reference_probes.npz holds arrays of inputs and what the reference's own functions (RayTracer.cl, wrapped
by oracle/ref_probes.cl, source-order build: oracle/Makefile) returned for them on an MI355X.  The test-only entry
points of include/solr_hip_probes.h evaluate the ENGINE's device functions - the ones k_standardRenderer is built
from, in the instantiations the renderer launches - on the same arrays (tests/engine_probes.py), and the results are
compared with the reference's BIT FOR BIT wherever the function is not under one of the 36 statements in which the
reference's two engines differ (the fixture is the OpenCL engine's, the product is held to the
CUDA engine's):

  function                                   engine == reference, bit for bit, on
  boxIntersection, three forms               every ray without a zero direction component (switch 0: the reciprocal of
    (compare chain, sign-free, node loop)      0); the hand-scheduled node loop on the elements with t0 = 0, its only form
  sphere / ellipsoid / cylinder / cone /     hit flag, hit point, shadow intensity of EVERY element, normal of every
    plane / checkerboard / triangle tests      primitive but triangles (switches 8-9: areas raw, normal normalised); the
    as both walks dispatch them                double-sided rule of triangles is switch 10
  intersectionWithPrimitives                 Cornell room with glass, sticks: every output of every ray; triangle meshes
    (lean and all-features instantiations,     and the textured scene: hit, primitive, hit point of every ray, normal and
    walk-order list / order-free lists /       areas where the primitive is no triangle; the mixed scene (cones: switch 11)
    the reference's own list)                  wherever the two pick the same primitive
  intersectionShader + mappers + maps        colour, bump normal, attributes, ambient occlusion of every element; the
                                               specular vector of everything but spheres (switch 2)
  skyboxMapping, vectorRefraction /          every element
    vectorReflection, makeColor RGB / BGR

  primitiveShader (solr_hip_probe_shader)    every output of every element on which no dialect statement can show (below):
                                               94 % of the Cornell room's, 100 % of the three "moot" cases'; the Blinn sum
                                               within the library pow's ULPs
  launchRayTracing: the frames rendered by   ids, depth, colour of every pixel on which no dialect statement can show
    k_standardRenderer ITSELF (pass 0)
  k_default, k_depthOfField,                 the RGB8 image: every pixel of k_default (plain and accumulated); the two
    k_ambientOcclusion over a frame buffer     others where the dialects agree

Where a switch applies the engine must equal the oracle's CUDA dialect on those elements (and does on ALL elements of
every case: asserted as well) - that is the residue that rests on the reading of the CUDA text
(tests/cuda_text_model.py).

THE SWITCH-OBSERVABILITY MASK (round 5).  processShadows sits under three of the 36 statements (14-16), primitiveShader
under four more (18-21), launchRayTracing under ten (22-31): no structural mask like "not a triangle" separates their
elements.  But most of those statements cannot be SEEN on most inputs (one lamp: 19; innerIllumination.x == 0: 18, 21;
pass < 10: 20; no transparent occluder: 16; nothing of the point's own primitive in the way: 15; no occluder within 5 %
of the way to the lamp: 14).  oracle.probes.dialects_agree runs the oracle in BOTH dialects on the case's inputs: an
output on which the two return the same bits is one on which the reference's own (OpenCL, source-order) output IS the
CUDA engine's answer, and the engine is held to it there bit for bit (the Blinn term: within the ULPs of the library
pow) - for every case of every kind, next to the structural masks above; the covered fraction is printed per output.
The "moot" cases (oracle.probes.case_shadow / case_shader with moot=True: opaque occluders, one lamp, no emissive
material but the lamp's, pass < 10, elements selected for agreement) are covered on EVERY element, and are probed the
way the renderer calls the walk (the shaded primitive left out, GI:829).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_probes as E  # noqa: E402
from helpers import ulp_distance  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_probes.npz")
ptTriangle, ptSphere, ptCone = 2, 0, 12


@pytest.fixture(scope="module")
def probes(solr, oracle):
    from oracle import probes as module
    return module


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


def _load(probes, fixture, name):
    inputs = {k.split("/", 2)[2]: fixture[k] for k in fixture.files if k.startswith(name + "/in/")}
    assert inputs, name
    case = probes.unpack(inputs)
    ref = {k.split("/")[2]: fixture[k] for k in fixture.files if k.startswith(name + "/source_order/")}
    return case, ref


def _rows_equal(probes, a, b):
    same = probes.same_bits(np.asarray(a), np.asarray(b))
    return same.reshape(len(same), -1).all(axis=1)


def _names():
    from oracle import probes as module
    return [n for n in module.CASES if n.split("_")[0] in ("box", "primitive", "closest", "shadow", "shader", "launch",
                                                           "post", "vectors", "make", "skybox", "intersection")]


def _columns(out):
    """a pixel's four id words are judged one by one (the emissive word may be under a switch where the primitive is not)"""
    flat = {}
    for key, value in out.items():
        if key == "ids":
            for c, word in enumerate("xyzw"):
                flat["ids." + word] = value[:, c]
        elif key == "bitmap":
            flat[key] = np.asarray(value).reshape(-1, 3)
        elif key != "features":
            flat[key] = value
    return flat


# engine against the REFERENCE where no dialect statement shows: bit for bit, but for the two outputs the library pow of
# the Blinn term reaches (RayTracer.cl:1761 - OCML's, within 2 ULP of glibc's; the engine rounds a binary64 pow once)
POW_ULPS = {"total_blinn": 4, "color": 3}
COVERAGE = {}


def _held_to_the_reference(probes, name, label, case, out, ref, cuda, cl):
    """the switch-observability mask: per output, the elements on which the oracle's two dialects agree; engine ==
    reference there.  Returns {output: (covered fraction, elements)}"""
    mine, theirs, a, b = _columns(out), _columns(ref), _columns(cuda), _columns(cl)
    covered = {}
    # what a test or a walk leaves in its outputs on a miss is nobody's business (in/out locals of the caller)
    found = None
    if case["name"] in ("primitive", "closest"):
        found = (mine["hit"] != 0) & (theirs["hit"] != 0)
        if "primitive" in mine:
            found &= mine["primitive"] == theirs["primitive"]
    for key in a:
        if key not in mine or key not in theirs:
            continue
        agree = _rows_equal(probes, a[key], b[key])
        if found is not None and key not in ("hit", "primitive"):
            agree &= found
        what = "%s (%s) %s vs the reference where the dialects agree" % (name, label, key)
        if key in POW_ULPS and case["name"] in ("shader", "launch"):
            # (two library pows differ in the last bit on some 9 % of the arguments; a pixel's colour keeps that on < 3 % of a bright frame, 3.2 % of the dimly lit mix under one lamp)
            u = ulp_distance(mine[key], theirs[key]).reshape(len(agree), -1).max(axis=1)
            assert (u[agree] <= POW_ULPS[key]).all(), (what, int(u[agree].max()))
            if key == "color" and agree.any():
                assert (u[agree] > 0).mean() <= 0.05, (what, float((u[agree] > 0).mean()))
        else:
            _all_equal(probes, what, mine[key], theirs[key], agree)
        covered[key] = (float(agree.mean()), int(agree.sum()))
    COVERAGE.setdefault(name, covered)
    return covered


def _all_equal(probes, what, mine, theirs, where=None):
    eq = _rows_equal(probes, mine, theirs)
    if where is not None:
        eq = eq | ~where
    assert eq.all(), "%s: %d of %d elements differ (first: %d)" % (what, int((~eq).sum()), len(eq), int(np.flatnonzero(~eq)[0]))


def _variants(case):
    if case["name"] in ("closest", "shadow", "shader", "launch"):
        return [("the renderer's instantiation, walk-order + order-free lists", 0, 0),
                ("the renderer's instantiation, the reference's own list", 0, 1),
                ("all-features instantiation", E.EVERYTHING, 0)]
    if case["name"] == "primitive":
        return [("the renderer's instantiation", 0, 0), ("all-features instantiation", E.EVERYTHING, 0)]
    return [("", 0, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names())
def test_engine_functions_reproduce_the_reference_functions(solr, probes, oracle, fixture, name):
    case, ref = _load(probes, fixture, name)
    if "renderer" in ref or not ref:                            # the post-processing kernels ran as they are
        ref = {k.split("/")[2]: fixture[k] for k in fixture.files if k.startswith(name + "/renderer/")}
    cuda, cl = probes.both_dialects(case)                        # the oracle's CUDA dialect: only where a switch applies
    assert oracle.lib().oracle_get_dialect() == 0
    kind = case["name"]
    for label, features, exact in _variants(case):
        out = E.engine_outputs(solr, case, features=features, exact=exact)
        what = "%s (%s)" % (name, label)
        covered = _held_to_the_reference(probes, name, label, case, out, ref, cuda, cl)
        print("%-28s %-62s held to the reference's output on: %s" % (
            name, label, ", ".join("%s %.3f" % (k, v[0]) for k, v in covered.items())))
        if kind == "box":
            no_zero = (case["directions"] != 0).all(axis=1)
            near0 = case["t0"] == 0
            assert no_zero.sum() > 400 and (no_zero & near0).sum() > 150 and (~no_zero).sum() > 100
            for key in ("hit", "hit_fast"):
                assert (out[key] >= 0).all()                      # every ray of the case meets the sign-free form's precondition
                _all_equal(probes, what + " " + key + " vs the reference", out[key], ref["hit"], no_zero)
                _all_equal(probes, what + " " + key + " vs the CUDA dialect", out[key], cuda["hit"])
            for key in ("hit_walk", "hit_walk_deep"):             # the node loop tests [0, far): its only form in both walks
                _all_equal(probes, what + " " + key + " vs the reference", out[key], ref["hit"], no_zero & near0)
                _all_equal(probes, what + " " + key + " vs the CUDA dialect", out[key], cuda["hit"], near0)
            assert 0.05 < ref["hit"].mean() < 0.95
        elif kind == "primitive":
            types = case["prims"]["type"]
            triangle = (types == ptTriangle) | (case["si"].extendedGeometry == 0)
            # switch 10: with double-sided triangles the CUDA text's dangling else makes every shadow test miss and keeps
            # every other hit (GI:638-648); the OpenCL engine rejects by the side the ray comes from (CL:1379-1394)
            switch10 = triangle & (case["si"].doubleSidedTriangles != 0)
            _all_equal(probes, what + " hit", out["hit"], ref["hit"], ~switch10)
            hit = (out["hit"] != 0) & (ref["hit"] != 0)
            assert hit.sum() > 0.15 * len(hit)
            _all_equal(probes, what + " hit point", out["intersection"], ref["intersection"], hit)
            _all_equal(probes, what + " shadow intensity", out["shadow"], ref["shadow"], hit)
            _all_equal(probes, what + " normal", out["normal"], ref["normal"], hit & ~triangle)
            _all_equal(probes, what + " areas", out["areas"], ref["areas"], hit & ~triangle)
            if case["si"].extendedGeometry:
                assert (hit & ~triangle).sum() > 500
            for key in ("hit", "intersection", "normal", "areas", "shadow"):     # ... and the CUDA dialect everywhere
                _all_equal(probes, what + " %s vs the CUDA dialect" % key, out[key], cuda[key],
                           None if key == "hit" else (out["hit"] != 0) & (cuda["hit"] != 0))
        elif kind == "closest":
            s = case["scene"]
            agree = (out["hit"] == ref["hit"]) & ((out["primitive"] == ref["primitive"]) | (out["hit"] == 0))
            if name == "closest_mix":
                assert agree.mean() > 0.9                          # the cone is not in the OpenCL engine's dispatch (switch 11)
            else:
                assert agree.all(), (what, int((~agree).sum()))
            hit = agree & (out["hit"] != 0)
            assert hit.sum() > 100
            prim_type = s.prims["type"][np.clip(out["primitive"], 0, len(s.prims) - 1)]
            triangle = (prim_type == ptTriangle) | (case["si"].extendedGeometry == 0)
            _all_equal(probes, what + " hit point", out["intersection"], ref["intersection"], hit)
            _all_equal(probes, what + " normal", out["normal"], ref["normal"], hit & ~triangle)
            _all_equal(probes, what + " areas", out["areas"], ref["areas"], hit & ~triangle)
            if name in ("closest_cornell", "closest_sticks"):
                assert not triangle[hit].any()                     # nothing of these two cases is under a switch
            for key in ("hit", "primitive", "intersection", "normal", "areas"):
                _all_equal(probes, what + " %s vs the CUDA dialect" % key, out[key], cuda[key],
                           None if key == "hit" else (out["hit"] != 0) & (cuda["hit"] != 0))
        elif kind == "shadow":
            # three switches in this one function: the CUDA dialect everywhere, the reference where they do not show
            # (_held_to_the_reference above).  The reference's probe leaves out the lamp only; so does this call, except
            # in the moot cases, which name the shaded primitive and are probed the way the renderer calls the walk.
            _all_equal(probes, what + " result vs the CUDA dialect", out["result"], cuda["result"])
            _all_equal(probes, what + " colour vs the CUDA dialect", out["color"], cuda["color"])
            assert 0.02 < (out["result"] > 0).mean() < 0.95
            assert covered["result"][0] > 0.8 and covered["color"][0] > 0.85
            if "shaded" in case:
                assert covered["result"][0] == 1.0 and covered["color"][0] == 1.0, covered
        elif kind == "shader":
            # engine == the oracle's CUDA dialect on every element: bit for bit, but for the Blinn sum (the oracle as
            # pinned takes glibc's powf, within 1 ULP of the power; the engine the power rounded once)
            for key in ("returned", "shadow", "normal", "closest_color", "attributes"):
                _all_equal(probes, what + " %s vs the CUDA dialect" % key, out[key], cuda[key])
            u = ulp_distance(out["total_blinn"], cuda["total_blinn"]).max(axis=1)
            assert u.max() <= 2 and (u > 0).mean() <= 0.02, (what, int(u.max()), float((u > 0).mean()))
            assert (out["total_blinn"] > 0).any()
            if case["si"].graphicsLevel > 3 and "triangles" not in name:
                assert (out["shadow"] > 0).mean() > 0.02           # shadow rays were traced and met occluders
            if name.endswith("_moot"):
                assert all(v[0] == 1.0 for v in covered.values()), covered
        elif kind == "launch":
            # the frame as k_standardRenderer renders it against the oracle's CUDA dialect: the bar of every parity test
            assert np.array_equal(out["ids"], cuda["ids"]), what
            _all_equal(probes, what + " depth vs the CUDA dialect", out["depth"], cuda["depth"])
            u = ulp_distance(out["color"], cuda["color"]).max(axis=1)
            assert u.max() <= 2 and (u > 1).sum() <= 2, (what, int(u.max()), int((u > 1).sum()))
            assert (out["ids"][:, 0] >= 0).mean() > 0.2
        elif kind == "post":
            _all_equal(probes, what + " bitmap vs the CUDA dialect", out["bitmap"].reshape(-1, 3), cuda["bitmap"].reshape(-1, 3))
            if case["ppi"].type == 0 or name.endswith("_moot"):
                # k_default is under no switch; nor is k_depthOfField once the random buffer repeats every 900 values
                assert covered["bitmap"][0] == 1.0, covered
        elif kind == "intersection_shader":
            sphere = case["prims"]["type"] == ptSphere
            for key in ("color", "bump", "advanced", "attributes"):
                _all_equal(probes, what + " " + key, out[key], ref[key])
            _all_equal(probes, what + " specular", out["specular"], ref["specular"], ~sphere)      # switch 2: specularMap
            _all_equal(probes, what + " specular vs the CUDA dialect", out["specular"], cuda["specular"])
            assert (~sphere).sum() > 300
        else:   # skybox, vectors, make_color
            for key, value in out.items():
                if key != "features":
                    _all_equal(probes, what + " " + key, value, ref[key])


@pytest.mark.gpu
def test_coverage_of_the_reference_pin_per_function(solr, probes, oracle, fixture):
    """(runs after the cases above) DESIGN.md section 2.4's table: per function, the fraction of the fixture's elements
    on which the engine was held to the reference's own output directly"""
    if not COVERAGE:
        pytest.skip("the cases did not run in this session")
    for name, covered in COVERAGE.items():
        print("%-30s %s" % (name, ", ".join("%s %.1f %% of %d" % (k, 100 * v[0], round(v[1] / max(v[0], 1e-9)))
                                            for k, v in covered.items())))
    for name in ("shadow_cornell_opaque_moot", "shader_cornell_opaque_moot"):
        if name in COVERAGE:
            assert all(v[0] == 1.0 for v in COVERAGE[name].values())


@pytest.mark.gpu
def test_the_probes_run_the_instantiations_the_renderer_launches(solr, probes, fixture):
    """features = 0 picks renderImpl's row for the resident scene: the lean sphere + plane kernel for the Cornell room,
    sphere + cylinder for the sticks, sphere + triangle for the meshes, everything for the mixed and textured scenes"""
    expect = {"closest_cornell": E.F_SPHERE | E.F_PLANE, "closest_sticks": E.F_SPHERE | E.F_CYL,
              "closest_triangles": E.F_SPHERE | E.F_TRI, "closest_mix": E.EVERYTHING, "closest_textured": E.EVERYTHING}
    for name, features in expect.items():
        case, _ = _load(probes, fixture, name)
        assert E.engine_outputs(solr, case)["features"] == features, name


def test_all_twenty_two_probe_entry_points_are_exported(solr):
    """(CPU) include/solr_hip_probes.h is test-only, but what it declares must be in the library: the eighteen probes of the
    device functions and of a frame - sixteen of the device functions (two of them the math stand-ins per element, scalar
    and vector; one the shader with the hit's records handed over) and the read-back tickets, two of the frame's launch
    (the tile sort, the last frame) - the two of the resident lists (their copies read back, what a walk is offered) and
    the two of the list builders on a node list of the caller's (the order-free lists, the prune decisions): twenty-two.
    And nothing of the product calls the last two: they are named in their own unit alone."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "solr_hip_probes.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(solr_hip_probe_\w+)\s*\(", text)))
    assert len(names) == 22
    assert names == sorted("solr_hip_probe_" + n for n in (
        "box", "box_walk", "primitive", "closest", "shadow", "shader", "shader_given", "postprocess", "ticket", "image_serial",
        "vectors", "make_color", "skybox", "intersection_shader", "order_tiles", "last_frame", "list_copy", "walk_offer", "free_lists",
        "prune_list", "math", "vector_math")), names
    hip = solr.hip_lib()
    assert all(hasattr(hip, n) for n in names), [n for n in names if not hasattr(hip, n)]
    csrc = os.path.join(root, "sol-r_amd", "csrc")
    for unit in sorted(os.listdir(csrc)):
        if unit.endswith((".hip", ".cpp", ".h", ".py")) and unit != "solr_probes.hip":
            source = open(os.path.join(csrc, unit), errors="replace").read()
            assert "solr_hip_probe_free_lists" not in source and "solr_hip_probe_prune_list" not in source, unit
