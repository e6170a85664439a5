"""The cases of tests/shader_edge_cases.py are worth comparing (CPU): on every element of them

  * the oracle in dialect 0, as pinned, gives the bits of the independent reading of the CUDA text (tests/cuda_text_model.py
    primitive_shader / process_shadows) - returned colour, shadow intensity, normal, closestColor, totalBlinn and attributes
    of the shader; result and colour of the shadow sum.  No element is left out and there is no tolerance: the power families
    hold only pairs whose power is a binary32 number, on which glibc's powf and the model's pow agree by arithmetic;
  * every family holds both outcomes by the model, and a family that claims an equality holds an element ON it: its
    strictness mutant differs from the model on an element of the family (it can differ nowhere else);
  * every wrong restatement in MUTANTS is told apart from the model by some element; the list of names is pinned;
  * the decisions no binary32 input can reach are listed in UNREACHABLE with the argument: not built, not counted;
  * the generator is deterministic: families, elements and a digest of the inputs are pinned (and checked again on the GPU,
    tests/test_shader_edges_gpu.py).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cuda_text_model as M  # noqa: E402
import shader_edge_cases as G  # noqa: E402
import text_mutants  # noqa: E402

F = np.float32
GROUP_NAMES = tuple(G.GROUPS)
SHADER_KEYS = ("returned", "shadow", "normal", "closest_color", "total_blinn")
NOT_RESET = 0.75         # what shadowIntensity holds when the shader is entered: the text sets it to 0 (GI:935)


# ---- the model over the cases --------------------------------------------------------------------------------------------------
def model_outputs(case, only=None):
    """per element, by the text model: (returned, shadow, normal, closestColor, totalBlinn) of a shader case, (result, colour) of
    a shadow case; an element on which a MUTANT leaves the domain of Python's pow gives the exception's name"""
    if case.get("_model") is None:
        case["_model"] = G.TextScene(case["scene"])          # (not an array: no part of the digest)
    s, si = case["_model"], case["si"]
    out = {}
    with np.errstate(all="ignore"):
        for e in (range(len(case["origins"])) if only is None else only):
            try:
                if case["name"] == "shader":
                    st = M.ShaderState()
                    st.closest_color = [F(x) for x in case["closest_color"][e]]
                    st.total_blinn = [F(x) for x in case["total_blinn"][e]] + [F(case["attributes"][e][1])]
                    st.shadow_intensity = F(NOT_RESET)
                    color, normal = M.primitive_shader(si, s, int(case["index"][e]), M.v(*case["origins"][e]), M.v(*case["normal"][e]),
                                                       int(case["object_id"][e]), M.v(*case["inter"][e]), int(case["iteration"][e]), st)
                    out[e] = (color, st.shadow_intensity, normal, tuple(st.closest_color), tuple(st.total_blinn[:3]))
                else:
                    out[e] = M.process_shadows(si, s, M.v(*case["lamps"][e]), M.v(*case["origins"][e]), int(case["object_id"][e]),
                                               int(case["iteration"][e]), int(case["shaded"][e]))
            except (ValueError, OverflowError) as error:
                out[e] = (type(error).__name__,)
    return out


def _same(a, b):
    """the same bits - +0 is not -0 here: the families step through both - or both no number"""
    if isinstance(a, str) or isinstance(b, str):
        return a == b
    a, b = np.atleast_1d(np.array(a, F)), np.atleast_1d(np.array(b, F))
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def outcomes_equal(x, y):
    return len(x) == len(y) and all(_same(a, b) for a, b in zip(x, y))


# ---- mutants of the model: name -> (function, text, replacement, which occurrence).  Strictness mutants first. --------------------
_SATURATE = "cc[:] = saturate(cc)\n%sst.total_blinn[:] = saturate(st.total_blinn)\n    else:"
_TINT = '                                for q in range(3):\n' \
        '                                    color[q] = color[q] + ratio * (F(0.3) - F(0.3) * m["color"][q])\n' \
        '                            result = result + ratio\n'
_TINT_LATE = '                                tint = True\n' \
             '                            else:\n' \
             '                                tint = False\n' \
             '                            result = result + ratio\n' \
             '                            if tint and result < limit:\n' \
             '                                for q in range(3):\n' \
             '                                    color[q] = color[q] + ratio * (F(0.3) - F(0.3) * m["color"][q])\n'
S, W = "primitive_shader", "process_shadows"
MUTANTS = {
    "range <": (S, 'if light_ray_length < lm["illum"][2]:', 'if light_ray_length <= lm["illum"][2]:', None),
    "lambert > 0": (S, "if lambert > F(0) and", "if lambert >= F(0) and", None),
    "iteration < 4": (S, "and iteration < 4 and", "and iteration <= 4 and", None),
    "wireframe == 1": (S, 'if m["attributes"][2] == 1:', "if False:", None),
    "Blinn gate <": (S, "st.shadow_intensity < F(si.shadowIntensity):", "st.shadow_intensity <= F(si.shadowIntensity):", None),
    "temp != 0": (S, "if temp != F(0):", "if True:", None),
    "shadow exit <": (W, "result < limit and", "result <= limit and", "all"),
    "pass >= 10 (the lamp choice)": (S, "si.pathTracingIteration >= NB_MAX_ITERATIONS", "si.pathTracingIteration > NB_MAX_ITERATIONS", 0),
    "pass >= 10 (the jitter)": (S, "si.pathTracingIteration >= NB_MAX_ITERATIONS", "si.pathTracingIteration > NB_MAX_ITERATIONS", 1),
    "graphicsLevel > 3": (S, "si.graphicsLevel > 3", "si.graphicsLevel >= 3", None),
    "graphicsLevel > 1": (S, "si.graphicsLevel > 1", "si.graphicsLevel >= 1", None),
    "graphicsLevel > glNoShading": (S, "    if si.graphicsLevel > glNoShading:\n        for k in range(3):",
                                    "    if si.graphicsLevel >= glNoShading:\n        for k in range(3):", None),
    # ---- the equalities: their opposite, or the clause dropped
    "lit: != dropped": (S, 'if li["prim"] != p["index"]:', "if True:", None),
    "innerIllumination.x == 0 dropped": (S, ' and m["illum"][0] == F(0):', ":", None),
    "noise: != read as ==": (S, 'if m["illum"][3] != F(0):', 'if m["illum"][3] == F(0):', None),
    "lamp material: != read as ==": (S, 'if li["mat"] != MATERIAL_NONE:', 'if li["mat"] == MATERIAL_NONE:', None),
    "shadow: transparency != 0 dropped": (W, 'if m["transparency"] != F(0):', "if True:", None),
    "wireframe: == 1 read as >= 1": (S, 'if m["attributes"][2] == 1:', 'if m["attributes"][2] >= 1:', None),
    # ---- wrong restatements that are no change of a comparison
    "lambert < 0: the transparency dropped": (S, '((-m["transparency"]) if lambert < F(0) else F(1))', "F(1)", None),
    "blinnTerm < 0: the clamp dropped": (S, "term = F(0) if term < F(0) else term", "term = term", None),
    "lamp 0 instead of pass % nbLights": (S, "(si.pathTracingIteration % n_lights) if", "0 if", None),
    "the lamp loop run once": (S, "for cpt in range(n_lights):", "for cpt in range(min(n_lights, 1)):", None),
    "saturation after the loop": (S, "            " + _SATURATE % "            ", "        " + _SATURATE % "        ", None),
    "shadowIntensity not reset to 0": (S, "    st.shadow_intensity = F(0)\n", "", None),
    "the shadow colour added": (S, "- shadow_color[k])", "+ shadow_color[k])", None),
    "the Blinn gate dropped": (S, " and st.shadow_intensity < F(si.shadowIntensity):", ":", None),
    "the early exit tested per node only": (W, 'while result < limit and k < box["n"]:', 'while k < box["n"]:', None),
    "the coloured shadow added after the exit test": (W, _TINT, _TINT_LATE, None),
    "final clamp: max(0, .) dropped": (W, "result = max(F(0), min(result, limit))", "result = min(result, limit)", None),
    "final clamp: min(., limit) dropped": (W, "result = max(F(0), min(result, limit))", "result = max(F(0), result)", None),
}

# Decisions that no binary32 input can reach, or whose two sides give the same bits, with the argument: not built, not counted.
UNREACHABLE = {
    "photonEnergy > 1": "inside the range test lightRayLength < innerIllumination.z, so the quotient is below 1 (a correctly rounded "
                        "quotient of a < b is at most 1, and 1 only when b - a is below half an ulp - then sqrt gives 1, not more); a "
                        "correctly rounded root of a number <= 1 is <= 1",
    "photonEnergy < 0": "the root of a quotient of a length (>= 0) and a number above it; a NaN compares false",
    "lambert < 0 (strictness)": "at lambert == 0 both sides give +-0; times the lamp's strength, the noise and 1 - shadow it stays +-0, and "
                                "adding backgroundColor.w (+0 or above in every group) gives the same number",
    "blinnTerm < 0 (strictness)": "at blinnTerm == +-0 both sides hand pow a zero; for the exponents built (0 ... above 4096) the power of -0 "
                                  "is +-0 or 1 like that of +0, and totalBlinn + (+-0) is totalBlinn",
    "graphicsLevel > glNoShading (inner, GI:1000)": "inside the outer test of the same comparison",
    "shadow: transparency == 0 ? 1 : 1 - transparency (GI:887)": "inside transparency != 0",
    "lamp loop: nbLights == 0": "pass % nbLights divides by zero from pass 10 on, and below it the loop body never runs: no stage has an "
                                "empty light list",
}


def mutant(name):
    return text_mutants.mutant(MUTANTS, name)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def evaluated(solr, oracle):
    """per group: [(case, families, the oracle's outputs in dialect 0 as pinned, the model's outcomes)] - computed once"""
    from oracle import probes
    L = oracle.lib()
    assert L.oracle_get_dialect() == 0 and L.oracle_get_rounded_transcendentals() == 0
    return {group: [(case, fams, probes._oracle_outputs(L, case), model_outputs(case)) for case, fams, _ in G.cases(solr, group)]
            for group in GROUP_NAMES}


def _oracle_element(case, got, e):
    if case["name"] == "shader":
        return tuple(got[k][e] for k in SHADER_KEYS)
    return (got["result"][e], got["color"][e])


# ---- the tests --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUP_NAMES)
def test_the_oracle_equals_the_text_model_on_every_element(evaluated, group):
    bad, total = [], 0
    for case, fams, got, want in evaluated[group]:
        n = len(case["origins"])
        total += n
        assert len(want) == n
        for e in range(n):
            mine = _oracle_element(case, got, e)
            keys = SHADER_KEYS if case["name"] == "shader" else ("result", "color")
            bad += [(fams[case["family"][e]].decision, e, k) for k, a, b in zip(keys, mine, want[e]) if not _same(a, b)]
        if case["name"] == "shader":       # an untextured material leaves the attributes alone
            assert np.array_equal(got["attributes"].view(np.uint32), case["attributes"].view(np.uint32)), case["key"]
    print("%s: %d elements in %d cases, %d outputs differ" % (group, total, len(evaluated[group]), len(bad)))
    assert not bad, bad[:20]


def _family_elements(evaluated_group, j):
    """[(case, want, elements)] of family j"""
    out = []
    for case, fams, got, want in evaluated_group:
        es = np.flatnonzero(case["family"] == j)
        if len(es):
            out.append((case, want, es))
    return out


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_every_family_holds_both_outcomes(evaluated, group):
    fams = evaluated[group][0][1]
    single = []
    for j, fam in enumerate(fams):
        seen = []
        for case, want, es in _family_elements(evaluated[group], j):
            for e in es:
                if not any(outcomes_equal(want[e], x) for x in seen):
                    seen.append(want[e])
        if len(seen) < 2:
            single.append(fam.decision)
    assert not single, single


EQUALITIES = {"dyadic": 13, "dyadic half": 13}


@pytest.mark.parametrize("group", ["dyadic", "dyadic half"])
def test_a_family_aimed_at_an_equality_holds_an_element_on_it(evaluated, group):
    """... by the model's own arithmetic: its strictness mutant differs from the model on an element of the family"""
    fams = evaluated[group][0][1]
    missing, found = [], 0
    for j, fam in enumerate(fams):
        if not fam.equality:
            continue
        differs = False
        for case, want, es in _family_elements(evaluated[group], j):
            with mutant(fam.equality):
                other = model_outputs(case, es)
            differs |= any(not outcomes_equal(other[e], want[e]) for e in es)
        if differs:
            found += 1
        else:
            missing.append((fam.decision, fam.equality))
    assert not missing, missing
    assert found == EQUALITIES[group], found


def test_every_mutant_is_told_apart(evaluated):
    """every wrong restatement gives another result on some element"""
    unnoticed = []
    for name in MUTANTS:
        kind = "shader" if MUTANTS[name][0] == S else None        # (a mutant of the shadow sum shows in the shader too)
        noticed = False
        for case, fams, got, want in evaluated["dyadic"] + evaluated["dyadic half"]:
            if kind and case["name"] != kind:
                continue
            with mutant(name):
                other = model_outputs(case)
            if any(not outcomes_equal(other[e], want[e]) for e in want):
                noticed = True
                break
        if not noticed:
            unnoticed.append(name)
    assert not unnoticed, unnoticed


MUTANT_NAMES = ['Blinn gate <', 'blinnTerm < 0: the clamp dropped', 'final clamp: max(0, .) dropped', 'final clamp: min(., limit) dropped',
 'graphicsLevel > 1', 'graphicsLevel > 3', 'graphicsLevel > glNoShading', 'innerIllumination.x == 0 dropped',
 'iteration < 4', 'lambert < 0: the transparency dropped', 'lambert > 0', 'lamp 0 instead of pass % nbLights',
 'lamp material: != read as ==', 'lit: != dropped', 'noise: != read as ==', 'pass >= 10 (the jitter)',
 'pass >= 10 (the lamp choice)', 'range <', 'saturation after the loop', 'shadow exit <',
 'shadow: transparency != 0 dropped', 'shadowIntensity not reset to 0', 'temp != 0', 'the Blinn gate dropped',
 'the coloured shadow added after the exit test', 'the early exit tested per node only', 'the lamp loop run once',
 'the shadow colour added', 'wireframe == 1', 'wireframe: == 1 read as >= 1']


def test_the_list_of_mutants_is_pinned():
    assert sorted(MUTANTS) == sorted(MUTANT_NAMES), sorted(set(MUTANTS) ^ set(MUTANT_NAMES))
    assert not set(UNREACHABLE) & set(MUTANTS)
    assert set(f.equality for g in GROUP_NAMES for f in G.families(g) if f.equality) <= set(MUTANTS)


# group -> (families, cases, elements, digest of the inputs)
PINNED = {'decimal': (38, 39, 1252, 'fba65c42a6ce54f646c37b13d16e73f670fc2b64'),
 'dyadic': (38, 39, 1532, '6421ae3f3be180f2b2ab34106f332c8ec28fdd66'),
 'dyadic half': (38, 39, 1316, '0c0eb88e1e9ffbcfca6da1caa91c8e184223be45')}


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_the_generator_is_deterministic(solr, group):
    import hashlib
    built = G.cases(solr, group)
    h = hashlib.sha1()
    for case, _, _ in built:
        h.update(G.digest(case).encode())
    elements = sum(len(case["origins"]) for case, _, _ in built)
    got = (len(G.families(group)), len(built), elements, h.hexdigest())
    print(group, got)
    assert got == PINNED[group]
    assert all(len(stage.prims) <= 16 for _, _, stage in built)


def test_the_cases_stay_below_twenty_thousand_elements(solr):
    assert sum(len(case["origins"]) for g in GROUP_NAMES for case, _, _ in G.cases(solr, g)) <= 20000
