"""The texture mappers' cases and their model, held on the CPU (no GPU).

tests/texture_mapper_model.py restates the reference's texture tier from its text; tests/texture_mapper_cases.py steers it to
the texel edges.  Here:
  * every generator reaches the edges it claims, counted per edge on the model's trace (EXPECT), and the counts that follow
    from the generators alone are written down (PINNED: the rows of a tall texture that TM:398's `v < W` leaves to the
    material's colour, the elements whose conversion saturates, the elements that convert a NaN);
  * every byte index the model computes lies inside the atlas and every table passes the engine's rule (asserted inside
    texture_mapper_model.run, so a case that breaks either fails here, on the CPU);
  * on the sphere and skybox cases the model's texel is never more than one texel away, cyclically, from the texel of the
    exact U, V (mpmath from the binary32 hit point, no intermediate rounding);
  * the C oracle in its CUDA dialect with rounded transcendentals equals the model bit for bit on every output of every
    element (NaN as NaN; an ambiguous element may take either neighbour);
  * at most 0.1 % of the sphere and skybox elements are ambiguous (none is expected);
  * each of twelve wrong restatements of one statement (texture_mapper_model.VARIANTS) differs from the oracle on at least
    one element: the cases can tell such a kernel from a right one.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import texture_mapper_cases as TC  # noqa: E402
import texture_mapper_model as T  # noqa: E402

AMBIGUITY_CAP = 1e-3

# counts that follow from the generators alone (measured on the model, which the oracle then confirms element by element)
PINNED = {
    "cube": {"blanked_row": 224, "elements with saturated": 40},
    "checker_far": {"elements with saturated": 14, "elements with nan": 4},
    "checker_near": {"elements with saturated": 14, "elements with nan": 4},
    "triangle": {"elements with saturated": 20, "elements with nan": 14},
    "triangle_zero_width": {"elements with nan": 2, "zero_width": 8},
    "scroll_t2147483647": {"elements with saturated": 12},
    "planes_lean": {"elements with saturated": 72},
    "fractal_t3_i1": {"blanked_row": 32, "fractal_nan": 18},
}


@pytest.fixture
def rounded_oracle(solr, oracle):
    with TC.rounded_oracle(oracle) as L:
        yield L


@pytest.mark.parametrize("name", TC.names())
def test_every_generator_reaches_the_edges_it_steers(solr, name):
    reached = TC.edges(name)
    print(name, {k: v for k, v in sorted(reached.items())})
    assert name in TC.EXPECT or name.startswith(("skybox", "mix_interleaved")), name
    for edge in TC.EXPECT.get(name, ()):
        assert reached.get(edge, 0) > 0, (name, edge)
    for edge, count in PINNED.get(name, {}).items():
        assert reached.get(edge, 0) == count, (name, edge, reached.get(edge, 0))


def test_a_tall_texture_keeps_only_its_first_w_rows_in_the_cube_mapper(solr):
    """TM:398 compares v with the mapping's WIDTH: of a 3 x 7 texture's 21 texels the 12 of rows 3 ... 6 show the material's
    colour, of a 1 x 5 texture's 5 texels the 4 of rows 1 ... 4; a wide texture loses none"""
    case = TC.case("cube")
    _, traces, _ = TC.model_outputs("cube")
    w = case["world"]
    for shape, blanked in (((3, 7), 12), ((1, 5), 4), ((7, 3), 0), ((5, 1), 0), ((2, 2), 0)):
        m = w.mat["diffuse", shape, 3]
        mine = [t for t, k, p in zip(traces, case["kind"], case["prims"])
                if k == "cube centre" and p["materialId"] == m and p["type"] == T.ptXYPlane]
        assert len(mine) == shape[0] * shape[1]
        assert sum(1 for t in mine if t["notes"].get("blanked_row")) == blanked, shape
        assert sum(1 for t in mine if t["fetched"]) == shape[0] * shape[1] - blanked, shape


def test_tables_and_atlas(solr):
    w = TC.world()
    w.check_tables(range(len(w.materials)))
    # the smaller secondary maps lie in front of larger textures: at the diffuse index they run past their own end
    m = w.material(w.mat["small", (7, 3)])
    assert all(w.own_texels[m["id"]][t] == 12 < 63 for t in range(1, 7))
    assert T.crem(-7, 3) == -1 and T.crem(7, -3) == 1 and T.wrap(2 ** 31) == T.INT_MIN
    model = T.Model(w)
    assert [model.to_int(x) for x in (np.float32(-2.9), np.float32(np.nan), np.float32(3e9), np.float32(-np.inf))] == \
        [-2, 0, T.INT_MAX, T.INT_MIN]


def test_the_checkerboard_never_hides_the_sign_of_p0_z(solr):
    """TM:390 ADDS p0.z: no checkerboard or XZ plane of a cube-mapped case may have p0.z == 0"""
    for name in ("cube", "planes_textured", "mix_sorted"):
        case = TC.case(name)
        p = case["prims"]
        sel = np.isin(p["type"], (T.ptCheckboard, T.ptXZPlane)) & (case["materials"]["textureIds"][p["materialId"]][:, 0] != -1)
        assert sel.any() and (p["p0"][sel][:, 2] != 0).all(), name


def test_the_wave_mix_deals_every_mapper_into_every_wave(solr):
    a, b = TC.case("mix_sorted"), TC.case("mix_interleaved")
    order = TC.mix_order(a["kind"])
    assert [a["kind"][i] for i in order] == b["kind"]
    for key in ("inter", "areas", "attributes"):
        assert np.array_equal(a[key][order], b[key], equal_nan=True)
    _, traces, _ = TC.model_outputs("mix_interleaved")
    n = len(traces)
    for wave in range(n // 64):
        lanes = traces[64 * wave: 64 * wave + 64]
        mappers = {t["mapper"] for t in lanes}
        assert {"cube", "triangle", "sphere", "checker"} <= mappers, (wave, mappers)
        assert any(t.get("fractal") for t in lanes), wave
        assert any(t["mapper"] != "checker" and not t["fetched"] for t in lanes), wave
    mine, _, _ = TC.model_outputs("mix_sorted")
    theirs, _, _ = TC.model_outputs("mix_interleaved")
    for key in mine:
        assert TC.rows_equal(mine[key][order], theirs[key]).all(), key


@pytest.mark.parametrize("name", [n for n in TC.names() if n.startswith(("sphere", "skybox")) and n != "skybox_3"])
def test_the_model_stays_within_one_texel_of_exact_geometry(solr, name):
    case = TC.case(name)
    _, traces, _ = TC.model_outputs(name)
    w = case["world"]
    checked, off_by_one = 0, 0
    for e, t in enumerate(traces):
        if "I" not in t:
            continue
        if name.startswith("sphere"):
            p = case["prims"][e]
            m = w.material(int(p["materialId"]))
            exact = T.exact_texel(case["inter"][e], m["W"], m["H"], p["vt1"][0], p["vt1"][1], centre=p["p0"])
        else:
            m = w.material(int(case["si"].skyboxMaterialId))
            exact = T.exact_texel(t["I"], m["W"], m["H"])
        du, dv = T.cyclic_distance(t["u"], exact[0], m["W"]), T.cyclic_distance(t["v"], exact[1], m["H"])
        assert du <= 1 and dv <= 1, (name, e, case["kind"][e], (t["u"], t["v"]), exact)
        checked += 1
        off_by_one += (du + dv) > 0
    print("%s: %d elements against exact geometry, %d one texel off" % (name, checked, off_by_one))
    assert checked >= len(traces) // 2


def test_ambiguity_cap(solr):
    names = [n for n in TC.names() if n.startswith(("sphere", "skybox"))]
    total = sum(len(TC.model_outputs(n)[1]) for n in names)
    ambiguous = sum(TC.edges(n).get("ambiguous", 0) for n in names)
    print("ambiguous elements: %d of %d (sphere and skybox cases)" % (ambiguous, total))
    assert ambiguous <= AMBIGUITY_CAP * total
    for n in TC.names():                     # (the fractals' sin and cos are counted with their own cases)
        assert TC.edges(n).get("ambiguous", 0) <= AMBIGUITY_CAP * len(TC.model_outputs(n)[1]), n


@pytest.mark.parametrize("name", [n for n in TC.names() if n not in TC.NOT_FOR_THE_ORACLE])
def test_the_oracle_equals_the_model_bit_for_bit(solr, rounded_oracle, name):
    case = TC.case(name)
    assert case["oracle"]
    model, _, alternatives = TC.model_outputs(name)
    theirs = TC.oracle_outputs(rounded_oracle, case)
    bad = TC.differing(case, model, alternatives, theirs)
    assert len(bad) == 0, "%s: %d of %d elements differ; first %d (%s)" % (name, len(bad), len(case["kind"]), bad[0],
                                                                       case["kind"][bad[0]])


@pytest.mark.parametrize("variant", T.VARIANTS)
def test_the_cases_tell_a_wrong_restatement_from_the_right_one(solr, rounded_oracle, variant):
    """a model with ONE statement restated wrongly differs from the oracle on at least one element of at least one case"""
    told = {}
    for name in TC.names():
        case = TC.case(name)
        if not case["oracle"] or name.startswith("mix"):
            continue
        wrong, _, alternatives = T.run(case, case["world"], variant)
        bad = TC.differing(case, wrong, alternatives, TC.oracle_outputs(rounded_oracle, case))
        if len(bad):
            told[name] = len(bad)
    print(variant, told)
    assert told, variant


def test_the_oracle_is_left_as_it_was_found(solr, oracle):
    """(the last test of the file: the fixture above has put the pinned setting back)"""
    assert oracle.lib().oracle_get_dialect() == 0 and not oracle.lib().oracle_get_rounded_transcendentals()
    assert all(TC.case(n)["oracle"] == (n not in TC.NOT_FOR_THE_ORACLE) for n in TC.names())
