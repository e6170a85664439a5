"""The iso-surface of a field of metaballs on the device (k_isoField, k_isoCount, k_isoEmit, csrc/solr_iso.hip): the cases
of tests/test_iso_surface.py through solr_hip_iso_field, solr_hip_iso_surface and solr_hip_metaballs, bit for bit against
the numpy model (tests/iso_surface_model.py); sizes that leave a wave or a workgroup part-filled; the reference's own size
against the host-only engine's loop; bad arguments; Kernel.add_metaballs and scenes.metaballs on the HIP engine.  The
engine's counter of classified cubes must advance by exactly N^3 per surface call: the kernels ran, not the loop."""
import ctypes as C

import numpy as np
import pytest

import iso_surface_model as M
from test_iso_surface import (CASES, METABALLS, METABALLS_BALLS, SIZES, assert_same_scene, assert_same_triangles,
                              bad_calls, call_field, call_surface, expected, scene_with_metaballs)

pytestmark = pytest.mark.gpu


@pytest.fixture
def hip(solr):
    lib = solr.hip_lib()
    lib.solr_hip_clear_error()
    yield lib
    assert lib.solr_hip_last_error(None, 0) == 0


def counted(hip, cubes, call):
    before = hip.solr_hip_iso_cubes()
    result = call()
    assert hip.solr_hip_iso_cubes() - before == cubes, "the cubes were not classified on the device"
    return result


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("n", SIZES)
def test_the_kernels_give_the_models_bits(solr, hip, n, case):
    grid, want_field, want = expected(solr, n, case)
    balls = np.asarray(CASES[case]["balls"], np.float32).reshape(-1, 4)
    room = np.zeros((max(len(balls), 1), 4), np.float32)
    room[:len(balls)] = balls
    fld = counted(hip, 0, lambda: call_field(solr, hip.solr_hip_iso_field, grid, balls))
    assert same_bits(fld, want_field), "%d field values differ" % (fld.view(np.uint32) != want_field.view(np.uint32)).sum()
    # two calls each (one to size, one to fetch): 2 N^3 cubes
    got = counted(hip, 2 * n ** 3, lambda: call_surface(solr, hip.solr_hip_iso_surface, grid, want_field))
    assert_same_triangles(solr, got, want, "solr_hip_iso_surface N=%d %s" % (n, case))
    got = counted(hip, 2 * n ** 3, lambda: call_surface(solr, hip.solr_hip_metaballs, grid, room, len(balls)))
    assert_same_triangles(solr, got, want, "solr_hip_metaballs N=%d %s" % (n, case))


@pytest.mark.parametrize("nb_balls", [1, 63, 64, 65])
def test_ball_counts_round_a_wave(solr, hip, nb_balls):
    """k_isoField does not stage the balls; 63 / 64 / 65 are the counts a wave-sized chunk would split at.  Ball 0 has
    radius sqrt(25) / 2 = 2.5, more than half a cell's diagonal (2.1), so it encloses a grid vertex whatever its place and
    the surface is not empty for any count; the others are small (radius below 0.9) and only add to the field"""
    rng = np.random.RandomState(nb_balls)
    balls = np.concatenate([rng.uniform(-4.0, 4.0, (nb_balls, 3)), rng.uniform(0.5, 3.0, (nb_balls, 1))],
                           axis=1).astype(np.float32)
    balls[0, 3] = 25.0
    grid = M.Grid(5)
    want_field = M.field(grid, balls)
    want = M.surface(solr, grid, want_field)
    assert same_bits(call_field(solr, hip.solr_hip_iso_field, grid, balls), want_field)
    assert len(want) > 0
    got = counted(hip, 2 * 5 ** 3, lambda: call_surface(solr, hip.solr_hip_metaballs, grid, balls, nb_balls))
    assert_same_triangles(solr, got, want, "%d balls" % nb_balls)


def test_the_all_cases_grid(solr, hip):
    grid, fld = M.Grid(15), M.all_cases_field()
    got = counted(hip, 2 * 15 ** 3, lambda: call_surface(solr, hip.solr_hip_iso_surface, grid, fld))
    assert_same_triangles(solr, got, M.surface(solr, grid, fld), "all cases")
    assert M.unbalanced_pairs(15, got) == []


def test_capacity_below_the_count_writes_only_that_many(solr, hip):
    grid, fld, want = expected(solr, 5, "merged")
    count, capacity = len(want), len(want) // 2
    out = np.full(count * 112, 0xA5, np.uint8)
    got = counted(hip, 125, lambda: hip.solr_hip_iso_surface(C.byref(grid.struct(solr)), fld.ctypes.data,
                                                             out.ctypes.data, capacity))
    assert got == count
    assert np.array_equal(out[:capacity * 112], M.bits(want[:capacity]).ravel())
    assert (out[capacity * 112:] == 0xA5).all()


def test_the_reference_size_against_the_host_loop(solr, hip):
    """N = 50, 50 balls on the scene's trajectories: the kernels against the host-only engine's C++ loops, every bit"""
    balls = solr.scenes.metaball_positions(7.5)
    grid = M.Grid(50, size=(150.0,) * 3, center=(0.0, 0.0, -2500.0), scale=(40.0,) * 3)
    host = solr.Kernel(engine="host-only")
    try:
        want_field = call_field(solr, host.L.SolRx_IsoField, grid, balls)
        want = call_surface(solr, host.L.SolRx_IsoSurface, grid, want_field)
    finally:
        host.finalize()
    assert len(want) > 100
    assert same_bits(call_field(solr, hip.solr_hip_iso_field, grid, balls), want_field)
    got = counted(hip, 2 * 50 ** 3, lambda: call_surface(solr, hip.solr_hip_metaballs, grid, balls, len(balls)))
    assert_same_triangles(solr, got, want, "N=50")
    assert M.unbalanced_pairs(50, got) == []


def test_bad_arguments_are_refused_with_the_counter_unmoved(solr):
    hip = solr.hip_lib()
    hip.solr_hip_clear_error()
    before = hip.solr_hip_iso_cubes()
    for name, call in bad_calls(solr, hip.solr_hip_iso_field, hip.solr_hip_iso_surface, hip.solr_hip_metaballs):
        assert call() == -1, name
        assert hip.solr_hip_last_error(None, 0) != 0, name
        hip.solr_hip_clear_error()
    assert hip.solr_hip_iso_cubes() == before


def test_add_metaballs_on_the_hip_engine_appends_the_models_triangles(solr, hip):
    before = hip.solr_hip_iso_cubes()
    n, got = scene_with_metaballs(solr, "hip", METABALLS_BALLS, False, **METABALLS)
    assert hip.solr_hip_iso_cubes() - before >= METABALLS["grid_size"] ** 3, "the cubes were not classified on the device"
    m, want = scene_with_metaballs(solr, "hip", METABALLS_BALLS, True, **METABALLS)
    assert n == m and n > 20
    assert_same_scene(got, want)


def test_a_frame_of_the_metaballs_scene_is_the_frame_of_the_scene_built_by_hand(solr, hip):
    """two frames of scenes.metaballs (the second after resetFrame), and the second frame's scene built by hand from the
    model's triangles: the same primitives and the same 64 x 64 image, byte for byte"""
    scenes = solr.scenes
    k = solr.Kernel(engine="hip", deterministic_seed=1)
    scenes.metaballs(k, timer=0.0, width=64, height=64)
    k.render()
    n = scenes.metaballs(k, timer=1.5, width=64, height=64)
    image, flat = k.render(), k.flat_scene()
    k.finalize()
    assert n > 100 and image.any()

    grid = M.Grid(50, size=(150.0,) * 3, center=(0.0, 0.0, -2500.0), scale=(40.0,) * 3)
    triangles = M.surface(solr, grid, M.field(grid, scenes.metaball_positions(1.5)))
    assert len(triangles) == n
    h = solr.Kernel(engine="hip", deterministic_seed=1)
    scenes.metaballs_begin(h, width=64, height=64)
    h.reset_frame()
    for t in triangles:
        p = h.add_primitive(solr.ptTriangle, t["p"][0], t["p"][1], t["p"][2], material=h.metaballs_materials["surface"])
        h.set_texture_coordinates(p, t["vt"][0], t["vt"][1], t["vt"][2])
        h.set_normals(p, t["n"][0], t["n"][1], t["n"][2])
    scenes.metaballs_surroundings(h)
    h.compact_boxes(True)
    by_hand, flat_by_hand = h.render(), h.flat_scene()
    h.finalize()
    assert_same_scene(flat, flat_by_hand)
    assert np.array_equal(image, by_hand)
