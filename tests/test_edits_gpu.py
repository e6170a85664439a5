"""Primitives set anew on the resident scene: GPUKernel::setPrimitives (SolRx_SetPrimitives, Kernel.set_primitives) with the
HIP engine runs on the device (solr_hip_set_primitives: sol-r_amd/csrc/solr_edits.hip) - one thread per record derives what
the host's setters derive and scatters it into the arena, the node lists are refitted like after a rotation - and the host
scene store follows lazily, through the one journal of the moves.

The bar: after any sequence of batches, rotations, translations and lamp moves the device holds, bit for bit, the primitive
records, the node list and the light records the host route - the setters on the host, flatten, upload:
tests/test_edits_host.py - produces; the frames rendered on the way match the oracle on the host-route scene; the host store,
once it catches up, equals the host route's; and what the engine cannot serve it refuses without changing anything."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_cases  # noqa: E402
import move_cases  # noqa: E402
from helpers import assert_parity, compare_frames, copy_frame, gpu_frame, oracle_frame  # noqa: E402
from test_moves_gpu import _light_rows, _node_rows, _oracle_on, _primitive_rows, _same_bits, _same_records  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
TRANSLATIONS = edit_cases.TRANSLATIONS


def _kernel(solr, name, engine):
    return move_cases.build(solr.Kernel(engine=engine, deterministic_seed=1), name)


_apply = edit_cases.apply


def _counters(hip):
    return (hip.solr_hip_device_rotations(), hip.solr_hip_device_translations(), hip.solr_hip_device_lamp_moves(),
            hip.solr_hip_device_edits())


def _slots(flat, batch):
    slot_of = {int(index): slot for slot, index in enumerate(flat.primitives["index"])}
    return np.array([slot_of[int(i)] for i in batch["index"]], np.int32)


def _device_route_equals_host_route(solr, oracle, name, make_steps, checked=None, flights=1):
    """the steps on the HIP engine, a frame after each; the same on the host-only engine; `checked`: the steps whose
    frames are held to the oracle (None: every one).  make_steps(flat): the steps, from the scene as flattened at the start"""
    hip = solr.hip_lib()
    k = _kernel(solr, name, "hip")
    frames = []
    try:
        hip.solr_hip_set_frames_in_flight(flights)
        lamps = move_cases.lamp_indices(k)
        start = k.flat_scene()
        steps = make_steps(start)
        checked = range(len(steps)) if checked is None else checked
        gpu_frame(k)                                   # uploads the scene
        uploaded = k.device_primitives().copy()
        order_free = hip.solr_hip_order_free_nodes()
        before = _counters(hip)
        for n, step in enumerate(steps):
            _apply(k, step, lamps)
            assert k.pending_moves() == n + 1, "%s took the host route" % step[0]
            frames.append(copy_frame(gpu_frame(k)))
            if step[0] == "edit":
                # the primitive the batch put on the stage is in the picture: a refit that did not happen would lose it
                far = edit_cases.far_index(start, name, step[1])[0]
                assert (frames[-1][1][..., 0] == far).any(), "primitive %d is not in view" % far
        served = tuple(b - a for a, b in zip(before, _counters(hip)))
        assert served == tuple(sum(1 for s in steps if s[0] == what) for what in ("rotate", "translate", "lamp", "edit"))
        assert hip.solr_hip_order_free_nodes() == order_free, "the order-free lists did not follow"
        nodes = k.device_nodes(exact=True)
        prims = k.device_primitives()
        lights = k.device_lights()
        assert k.pending_moves() == len(steps)         # reading the device does not wake the host store
        caught_up = k.flat_scene()                     # this does
        assert k.pending_moves() == 0 and k.pending_rotations() == 0
        k.compact_boxes(False)                         # flattened again: the next frame uploads the replayed scene
        fresh = copy_frame(gpu_frame(k))
        fresh_prims, fresh_lights = k.device_primitives(), k.device_lights()
        k.check(0, "the sequence")
    finally:
        hip.solr_hip_set_frames_in_flight(1)
        k.finalize()

    h = _kernel(solr, name, "host-only")
    try:
        assert move_cases.lamp_indices(h) == lamps
        for n, step in enumerate(steps):
            _apply(h, step, lamps)
            assert h.pending_moves() == 0
            if n in checked:
                _oracle_on(h, oracle, frames[n], caught_up.randoms)
        flat = h.flat_scene()
    finally:
        h.finalize()
    # the host store after its lazy replay == the host route
    assert _same_records(caught_up.boxes, flat.boxes)
    assert _same_records(caught_up.primitives, flat.primitives)
    assert _same_records(caught_up.lights, flat.lights)
    # the resident scene == what the host route would upload: all eight rows of every primitive, every node, every light
    assert _same_bits(prims, _primitive_rows(flat, uploaded))
    assert _same_bits(fresh_prims, prims)
    assert _same_bits(nodes, _node_rows(flat))
    assert len(flat.lights) >= flat.nb_lamps > 0
    assert _same_bits(lights, _light_rows(flat))
    assert _same_bits(fresh_lights, lights)
    # ... and renders the frame a fresh upload renders
    res = compare_frames(*frames[-1], *fresh)
    assert res["ids_all_equal"] and res["max_ulp"] == 0 and res["rgb_max_diff"] == 0, res


@pytest.mark.parametrize("grouping", [True, False], ids=["grouped", "ungrouped"])
@pytest.mark.parametrize("name", ["mesh", "sticks", "mix"])
def test_device_edits_equal_host_edits(solr, oracle, name, grouping):
    """three batches - of 65, 257 and all 289 records with normals and texture coordinates on the mesh, of 1, 65 and all on
    the sticks, of 1, 7 and all on the mix -, a frame after each"""
    hip = solr.hip_lib()
    hip.solr_hip_set_variant(0 if grouping else 5)      # 5: no grouping nodes, from the next upload on
    try:
        _device_route_equals_host_route(solr, oracle, name, lambda flat: edit_cases.batch_steps(flat, name))
    finally:
        hip.solr_hip_set_variant(0)


@pytest.mark.parametrize("flights", [1, 3], ids=["one_frame", "three_in_flight"])
def test_edits_rotations_translations_and_a_lamp_move_mixed(solr, oracle, flights):
    """one journal, in order"""
    _device_route_equals_host_route(solr, oracle, "sticks", edit_cases.mixed_steps, checked=edit_cases.MIXED_CHECKED, flights=flights)


def test_a_long_sequence_with_edits_is_replayed_not_fetched(solr, oracle):
    """more than eight rotations: without an edit the store would take the primitives from the device, which hands back
    neither sizes nor texture coordinates nor the primitive the store believes unmovable - the mix's, edited by the last
    batch.  A journal that holds an edit is replayed"""
    _device_route_equals_host_route(solr, oracle, "mix", edit_cases.long_steps, checked=edit_cases.LONG_CHECKED)


def test_degenerate_edits_and_the_movable_flag_on_the_device(solr):
    """no frames, rows only: a cylinder of zero length, a triangle with two equal vertices and a zero normal with the
    normals flag leave what the host's setters leave; and the unmovable sphere of the mix, edited, follows the translation
    behind the edit - k_setPrimitives sets its movable flag as setPrimitive does"""
    hip = solr.hip_lib()
    k = _kernel(solr, "mix", "hip")
    try:
        start = k.flat_scene()
        p = start.primitives
        rod = edit_cases.record(p[np.flatnonzero(p["type"] == solr.ptCylinder)[0]], seed=1)
        rod["p1"] = rod["p0"]
        triangles = np.flatnonzero(p["type"] == solr.ptTriangle)
        tri = edit_cases.record(p[triangles[0]], seed=2)
        tri["p1"] = tri["p0"]
        flat_normal = edit_cases.record(p[triangles[1]], seed=3, flags=solr.EDIT_NORMALS)
        flat_normal["n1"] = 0.0
        fixed = int(np.flatnonzero((p["type"] == solr.ptSphere) & (p["size"][:, 0] == 1300.0))[0])
        batches = [edit_cases.records([rod, tri, flat_normal]),
                   edit_cases.records([edit_cases.record(p[fixed], seed=4, flags=solr.EDIT_TEXTURE_COORDINATES)])]
        gpu_frame(k)
        uploaded = k.device_primitives().copy()
        edits = hip.solr_hip_device_edits()
        for n, batch in enumerate(batches):
            assert k.set_primitives(batch) == 0
            assert k.pending_moves() == n + 1
        k.translate_primitives(TRANSLATIONS[0])
        assert k.pending_moves() == 3 and hip.solr_hip_device_edits() == edits + 2
        prims, nodes = k.device_primitives(), k.device_nodes(exact=True)
        k.check(0, "degenerate edits")
        caught_up = k.flat_scene()
    finally:
        k.finalize()
    h = _kernel(solr, "mix", "host-only")
    try:
        for batch in batches:
            assert h.set_primitives(batch) == 0
        h.translate_primitives(TRANSLATIONS[0])
        flat = h.flat_scene()
    finally:
        h.finalize()
    assert np.array_equal(flat.primitives["p0"][fixed], (batches[1]["p0"][0] + np.asarray(TRANSLATIONS[0], f32)).astype(f32))
    assert _same_bits(prims, _primitive_rows(flat, uploaded))
    assert _same_bits(nodes, _node_rows(flat))
    assert _same_records(caught_up.primitives, flat.primitives) and _same_records(caught_up.boxes, flat.boxes)


@pytest.mark.parametrize("case", ["emissive", "material", "nan", "slots", "touched", "other_frame"])
def test_requests_the_engine_cannot_serve_change_nothing(solr, oracle, case):
    """a primitive of an emissive material (its light record would have to follow), another material id (tags and colour
    keys are a join with the materials made at upload), a NaN coordinate, slots out of range or twice, a touched store, a
    frame that is not the resident one: the device's primitives, nodes and lights are what they were, the counter too, and
    the host route serves the request with the host-only engine's result"""
    hip = solr.hip_lib()

    def prepare(kernel):
        """what keeps the batch off the device in the cases where the batch itself is fine"""
        if case == "touched":
            kernel.L.SolR_SetPrimitiveMaterial(3, kernel.L.SolR_GetPrimitiveMaterial(3))
        elif case == "other_frame":
            kernel.set_frame(0)

    k = _kernel(solr, "mix", "hip")
    mine = None
    try:
        start = k.flat_scene()
        p = start.primitives
        view_distance = k.info["viewDistance"]
        batch = edit_cases.batches(start, "mix")[1].copy()
        gpu_frame(k)
        prims, nodes, lights = k.device_primitives().copy(), k.device_nodes(exact=True).copy(), k.device_lights().copy()
        counters = _counters(hip)

        def unchanged(what):
            assert _same_bits(k.device_primitives(), prims) and _same_bits(k.device_nodes(exact=True), nodes), what
            assert _same_bits(k.device_lights(), lights), what
            assert _counters(hip) == counters, what
            k.check(0, what + ": a refusal is not an error")

        def engine_refuses(records, slots, what):
            records, slots = np.ascontiguousarray(records), np.ascontiguousarray(slots, np.int32)
            assert hip.solr_hip_set_primitives(records.ctypes.data, slots.ctypes.data, len(records), view_distance) == 0, what
            unchanged(what)

        if case == "emissive":
            assert start.nb_lamps == 1
            batch = edit_cases.records(list(batch) + [edit_cases.record(p[0], seed=8)])
            engine_refuses(batch, _slots(start, batch), "a primitive of an emissive material")
        elif case == "material":
            batch["materialId"][2] = next(int(m) for m in p["materialId"][start.nb_lamps:] if m != batch["materialId"][2])
            engine_refuses(batch, _slots(start, batch), "another material id")
        elif case == "nan":
            batch["p1"][1, 1] = np.nan
            engine_refuses(batch, _slots(start, batch), "a NaN coordinate")
            infinite = edit_cases.batches(start, "mix")[1].copy()
            infinite["vt2"][3, 0] = np.inf
            engine_refuses(infinite, _slots(start, infinite), "an infinite texture coordinate without the flag")
        elif case == "slots":
            # (the engine's own boundary: the host side never sends these)
            slots = _slots(start, batch)
            for what, bad in (("a slot twice", np.r_[slots[:-1], slots[0]]), ("a slot out of range", np.r_[slots[:-1], len(p)]),
                              ("slot -1", np.r_[slots[:-1], -1]), ("a record for another slot's primitive", slots[::-1])):
                engine_refuses(batch, bad, what)
            assert hip.solr_hip_set_primitives(None, None, 0, view_distance) == 0
            assert hip.solr_hip_set_primitives(batch.ctypes.data, slots.ctypes.data, 0, view_distance) == 0
            unchanged("no records")
            assert hip.solr_hip_set_primitives(batch.ctypes.data, slots.ctypes.data, len(batch), 2.0e6) == 0
            unchanged("seeds would not commute")
            # the same records with their own slots are served
            assert k.set_primitives(batch) == 0
            assert k.pending_moves() == 1 and _counters(hip) == counters[:3] + (counters[3] + 1,)
            return
        prepare(k)
        # the Kernel-level call takes the host route then
        assert k.set_primitives(batch) == 0
        assert k.pending_moves() == 0, "the batch was served on the device"
        unchanged("the host route")
        mine = k.flat_scene()
        if case != "nan":
            frame = copy_frame(gpu_frame(k))          # uploads what the host route made
            opp, oids, orgb, _, status = oracle_frame(k, oracle)
            assert status == 0
            assert_parity(compare_frames(*frame, opp, oids, orgb))
            assert _counters(hip) == counters
            # ... after which the scene is resident again and the next valid batch is served over there
            valid = edit_cases.batches(mine, "mix")[0]       # (the materials as the store has them now)
            assert k.set_primitives(valid) == 0
            assert k.pending_moves() == 1 and _counters(hip) == counters[:3] + (counters[3] + 1,)
            frame = copy_frame(gpu_frame(k))
            opp, oids, orgb, _, status = oracle_frame(k, oracle)      # catches the host store up
            assert status == 0 and k.pending_moves() == 0
            assert_parity(compare_frames(*frame, opp, oids, orgb))
    finally:
        k.finalize()
    h = _kernel(solr, "mix", "host-only")
    try:
        prepare(h)
        assert h.set_primitives(batch) == 0
        theirs = h.flat_scene()
    finally:
        h.finalize()
    assert _same_records(mine.primitives, theirs.primitives) and _same_records(mine.boxes, theirs.boxes)
    assert _same_records(mine.lights, theirs.lights)


def test_a_morph_behind_a_device_edit(solr, oracle):
    """k_morphPrimitives would leave the texture coordinates and the movable flags as the edit set them: the engine
    declines, the host serves the morph, and the result is the host-only engine's"""
    hip = solr.hip_lib()
    k = _kernel(solr, "mix", "hip")
    try:
        start = k.flat_scene()
        batch = edit_cases.batches(start, "mix")[2]
        gpu_frame(k)
        uploaded = k.device_primitives().copy()
        morphs, edits = hip.solr_hip_device_morphs(), hip.solr_hip_device_edits()
        assert k.set_primitives(batch) == 0
        assert k.pending_moves() == 1 and hip.solr_hip_device_edits() == edits + 1
        gpu_frame(k)
        assert hip.solr_hip_morph_primitives(0.5, k.info["viewDistance"]) == 0      # the engine's own rule
        assert k.morph_frame(0.5) == 0
        assert k.pending_moves() == 0 and not k.pending_morph(), "the morph was served behind an edit"
        assert hip.solr_hip_device_morphs() == morphs
        frame = copy_frame(gpu_frame(k))
        prims = k.device_primitives()
        k.check(0, "a morph behind an edit is not an error")
        mine = k.flat_scene()
    finally:
        k.finalize()
    h = _kernel(solr, "mix", "host-only")
    try:
        assert h.set_primitives(batch) == 0 and h.morph_frame(0.5) == 0
        _oracle_on(h, oracle, frame, mine.randoms)
        flat = h.flat_scene()
    finally:
        h.finalize()
    assert _same_records(mine.primitives, flat.primitives) and _same_records(mine.boxes, flat.boxes)
    assert _same_bits(prims, _primitive_rows(flat, uploaded))


def test_the_water_scene_is_edited_on_the_device(solr):
    """scenes.water / scenes.water_edits, the reference's torus animation restated: 1152 textured triangles set anew per
    frame, served on the device, the rows those of the host-only engine after the same batches"""
    hip = solr.hip_lib()
    timers = (0.25, 0.5)
    k = solr.scenes.water(solr.Kernel(engine="hip", deterministic_seed=1), width=96, height=64)
    try:
        assert len(solr.scenes.water_edits(0.0, **k.water)) == 1152
        gpu_frame(k)
        uploaded = k.device_primitives().copy()
        edits = hip.solr_hip_device_edits()
        for n, timer in enumerate(timers):
            assert k.set_primitives(solr.scenes.water_edits(timer, **k.water)) == 0
            assert k.pending_moves() == n + 1 and hip.solr_hip_device_edits() == edits + n + 1
            gpu_frame(k)
        prims, nodes = k.device_primitives(), k.device_nodes(exact=True)
        k.check(0, "the water scene")
    finally:
        k.finalize()
    h = solr.scenes.water(solr.Kernel(engine="host-only", deterministic_seed=1), width=96, height=64)
    try:
        for timer in timers:
            assert h.set_primitives(solr.scenes.water_edits(timer, **h.water)) == 0
        flat = h.flat_scene()
    finally:
        h.finalize()
    assert _same_bits(prims, _primitive_rows(flat, uploaded))
    assert _same_bits(nodes, _node_rows(flat))
    assert not _same_bits(prims, uploaded)
