"""Materials edited under a resident scene, no GPU: the cases of tests/material_edit_cases.py against their own model, the
symbols of the two libraries, and the switch on an engine without a device.

  - what every case expects of the engine - serve, or decline because a primitive would be of another kind - is what
    served_model says from the kind rule alone;
  - the three words an edit leaves in the primitives of the edited materials, next to the words everybody else keeps, are the
    three words of a fresh retag of the whole flattened scene under the new table: SolR_SetMaterial reaches the record it
    names and no other;
  - SolRx_SetMaterialEdits / SolRx_MaterialEdits and the engine's three entry points exist;
  - on the host-only engine the switch changes nothing: the same steps leave the same flattened scene and the same table,
    and no edit is counted.

The engine's kernel is held to the table upload it replaces in tests/test_material_edits_gpu.py."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import material_edit_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = ("solr_hip_edit_materials", "solr_hip_device_material_edits", "solr_hip_device_material_retags")
HOST = ("SolRx_SetMaterialEdits", "SolRx_MaterialEdits")


def _kernel(solr, case, engine="host-only"):
    return cases.build_case(solr.Kernel(engine=engine, deterministic_seed=1), case)


def _same(a, b):
    """field by field: the structs carry padding that no one initialises"""
    return len(a) == len(b) and all(
        np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8))
        for f in a.dtype.names)


def _tables(solr, name, switch=None):
    """the case's frames on a host-only kernel: the flattened scene, and per frame the table before and after its steps"""
    case = cases.CASES[name]
    k = _kernel(solr, case)
    try:
        if switch is not None:
            assert k.set_material_edits(switch) == 0
        flat = k.flat_scene()
        out = []
        for frame in case["frames"](k, flat):
            before = cases.materials_of(k)
            for step in frame:
                cases.apply(k, step)
            k.L.SolRx_Render(0.0)          # one frame of the protocol; without a device it renders nothing
            out.append((before, cases.materials_of(k)))
        return flat, out, k.flat_scene(), k.material_edits()
    finally:
        k.finalize()


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_what_a_case_expects_is_what_the_kind_rule_says(solr, name):
    case = cases.CASES[name]
    flat, tables, _, _ = _tables(solr, name)
    assert len(tables) == len(case["expect"])
    for n, ((before, after), expect) in enumerate(zip(tables, case["expect"])):
        assert expect in ("served", "kind", "table", "contained")
        if expect == "table":
            assert len(after) == len(before) + 1, "frame %d: the table did not grow" % n
            continue
        assert cases.changed_materials(before, after), "frame %d changes no material" % n
        assert cases.served_model(flat, before, after) == (expect != "kind"), "frame %d" % n
        if expect == "contained":
            # (engine.h primitiveContained: a procedural sphere's surface is displaced beyond its leaf's box)
            p = flat.primitives
            (m,) = cases.changed_materials(before, after)
            assert ((p["materialId"] == m) & (p["type"] == cases.solr.ptSphere)).any()
            assert before[m]["attributes"][1] == 0 and after[m]["attributes"][1] == 1
            others = np.unique(p["type"])
            assert set(int(t) for t in others) <= {cases.solr.ptSphere, cases.solr.ptXZPlane}, "everything lay inside its leaf"


def test_the_cases_cover_both_ends_of_the_retag_rule(solr):
    """a served edit that rewrites nothing in the scene (two copies, no kernel) and ones that do"""
    launches = {}
    for name in sorted(cases.SERVED):
        _, tables, _, _ = _tables(solr, name)
        launches[name] = [cases.retags_model(before, after) for before, after in tables]
    assert launches["reflection_only"] == [False, False]
    assert launches["texture_swapped"] == [False, False]       # (the cold record alone: the facts say "textured" either way)
    assert launches["colour_of_the_most_used"] == [True, True] and launches["transparent_and_back"] == [True, True]
    assert launches["a_material_nobody_has"] == [True]           # (its facts change; no lane finds it)
    # both ways k_retagMaterials looks a material up: more records than RETAG_LINEAR (solr_materials.hip), and exactly as many
    _, tables, _, _ = _tables(solr, "ten_materials_then_eight")
    assert [len(cases.changed_materials(before, after)) for before, after in tables] == [10, 8]
    assert all(np.float32(cases.key_model(b[m])).view(np.int32) != np.float32(cases.key_model(a[m])).view(np.int32)
               for b, a in tables for m in cases.changed_materials(b, a)), "a record that would not be in the batch"


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_an_edits_three_words_are_those_of_a_fresh_retag(solr, name):
    flat, tables, _, _ = _tables(solr, name)
    for n, (before, after) in enumerate(tables):
        if len(before) != len(after):
            before = np.concatenate([before, after[len(before):]])      # (the material that was added, as it was added)
        mine = cases.edited_words_model(flat, before, after)
        fresh = cases.three_words_model(flat, after)
        assert np.array_equal(mine, fresh), "frame %d: slots %s" % (n, np.flatnonzero((mine != fresh).any(axis=1))[:8])
        assert np.array_equal(mine[:, 1], flat.primitives["materialId"])


def test_the_new_symbols_exist(solr):
    hip, host = solr.hip_lib(), solr.host_lib()
    for name in ENGINE:
        assert getattr(hip, name) is not None
    for name in HOST:
        assert getattr(host, name) is not None
    header = open(os.path.join(ROOT, "include", "solr_hip.h")).read()
    stub = open(os.path.join(ROOT, "sol-r_amd", "host", "SolRStub.h")).read()
    for name in ENGINE:
        assert re.search(r"\bint %s\(" % name, header), name + " is not declared in include/solr_hip.h"
    for name in HOST:
        assert re.search(r"\bint %s\(" % name, stub), name + " is not declared in SolRStub.h"


def test_the_engine_declines_without_an_initialised_engine(solr):
    """no device is touched: the first condition of the decline list"""
    hip = solr.hip_lib()
    table = np.zeros(3, solr.MATERIAL_DTYPE)
    counters = hip.solr_hip_device_material_edits(), hip.solr_hip_device_material_retags()
    assert hip.solr_hip_edit_materials(table.ctypes.data, 3) == 0
    assert hip.solr_hip_edit_materials(None, 0) == 0
    assert (hip.solr_hip_device_material_edits(), hip.solr_hip_device_material_retags()) == counters


@pytest.mark.parametrize("name", ["transparent_and_back", "table_grown", "texture_swapped"])
def test_the_switch_changes_nothing_on_the_host_only_engine(solr, name):
    _, off, flat_off, edits_off = _tables(solr, name)
    _, on, flat_on, edits_on = _tables(solr, name, switch=True)
    assert edits_off == 0 and edits_on == 0, "an engine without a device followed an edit"
    for (b0, a0), (b1, a1) in zip(off, on):
        assert _same(b0, b1) and _same(a0, a1)
    for part in ("primitives", "boxes", "lights", "materials"):
        assert _same(getattr(flat_off, part), getattr(flat_on, part)), part


def test_set_material_is_solr_set_material(solr):
    """Kernel.set_material with a material's own keywords leaves its record as it was; with a change, that change"""
    case = cases.CASES["reflection_only"]
    k = _kernel(solr, case)
    try:
        before = cases.materials_of(k)
        for m in range(len(before)):
            k.set_material(m, **cases.keywords_of(before[m]))
        assert _same(before, cases.materials_of(k))
        cases.apply(k, ("edit", 3, dict(r=0.25, wireframe=True, wireframeWidth=3)))
        after = cases.materials_of(k)
        assert cases.changed_materials(before, after) == [3]
        assert after[3]["color"][0] == np.float32(0.25) and list(after[3]["attributes"][2:]) == [2, 3]
    finally:
        k.finalize()


def test_material_pulse_alternates_the_two_kinds_of_edit(solr):
    """scenes.material_pulse: every frame another colour key, every other frame other facts"""
    case = cases.CASES["transparent_and_back"]
    k = _kernel(solr, case)
    try:
        tables = [cases.materials_of(k)]
        for step in range(4):
            solr.scenes.material_pulse(k, 2, float(step), specValue=0.6, specPower=80.0)
            tables.append(cases.materials_of(k))
        for step, (before, after) in enumerate(zip(tables[1:], tables[2:]), 1):
            assert cases.changed_materials(before, after) == [2]
            assert cases.key_model(before[2]) != cases.key_model(after[2])
            assert cases.facts_model(before[2]) != cases.facts_model(after[2])
            assert (after[2]["transparency"] != 0) == (step % 2 == 1)
    finally:
        k.finalize()
