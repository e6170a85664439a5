"""The entry points of key-frame tracks: declared in the headers, exported by the libraries, let through by the version script,
taken up by the Python layer."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = ("solr_hip_set_morph_track_key", "solr_hip_morph_between", "solr_hip_morph_track_keys", "solr_hip_device_track_morphs")


def _declared(path):
    text = open(os.path.join(ROOT, path)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"^\s*(?:[A-Za-z_][\w \*]*?)\b(\w+)\s*\([^;{]*\)\s*;", text, flags=re.M))


def test_the_engine_declares_and_exports_the_track(solr):
    header = open(os.path.join(ROOT, "include", "solr_hip.h")).read()
    assert re.search(r"^#define SOLR_MORPH_TRACK_MAX_KEYS 256$", header, flags=re.M)
    assert set(ENGINE) <= _declared("include/solr_hip.h")
    assert "solr_hip_probe_pack_morph_key" in _declared("include/solr_hip_probes_morph.h")
    lib = solr.hip_lib()
    for name in ENGINE + ("solr_hip_probe_pack_morph_key", "solr_hip_set_morph_keys", "solr_hip_morph_primitives",
                          "solr_hip_device_morphs"):
        assert hasattr(lib, name), name


def test_the_version_script_lists_them():
    """csrc/exports.map names what libsolr_hip.so exports, by pattern: every one of the names must match a global pattern
    and the catch-all must stay local"""
    text = open(os.path.join(ROOT, "sol-r_amd", "csrc", "exports.map")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    exported = re.search(r"global:(.*?)local:", text, flags=re.S).group(1)
    patterns = [p.strip() for p in exported.split(";") if p.strip()]
    assert re.search(r"local:\s*\*\s*;", text)
    for name in ENGINE + ("solr_hip_probe_pack_morph_key",):
        assert any(re.fullmatch(p.replace("*", ".*"), name) for p in patterns), name


def test_the_flat_api_and_the_python_layer(solr):
    assert {"SolRx_MorphBetween", "SolRx_GetNbFrames", "SolRx_MorphFrame"} <= _declared("sol-r_amd/host/SolRStub.h")
    lib = solr.host_lib()
    assert hasattr(lib, "SolRx_MorphBetween") and hasattr(lib, "SolRx_GetNbFrames")
    assert callable(solr.Kernel.morph_between) and callable(solr.Kernel.play)
    k = track_cases.build(solr.Kernel(engine="host-only", deterministic_seed=1), "sticks")
    try:
        assert k.L.SolRx_GetNbFrames() == track_cases.NB_KEYS + 1
        before = k.flat_scene().primitives
        assert k.L.SolRx_MorphBetween(0, 1, 0.5) == 0 and k.L.SolRx_MorphBetween(0, track_cases.NB_KEYS, 0.5) == -1
        assert not np.array_equal(before["p0"], k.flat_scene().primitives["p0"])
        assert k.play(1.5) == 0 and k.morph_between(2, 3, 0.5) == 0
    finally:
        k.finalize()
