"""The device builders of the node lists (sol-r_amd/csrc/solr_lists.hip) against the host's (list_builders.cpp) on the
synthetic node lists of tests/list_builder_cases.py: lists chosen so that a leaf falls where a branch of the device builder
is taken - a node's edge on a wave's or a workgroup's, zeros of both signs, centres that coincide, costs that tie, centres
on a bin's edge, extents too small for the bin scale, a dominant leaf, a sampling stride other than 1 - which the scenes
of tests/test_lists_gpu.py, all from the reference's box grid, never steer.  Both input routes of the device builder (host
rows; rows that are on the device already, as the arena's are) must give the host's lists word for word, and the device's
lists must pass, on their own, what tests/free_lists_check.py asks of any eight order-free lists, so that a failure says
what is wrong with them.  No case is skipped or tolerated: the device may decline only the lists named below."""
import numpy as np
import pytest

import engine_probes as E
import free_lists_check
import list_builder_cases as K

pytestmark = pytest.mark.gpu
i32 = np.int32

# the only lists the device builder may leave to the host: fewer than two leaves
MAY_DECLINE = ("minimum-L0",)
# ... and the device's prune decider: nested deeper than the 256 levels it launches
PRUNE_MAY_DECLINE = ("chain-300-deep-threshold-1", "chain-300-deep-threshold-0.25", "chain-300-deep-threshold-4")


@pytest.fixture(scope="module")
def hip(solr):
    lib = solr.hip_lib()
    E.declare(lib)
    lib.solr_hip_clear_error()
    return lib


def _same(what, got, want):
    assert got["count"] == want["count"], "%s: %d nodes a list, the host %d" % (what, got["count"], want["count"])
    assert got["pruned"] == want["pruned"], "%s: %d inner nodes left out, the host %d" % (what, got["pruned"], want["pruned"])
    for o in range(8):
        a, b = got["rows"][o].view(i32), want["rows"][o].view(i32)
        if not np.array_equal(a, b):
            bad = int(np.flatnonzero((a != b).any(axis=(1, 2)))[0])
            raise AssertionError("%s, list %d: node %d is %s (%s), the host's %s (%s)" % (
                what, o, bad, got["rows"][o][bad].tolist(), a[bad].tolist(), want["rows"][o][bad].tolist(), b[bad].tolist()))
        for key in ("start", "origin"):
            if not np.array_equal(got[key][o], want[key][o]):
                bad = int(np.flatnonzero(got[key][o] != want[key][o])[0])
                raise AssertionError("%s, list %d: %s of node %d is %d, the host's %d" % (
                    what, o, key, bad, got[key][o][bad], want[key][o][bad]))


@pytest.mark.parametrize("name", K.FREE_CASES)
def test_device_lists_are_the_hosts_word_for_word(hip, name):
    rows, start, prims, margin, share, threshold = K.free_case(name)
    host = E.free_lists(hip, E.HOST_BUILDER, rows, start, prims, margin, share, threshold)
    for route, what in ((E.DEVICE_FROM_HOST_ROWS, "from host rows"), (E.DEVICE_FROM_DEVICE_ROWS, "from rows on the device")):
        device = E.free_lists(hip, route, rows, start, prims, margin, share, threshold)
        if name in MAY_DECLINE:
            assert device is None and host is None, "%s (%s): a list of fewer than two leaves was built" % (name, what)
            continue
        assert host is not None, name
        assert device is not None, "%s (%s): the device builder declined" % (name, what)
        if route == E.DEVICE_FROM_HOST_ROWS:
            free_lists_check.check(rows, start, device, name + " (device)")
        _same("%s (%s)" % (name, what), device, host)


@pytest.mark.parametrize("name", K.PRUNE_CASES)
def test_device_prune_decisions_are_the_hosts(hip, name):
    rows, start, threshold = K.prune_case(name)
    host = E.prune_list(hip, E.HOST_BUILDER, rows, start, threshold)
    device = E.prune_list(hip, E.DEVICE_FROM_HOST_ROWS, rows, start, threshold)
    # (pruneInnerNodes asks no decider about a list of one node)
    assert device["declined"] == (1 if name in PRUNE_MAY_DECLINE else 0), "%s: declined %d" % (name, device["declined"])
    assert device["count"] == host["count"] and device["pruned"] == host["pruned"], \
        "%s: %d nodes (%d left out), the host %d (%d)" % (name, device["count"], device["pruned"], host["count"], host["pruned"])
    if not np.array_equal(device["origin"], host["origin"]):
        bad = int(np.flatnonzero(device["origin"] != host["origin"])[0])
        raise AssertionError("%s: node %d is input node %d, the host's %d" % (name, bad, device["origin"][bad], host["origin"][bad]))
    assert np.array_equal(device["rows"].view(i32), host["rows"].view(i32)) and np.array_equal(device["start"], host["start"]), name
