"""Translations and lamp moves with several in-process devices (occupancyParameters.x > 1): every device holds the scene and
moves its own copy (solr_hip_translate_primitives, solr_hip_move_lamp: each engine is asked before any is changed), and the
frame the devices render in strips is the one-device frame.  A one-GPU box pretends four devices
(SOLR_HIP_VIRTUAL_DEVICES, as tests/test_in_process_devices_gpu.py does)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scenes_extra as X  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 200, 148          # 148 rows: not a multiple of the 8-pixel tiles within a strip


@pytest.fixture(scope="module", autouse=True)
def four_virtual_devices():
    """SOLR_HIP_VIRTUAL_DEVICES for THIS module's tests only (the library reads it at every initialize_scene)"""
    before = os.environ.get("SOLR_HIP_VIRTUAL_DEVICES")
    os.environ["SOLR_HIP_VIRTUAL_DEVICES"] = "4"
    yield
    if before is None:
        os.environ.pop("SOLR_HIP_VIRTUAL_DEVICES", None)
    else:
        os.environ["SOLR_HIP_VIRTUAL_DEVICES"] = before


def _frame(k):
    image = k.render()
    return image.copy(), k.postprocessing_buffer(), k.primitive_ids().copy()


def test_moves_on_the_resident_scenes_of_every_device(solr):
    hip = solr.hip_lib()
    frames = {}
    for devices in (1, 2):
        k = solr.Kernel(engine="hip")
        X.sticks(k, width=W, height=H)
        try:
            lamp = k.L.SolR_GetLight(0)
            assert lamp >= 0
            there = tuple(c + d for c, d in zip(k.get_primitive_center(lamp), (-2500.0, 1500.0, 3000.0)))
            assert k.set_gpu_count(devices) == devices
            got = [_frame(k)]
            for n, move in enumerate((lambda: k.translate_primitives((300.0, 0.0, -250.5)), lambda: k.set_primitive_center(lamp, there),
                                      lambda: k.rotate_primitives(center=(0.0, 0.0, 0.0), angles=(0.05, 0.11, -0.07)),
                                      lambda: k.translate_primitives((-450.0, 120.0, 80.25)))):
                move()
                assert k.pending_moves() == n + 1, "move %d ran on the host route" % n
                got.append(_frame(k))
            assert (hip.solr_hip_device_rotations(), hip.solr_hip_device_translations(), hip.solr_hip_device_lamp_moves()) == (1, 2, 1)
            frames[devices] = got
            k.check(0, "moves")
        finally:
            k.finalize()
    for i in range(1, 5):
        assert not np.array_equal(frames[1][i - 1][0], frames[1][i][0]), "move %d changed nothing in the picture" % i
    for i in range(5):
        assert np.array_equal(frames[2][i][0], frames[1][i][0]), "after %d moves: image" % i
        assert np.array_equal(frames[2][i][1].view(np.uint32), frames[1][i][1].view(np.uint32)), "after %d moves: float frame buffer" % i
        assert np.array_equal(frames[2][i][2], frames[1][i][2]), "after %d moves: primitive ids" % i
