"""Materials set with several in-process devices (occupancyParameters.x > 1): every device holds the scene and sets the
batch's materials in its own copy (solr_hip_set_primitive_materials: each engine is asked before any is changed), and the
frame the devices render in strips is the one-device frame.  A one-GPU box pretends four devices
(SOLR_HIP_VIRTUAL_DEVICES, as tests/test_moves_devices_gpu.py does)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scenes_extra as X  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 64, 52            # 52 rows: not a multiple of the 8-pixel tiles within a strip


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


def test_material_sets_on_the_resident_scenes_of_every_device(solr):
    hip = solr.hip_lib()
    frames = {}
    for devices in (1, 2):
        k = solr.Kernel(engine="hip")
        X.sticks(k, width=W, height=H)
        try:
            clear = k.add_material(0.8, 0.9, 1.0, refraction=1.1, transparency=0.5, opacity=0.1, specValue=1.0, specPower=120.0)
            lamp = k.L.SolR_GetLight(0)
            light = k.get_primitive_material(lamp)
            p = k.flat_scene().primitives
            spheres = [int(i) for i in p["index"][p["type"] == solr.ptSphere] if int(i) != lamp]
            rods = [int(i) for i in p["index"][p["type"] == solr.ptCylinder]]
            assert k.set_gpu_count(devices) == devices
            got = [_frame(k)]
            served = hip.solr_hip_device_material_sets()
            for n, (indices, materials) in enumerate(((spheres[:7], [clear] * 7), (rods, [light] * len(rods)),
                                                      (spheres[3:5] + rods[:1], [0, 1, 2]))):
                assert k.set_primitive_materials(indices, materials) == 0
                assert k.pending_moves() == n + 1, "batch %d ran on the host route" % n
                got.append(_frame(k))
            assert hip.solr_hip_device_material_sets() == served + 3
            # a lamp among the records: no device changes anything, the host route serves the batch
            assert k.set_primitive_materials([spheres[0], lamp], [1, light]) == 0
            assert k.pending_moves() == 0 and hip.solr_hip_device_material_sets() == served + 3
            got.append(_frame(k))
            frames[devices] = got
            k.check(0, "material sets")
        finally:
            k.finalize()
    for i in range(1, 5):
        assert not np.array_equal(frames[1][i - 1][0], frames[1][i][0]), "batch %d changed nothing in the picture" % i
    for i in range(5):
        assert np.array_equal(frames[2][i][0], frames[1][i][0]), "after %d batches: image" % i
        assert np.array_equal(frames[2][i][1].view(np.uint32), frames[1][i][1].view(np.uint32)), "after %d batches: float frame buffer" % i
        assert np.array_equal(frames[2][i][2], frames[1][i][2]), "after %d batches: primitive ids" % i
