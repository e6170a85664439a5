"""Materials edited with several in-process devices (occupancyParameters.x > 1): every device holds the table and the scene
and follows an edit in its own copy (solr_hip_edit_materials: each engine is asked before any is changed), and the frame the
devices render in strips is the one-device frame.  A one-GPU box pretends four devices (SOLR_HIP_VIRTUAL_DEVICES, as
tests/test_material_sets_devices_gpu.py does)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import material_edit_cases as cases  # noqa: E402
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


def test_material_edits_on_the_tables_and_scenes_of_every_device(solr):
    hip = solr.hip_lib()
    frames = {}
    for devices in (1, 2):
        k = solr.Kernel(engine="hip")
        X.sticks(k, width=W, height=H)
        try:
            k.set_material_edits(True)
            assert k.set_gpu_count(devices) == devices
            for _ in range(2):          # (until the order-free lists are built and in the arena: no layout is due any more)
                _frame(k)
            got = [_frame(k)]
            served = hip.solr_hip_device_material_edits(), hip.solr_hip_device_material_retags(), k.material_edits()
            for n, steps in enumerate(([("edit", 2, dict(r=0.9, g=0.2, b=0.1))],
                                       [("edit", 0, dict(transparency=0.5, refraction=1.1, opacity=0.1)), ("edit", 4, dict(r=0.1, g=0.9, b=0.9))],
                                       [("edit", 3, dict(reflection=0.6))])):
                for step in steps:
                    cases.apply(k, step)
                uploads = k.scene_uploads()
                got.append(_frame(k))
                assert k.scene_uploads() == uploads
                assert k.material_edits() == served[2] + n + 1, "edit %d was uploaded as a table" % n
            assert hip.solr_hip_device_material_edits() == served[0] + 3
            assert hip.solr_hip_device_material_retags() == served[1] + 2       # (a reflection launches nothing)
            # a sphere's material turned procedural: no device changes anything, the table is uploaded to all of them
            cases.apply(k, ("edit", 1, dict(procedural=True)))
            assert hip.solr_hip_edit_materials(*cases.table_pointer(k)) == 0
            got.append(_frame(k))
            assert k.material_edits() == served[2] + 3 and hip.solr_hip_device_material_edits() == served[0] + 3
            # ... behind which an edit is followed in place again
            cases.apply(k, ("edit", 5, dict(r=0.3, g=0.3, b=0.9)))
            got.append(_frame(k))
            assert k.material_edits() == served[2] + 4
            frames[devices] = got
            k.check(0, "material edits")
        finally:
            k.finalize()
    for i in (1, 2, 4, 5):
        assert not np.array_equal(frames[1][i - 1][0], frames[1][i][0]), "edit %d changed nothing in the picture" % i
    for i in range(6):
        assert np.array_equal(frames[2][i][0], frames[1][i][0]), "after %d edits: image" % i
        assert np.array_equal(frames[2][i][1].view(np.uint32), frames[1][i][1].view(np.uint32)), "after %d edits: float frame buffer" % i
        assert np.array_equal(frames[2][i][2], frames[1][i][2]), "after %d edits: primitive ids" % i
