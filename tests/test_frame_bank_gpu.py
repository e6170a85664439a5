"""The frame bank on the engine: resident scenes set aside and put back (solr_hip_park_scene, solr_hip_resume_scene ...:
sol-r_amd/csrc/solr_bank.hip), and GPUKernel's frame switch on top of it (Kernel.set_frame_bank, scenes.animation).

Engine level, straight through the C ABI, with three scenes that share one material table: A, a Cornell box with spheres and
one lamp; B, a larger triangle mesh with two lamps; C, a lamp, one textured plane and some sticks (another kernel row, no order-free
lists).  The bar is BIT FOR BIT throughout: what the device holds of a scene after a round trip through the bank - primitive
records, light records, every copy of every list, a rendered frame's float buffer, ids and image - is what it held before,
and the bank's own figures are derived in the test (no byte count is written down).  Through Kernel, the frames of
scenes.animation are held to a kernel without the bank and to the oracle (helpers.assert_parity)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_probes as E  # noqa: E402
import material_set_cases  # noqa: E402
import morph_cases  # noqa: E402
import move_cases  # noqa: E402
from helpers import assert_parity, compare_frames, copy_frame, gpu_frame, oracle_frame, same_frames  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 101, 67
K = 4
BANK = 1 << 30
f4, i4 = np.float32, np.int32
LISTS = (E.WALK_LIST, E.EXACT_LIST, E.FREE_LISTS)
COPIES = (E.NODE_ROWS, E.THIN_COPY, E.SORTED_COPY, E.LEAF_RECORDS, E.START_INDICES)
_SCENES = {}


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Flat:
    def __init__(self, k):
        flat = k.flat_scene()
        self.boxes, self.prims, self.lights, self.nb_lamps = flat.boxes, flat.primitives, flat.lights, flat.nb_lamps
        self.lamps = np.ascontiguousarray(flat.lights["primitiveId"][:max(flat.nb_lamps, 1)], i4)
        ptr, n = C.c_void_p(), C.c_int()
        k.L.SolRx_GetMovable(C.byref(ptr), C.byref(n))
        self.movable = np.frombuffer((C.c_char * n.value).from_address(ptr.value), np.uint8).copy()
        self.objects = None


def scenes(solr):
    """A, B and C flattened by the host builder (one host-only kernel, three frames: they share the materials), once"""
    if _SCENES:
        return _SCENES
    S = solr.scenes
    k = solr.Kernel(engine="host-only", deterministic_seed=1)
    try:
        k.initialize(width=W, height=H, nbRayIterations=3, graphicsLevel=solr.glFull)
        rng = S.LCG(11)
        k.set_texture(0, np.fromfunction(lambda y, x, c: ((x // 4 + y // 4) % 2) * 140 + 50 + 20 * c, (32, 32, 3)).astype(np.uint8))
        shiny = [k.add_material(*S._wall_color(rng), reflection=0.4, specValue=1.0, specPower=200.0) for _ in range(3)]
        glass = k.add_material(0.9, 0.95, 1.0, reflection=1.0, refraction=1.1, transparency=0.7, specValue=1.0, specPower=200.0)
        mesh = [k.add_material(*S._wall_color(rng), specValue=0.6, specPower=80.0) for _ in range(3)]
        textured = k.add_material(*S._wall_color(rng), specValue=0.3, specPower=50.0, diffuseTextureId=0)
        k.set_nb_frames(3)
        flats = {}
        # (the smallest first: the builder keeps the depth of the build before, GPUKernel.h m_depthBeforeBuild)
        k.set_frame(2)                                  # C
        k.add_primitive(solr.ptXYPlane, (0.0, 0.0, 4000.0), size=(9000.0, 6000.0, 0.0), material=textured)
        # (the builder wants a dozen primitives for a tree with a lamps' cell; a cone is not held by its leaf's box, so the
        # engine walks no order-free lists of this scene)
        for n in range(9):
            k.add_primitive(solr.ptCylinder, (-8000.0 + 2000.0 * n, -3000.0, 1000.0), (-8000.0 + 2000.0 * n, 500.0 + 150.0 * n, 1000.0),
                            size=(300.0, 0, 0), material=mesh[n % 3])
        k.add_primitive(solr.ptCone, (0.0, 3000.0, 0.0), (0.0, 5500.0, 0.0), size=(900.0, 0, 0), material=mesh[0])
        S.add_light(k, position=(2000.0, 5000.0, -9000.0))
        k.compact_boxes(True)
        flats["C"] = Flat(k)
        k.set_frame(0)                                  # A
        for n, (x, y) in enumerate(((2200.0, 0.0), (-2200.0, 0.0), (0.0, 2600.0))):
            k.add_primitive(solr.ptSphere, (x, y, 0.0), size=(1800.0, 0, 0), material=shiny[n])
        for n in range(7):
            a = 2.0 * np.pi * n / 7
            k.add_primitive(solr.ptSphere, (8000.0 * np.cos(a), -4400.0, 8000.0 * np.sin(a)), size=(600.0, 0, 0), material=mesh[n % 3])
        k.add_primitive(solr.ptSphere, (-4000.0, 3500.0, -6000.0), size=(1200.0, 0, 0), material=glass)
        S.add_room(k, rng)
        S.add_light(k)
        k.compact_boxes(True)
        flats["A"] = Flat(k)
        k.set_frame(1)                                  # B
        n = 13

        def point(i, j):
            u, v = (i / n) * 2.0 - 1.0, (j / n) * 2.0 - 1.0
            return (u * 9000.0, 1300.0 * np.sin(4.0 * u) * np.cos(3.0 * v) - 2500.0, v * 9000.0)

        for i in range(n):
            for j in range(n):
                a, b, c, d = point(i, j), point(i + 1, j), point(i + 1, j + 1), point(i, j + 1)
                k.add_primitive(solr.ptTriangle, a, b, c, material=mesh[(i + j) % 3])
                k.add_primitive(solr.ptTriangle, a, c, d, material=mesh[(i + j) % 3])
        S.add_light(k)
        S.add_light(k, position=(-7000.0, 9000.0, -6000.0))
        k.compact_boxes(True)
        flats["B"] = Flat(k)
        k.set_camera((0.0, 1500.0, -15000.0))
        final = k.flat_scene()
        si, ppi, eye, direction, angles = k.frame_parameters()
        si.pathTracingIteration = 0
        for flat in flats.values():
            flat.objects = solr.Vec4i(len(flat.boxes), len(flat.prims), flat.nb_lamps, flat.nb_lamps)
        assert flats["B"].nb_lamps == 2 and flats["A"].nb_lamps == flats["C"].nb_lamps == 1
        assert len(flats["B"].prims) > 10 * len(flats["A"].prims)
        _SCENES.update(flats=flats, materials=final.materials, textures=final.textures, randoms=final.randoms,
                       frame=(si, ppi, eye, direction, angles), glass=glass, a_material=shiny[0])
    finally:
        k.finalize()
    return _SCENES


class Boundary:
    """the engine driven through the C ABI alone; `with Boundary(solr) as b:` finalizes it afterwards"""

    def __init__(self, solr, materials=None, bank=BANK, flights=1):
        self.solr, self.hip, self.s = solr, solr.hip_lib(), scenes(solr)
        hip = self.hip
        E.declare(hip)
        hip.solr_hip_clear_error()
        hip.solr_hip_set_variant(0)
        hip.solr_hip_set_frames_in_flight(flights)
        hip.solr_hip_set_scene_bank_bytes(bank)
        self.si = self.s["frame"][0]
        hip.solr_hip_initialize(C.byref(self.si))
        self.keep = []
        self.materials(self.s["materials"] if materials is None else materials)
        tex = np.ascontiguousarray(self.s["textures"])
        info = E.TextureInfo(tex.ctypes.data, 0, (C.c_int * 3)(len(tex), 1, 1), 0, 0)
        self.keep += [tex, info]
        hip.h2d_textures(0, 1, C.addressof(info))
        rnd = np.ascontiguousarray(self.s["randoms"], f4)
        self.keep.append(rnd)
        hip.solr_hip_h2d_randoms_sized(E._p(rnd), len(rnd))
        self.check("set-up")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.hip.finalize_scene(0)
        self.hip.solr_hip_set_scene_bank_bytes(0)       # (the knobs outlive finalize_scene)
        self.hip.solr_hip_set_frames_in_flight(1)
        self.hip.solr_hip_clear_error()
        return False

    def check(self, what):
        E._check(self.hip, 0, what)

    def materials(self, table):
        table = np.ascontiguousarray(table)
        self.keep.append(table)
        self.hip.h2d_materials(0, E._p(table), len(table))
        self.check("h2d_materials")

    def upload(self, name):
        flat, hip = self.s["flats"][name], self.hip
        hip.h2d_scene(0, E._p(flat.boxes), len(flat.boxes), E._p(flat.prims), len(flat.prims), E._p(flat.lamps), flat.nb_lamps)
        hip.h2d_lightInformation(0, E._p(flat.lights), flat.nb_lamps)
        hip.solr_hip_set_movable(E._p(flat.movable), len(flat.movable))
        self.check("upload of " + name)

    def launch(self, name):
        _, ppi, eye, direction, angles = self.s["frame"]
        self.hip.solr_hip_render(C.byref(self.si), C.byref(self.s["flats"][name].objects), C.byref(ppi), _fp(eye), _fp(direction),
                                 _fp(angles))

    def render(self, name):
        """one frame of the resident scene `name`: (float buffer, ids, image)"""
        self.launch(name)
        pp, ids, rgb = np.zeros((H, W, 8), f4), np.zeros((H, W, 4), i4), np.zeros((H, W, 3), np.uint8)
        self.hip.solr_hip_d2h_postprocessing(C.c_void_p(pp.ctypes.data))
        self.hip.solr_hip_d2h(C.byref(self.si), C.c_void_p(rgb.ctypes.data), C.c_void_p(ids.ctypes.data))
        self.check("a frame of " + name)
        assert len(np.unique(rgb.reshape(-1, 3), axis=0)) > 1, "the frame of %s is one colour" % name
        return pp, ids, rgb

    def settle(self, name, frames=3):
        for _ in range(frames - 1):
            self.render(name)
        return self.render(name)

    def lights(self):
        n = self.hip.solr_hip_read_lights(None, 0)
        out = np.zeros((max(n, 1), 4), f4)
        assert n >= 0 and self.hip.solr_hip_read_lights(out.ctypes.data, n) == n
        return out[:n]

    def snapshot(self, name, frame=True):
        """what the device holds of the resident scene: primitive and light records, every copy of every list, a frame"""
        state = {"primitives": E.primitive_records(self.hip).tobytes(), "lights": self.lights().tobytes(),
                 "order-free nodes": self.hip.solr_hip_order_free_nodes()}
        for which in LISTS:
            for what in COPIES:
                copy = E.list_copy(self.hip, which, what)
                state["list %d, copy %d" % (which, what)] = None if copy is None else copy.tobytes()
        if frame:
            pp, ids, rgb = self.render(name)
            state.update({"frame: float buffer": pp.tobytes(), "frame: ids": ids.tobytes(), "frame: image": rgb.tobytes()})
        return state

    def counters(self):
        hip = self.hip
        return (hip.solr_hip_device_rotations(), hip.solr_hip_device_translations(), hip.solr_hip_device_lamp_moves(),
                hip.solr_hip_device_edits(), hip.solr_hip_device_material_sets(), hip.solr_hip_device_morphs(),
                hip.solr_hip_device_track_morphs())

    def rotate(self, angles=(0.02, 0.1, -0.03)):
        centre, angles = np.array([100.0, -50.0, 25.0], f4), np.array(angles)
        cos, sin = np.cos(angles).astype(f4), np.sin(angles).astype(f4)
        return self.hip.solr_hip_rotate_primitives(_fp(centre), _fp(cos), _fp(sin), self.si.viewDistance)

    def translate(self, t=(300.0, 0.0, -250.5)):
        return self.hip.solr_hip_translate_primitives(_fp(np.array(t, f4)), self.si.viewDistance)


def _assert_same(mine, theirs, label):
    assert mine.keys() == theirs.keys()
    for key in mine:
        assert mine[key] == theirs[key], "%s: %s differs" % (label, key)


@pytest.mark.parametrize("order", ["A then B", "B then A"])
def test_park_and_resume_keeps_everything(solr, order):
    """the parked scene against the larger / the smaller arena uploaded after it, in either order; C (another kernel row,
    no lists of the engine's own) in between"""
    first, second = ("A", "B") if order == "A then B" else ("B", "A")
    with Boundary(solr) as b:
        hip = b.hip
        b.upload(first)
        b.settle(first)
        assert hip.solr_hip_order_free_nodes() > 0, "%s has no order-free lists" % first
        before = b.snapshot(first)
        memory = (C.c_ulonglong * 4)()
        hip.solr_hip_memory_usage(memory)
        uploads, switches = hip.solr_hip_scene_uploads(), hip.solr_hip_scene_switches()
        assert uploads == 1 and switches == 0
        assert hip.solr_hip_park_scene(0) == 1
        assert hip.solr_hip_parked_scenes() == 1 and hip.solr_hip_parked_bytes() >= memory[0] > 0
        after = (C.c_ulonglong * 4)()
        hip.solr_hip_memory_usage(after)
        assert after[0] == 0 and list(after[1:]) == list(memory[1:])      # the resident scene only: there is none
        assert hip.solr_hip_read_primitives(None, 0) == -1                # as after initialize_scene
        hip.solr_hip_clear_error()
        b.upload(second)
        other = b.settle(second)
        assert hip.solr_hip_order_free_nodes() > 0
        b.upload("C")
        b.settle("C")
        assert hip.solr_hip_order_free_nodes() == 0
        uploads = hip.solr_hip_scene_uploads()
        assert uploads == 3
        assert hip.solr_hip_resume_scene(0) == 1
        assert hip.solr_hip_scene_uploads() == uploads and hip.solr_hip_scene_switches() == switches + 1
        assert hip.solr_hip_parked_scenes() == 0 and hip.solr_hip_parked_bytes() == 0
        _assert_same(b.snapshot(first), before, "%s after the round trip" % first)
        hip.solr_hip_memory_usage(after)
        assert list(after) == list(memory)
        assert not same_frames(other, b.render(first))
        assert hip.solr_hip_resume_scene(0) == 0                          # it is not in the bank any more
        b.check("a resume of a key that is not there is not an error")


def test_device_moves_survive_a_round_trip(solr):
    with Boundary(solr) as b:
        hip = b.hip
        b.upload("A")
        b.settle("A")
        assert b.rotate() == 1 and b.translate() == 1 and b.rotate() == 1, "a move was declined"
        straight = b.snapshot("A", frame=False)
        assert b.rotate() == 1
        three = b.snapshot("A")
        counts = b.counters()
        assert counts[:2] == (3, 1)
    with Boundary(solr) as b:
        hip = b.hip
        b.upload("A")
        b.settle("A")
        assert b.counters() == (0,) * 7
        assert b.rotate() == 1 and b.translate() == 1 and b.rotate() == 1
        moved = b.counters()
        assert moved[:2] == (2, 1)
        assert hip.solr_hip_park_scene(5) == 1
        assert b.counters() == moved, "the counters jumped at the park"
        b.upload("B")
        b.settle("B")
        assert b.rotate((0.0, 0.3, 0.0)) == 1                             # B moves on the device too
        assert b.counters()[0] == moved[0] + 1
        assert hip.solr_hip_park_scene(6) == 1
        assert hip.solr_hip_resume_scene(5) == 1
        assert b.counters()[0] == moved[0] + 1, "the counters jumped at the resume"
        _assert_same(b.snapshot("A", frame=False), straight, "A after its round trip")
        assert b.rotate() == 1
        _assert_same(b.snapshot("A"), three, "one more rotation after the round trip, against the three moves with no detour")
        assert b.counters() == (counts[0] + 1,) + counts[1:]
        assert hip.solr_hip_scene_switches() == 1 and hip.solr_hip_scene_uploads() == 2 and hip.solr_hip_parked_scenes() == 1


def test_the_counters_are_the_engines_not_a_scenes(solr):
    """the two lifetimes the round trip above does not reach: an h2d_scene over a moved scene, and a resume over a resident
    scene (which is dropped for it) - neither moves a counter, and the request after them adds exactly one"""
    with Boundary(solr) as b:
        hip = b.hip
        b.upload("A")
        b.settle("A")
        assert b.counters() == (0,) * 7
        assert b.rotate() == 1 and b.translate() == 1, "a move was declined"
        moved = b.counters()
        assert moved == (1, 1, 0, 0, 0, 0, 0)
        b.upload("B")                                   # over the moved A, which goes
        assert b.counters() == moved, "the counters jumped at h2d_scene"
        b.settle("B")
        assert b.counters() == moved
        assert hip.solr_hip_park_scene(3) == 1
        b.upload("A")
        b.settle("A")
        assert b.rotate() == 1
        rotated = b.counters()
        assert rotated == (2,) + moved[1:]
        assert hip.solr_hip_resume_scene(3) == 1        # over the resident A: dropped, not parked
        assert hip.solr_hip_parked_scenes() == 0 and hip.solr_hip_scene_switches() == 1
        assert b.counters() == rotated, "the counters jumped at a resume that dropped the resident scene"
        b.render("B")
        assert b.rotate((0.0, 0.3, 0.0)) == 1
        assert b.counters() == (3,) + moved[1:]
        b.render("B")


def test_the_order_free_countdown_is_parked_with_the_scene(solr, monkeypatch):
    monkeypatch.setenv("SOLR_HIP_FREE_AFTER", "3")      # (read at h2d_scene)
    with Boundary(solr) as b:
        hip = b.hip
        b.upload("B")
        b.render("B")
        assert hip.solr_hip_order_free_nodes() == 0
        assert hip.solr_hip_park_scene(1) == 1          # two renders short of its lists
        b.upload("A")
        b.settle("A", 4)                                # A's own countdown runs out meanwhile
        assert hip.solr_hip_order_free_nodes() > 0
        assert hip.solr_hip_park_scene(0) == 1
        assert hip.solr_hip_resume_scene(1) == 1
        assert hip.solr_hip_order_free_nodes() == 0
        b.render("B")
        assert hip.solr_hip_order_free_nodes() == 0, "the lists came a render early"
        b.render("B")
        assert hip.solr_hip_order_free_nodes() > 0, "the lists are not there the stated number of renders after the upload"
        late = b.snapshot("B")
    with Boundary(solr) as b:
        b.upload("B")
        b.settle("B", 3)
        _assert_same(b.snapshot("B"), late, "B with its lists after a detour through the bank, against B left alone")


def test_materials_uploaded_between_park_and_resume(solr):
    s = scenes(solr)
    other = s["materials"].copy()
    m = s["a_material"]
    assert other["transparency"][m] == 0.0
    other["color"][m][:3] = (0.9, 0.2, 0.1)
    other["transparency"][m], other["refraction"][m], other["reflection"][m] = 0.6, 1.2, 0.0
    with Boundary(solr, materials=other) as b:
        b.upload("A")
        b.settle("A")
        fresh = b.snapshot("A")
    with Boundary(solr) as b:
        hip = b.hip
        b.upload("A")
        b.settle("A")
        old = b.snapshot("A")
        assert old["primitives"] != fresh["primitives"] and old["frame: image"] != fresh["frame: image"]
        assert hip.solr_hip_park_scene(0) == 1
        b.upload("C")
        b.render("C")
        b.materials(other)
        b.render("C")
        uploads = hip.solr_hip_scene_uploads()
        assert hip.solr_hip_resume_scene(0) == 1
        assert hip.solr_hip_scene_uploads() == uploads
        b.settle("A")
        _assert_same(b.snapshot("A"), fresh, "A resumed under other materials, against A uploaded fresh under them")
        # ... and under the same table again a plain resume: nothing is retagged
        assert hip.solr_hip_park_scene(0) == 1 and hip.solr_hip_resume_scene(0) == 1
        _assert_same(b.snapshot("A"), fresh, "a second round trip")


def test_the_byte_limit(solr):
    with Boundary(solr) as b:
        hip = b.hip
        b.upload("A")
        b.settle("A")
        assert hip.solr_hip_park_scene(0) == 1
        held = hip.solr_hip_parked_bytes()
        b.upload("B")
        b.settle("B")
        assert hip.solr_hip_park_scene(1) == 1          # what B needs: measured, then B is taken back
        needs = hip.solr_hip_parked_bytes() - held
        assert needs > 0 and hip.solr_hip_resume_scene(1) == 1 and hip.solr_hip_parked_bytes() == held
        before = b.snapshot("B")
        hip.solr_hip_set_scene_bank_bytes(held + needs - 1)
        uploads = hip.solr_hip_scene_uploads()
        assert hip.solr_hip_park_scene(1) == 0
        b.check("a declined park is not an error")
        assert hip.solr_hip_parked_scenes() == 1 and hip.solr_hip_parked_bytes() == held
        _assert_same(b.snapshot("B"), before, "B after its park was declined")      # it stays resident
        hip.solr_hip_set_scene_bank_bytes(held + needs)
        assert hip.solr_hip_park_scene(1) == 1 and hip.solr_hip_resume_scene(1) == 1
        hip.solr_hip_set_scene_bank_bytes(0)            # lowering the limit drops nothing; every park is declined
        assert hip.solr_hip_parked_scenes() == 1 and hip.solr_hip_parked_bytes() == held
        assert hip.solr_hip_park_scene(1) == 0 and hip.solr_hip_park_scene(7) == 0
        b.upload("C")                                   # ... and the next h2d_scene replaces B
        assert hip.solr_hip_scene_uploads() == uploads + 1
        b.settle("C")
        assert hip.solr_hip_read_primitives(None, 0) == 8 * len(b.s["flats"]["C"].prims)
        assert hip.solr_hip_resume_scene(0) == 1        # what was parked can still be had
        b.render("A")
    with Boundary(solr, bank=0) as b:
        b.upload("A")
        b.render("A")
        assert b.hip.solr_hip_park_scene(0) == 0 and b.hip.solr_hip_parked_scenes() == 0
        b.check("limit 0")


@pytest.mark.parametrize("flights", [2, 3])
def test_frames_in_flight_across_parks_and_resumes(solr, flights):
    """park and resume between frames with nothing flushed: the images delivered, in order, are those rendered one at a time"""
    order = ["A", "B", "A", "C", "B", "A", "C", "B"]
    with Boundary(solr) as b:
        alone = {}
        for name in "ABC":
            b.upload(name)
            alone[name] = b.settle(name)[2]
    with Boundary(solr, flights=flights) as b:
        hip = b.hip
        for key, name in enumerate("ABC"):
            b.upload(name)
            b.settle(name)
            assert hip.solr_hip_park_scene(key) == 1
        uploads = hip.solr_hip_scene_uploads()
        tickets, delivered = [], []

        def deliver():
            image = hip.solr_hip_image_wait(tickets.pop(0))
            assert image
            delivered.append(np.frombuffer(C.string_at(image, W * H * 3), np.uint8).reshape(H, W, 3).copy())

        for name in order:
            key = "ABC".index(name)
            assert hip.solr_hip_resume_scene(key) == 1
            b.launch(name)
            ticket = hip.solr_hip_d2h_image_async()
            assert ticket >= 0
            tickets.append(ticket)
            assert hip.solr_hip_park_scene(key) == 1    # ... while its frame is in flight
            if len(tickets) >= flights:
                deliver()
        while tickets:
            deliver()
        b.check("frames in flight")
        assert hip.solr_hip_scene_uploads() == uploads and hip.solr_hip_scene_switches() == len(order)
        for n, name in enumerate(order):
            assert np.array_equal(delivered[n], alone[name]), "frame %d, of %s" % (n, name)


@pytest.mark.parametrize("how", ["drop one", "drop all", "finalize_scene", "solr_hip_set_variant"])
def test_what_drops_the_bank(solr, how):
    with Boundary(solr) as b:
        hip = b.hip
        for key, name in enumerate("AB"):
            b.upload(name)
            b.settle(name)
            assert hip.solr_hip_park_scene(key) == 1
        assert hip.solr_hip_parked_scenes() == 2
        if how == "drop one":
            both = hip.solr_hip_parked_bytes()
            hip.solr_hip_drop_parked_scenes(0)
            assert hip.solr_hip_parked_scenes() == 1 and 0 < hip.solr_hip_parked_bytes() < both
            assert hip.solr_hip_resume_scene(0) == 0
            assert hip.solr_hip_resume_scene(1) == 1
            b.render("B")
        else:
            if how == "drop all":
                hip.solr_hip_drop_parked_scenes(-1)
            elif how == "finalize_scene":
                hip.finalize_scene(0)
            else:
                hip.solr_hip_set_variant(6)
                hip.solr_hip_set_variant(0)
            assert hip.solr_hip_resume_scene(0) == 0 and hip.solr_hip_resume_scene(1) == 0
        if how != "drop one":
            assert hip.solr_hip_parked_scenes() == 0 and hip.solr_hip_parked_bytes() == 0
        b.check("a resume of a dropped key is not an error")


# ---- through Kernel -------------------------------------------------------------------------------------------------------
def _animation(solr, bank):
    k = solr.Kernel(engine="hip", deterministic_seed=1)
    solr.scenes.animation(k, frames=K)
    if bank:
        k.set_frame_bank(bank)
    return k


def _laps(solr, k, laps):
    frames = []
    for i in range(laps * K):
        solr.scenes.animation_step(k, i)
        frames.append(copy_frame(gpu_frame(k)))
    return frames


def test_two_laps_with_the_bank_on(solr, oracle):
    plain = _animation(solr, 0)
    try:
        reference = _laps(solr, plain, 1)
        assert plain.scene_uploads() == K and plain.frame_switches() == 0
    finally:
        plain.finalize()
    hip = solr.hip_lib()
    k = _animation(solr, BANK)
    try:
        frames = _laps(solr, k, 2)
        assert k.scene_uploads() == K and k.frame_switches() == K and k.parked_frames() == K - 1
        assert hip.solr_hip_scene_uploads() == K and hip.solr_hip_scene_switches() == K and hip.solr_hip_parked_scenes() == K - 1
        assert len({f[2].tobytes() for f in frames[:K]}) == K               # four meshes, four pictures
        for f in range(K):
            assert same_frames(frames[K + f], reference[f]), "frame %d of lap 2 against a kernel without the bank" % f
            # (lap 1 saw the frame before its order-free lists were due - conftest: with the first frame - so it is the same too)
            assert same_frames(frames[K + f], frames[f]), "frame %d of lap 2 against lap 1" % f
            solr.scenes.animation_step(k, f)
            opp, oids, orgb, _, status = oracle_frame(k, oracle)
            assert status == 0
            assert_parity(compare_frames(*frames[K + f], opp, oids, orgb))
        k.check(0, "two laps")
    finally:
        k.finalize()


def test_rotating_a_resumed_frame(solr, oracle):
    hip = solr.hip_lib()
    k = _animation(solr, BANK)
    try:
        _laps(solr, k, 1)
        solr.scenes.animation_step(k, 1)
        gpu_frame(k)
        uploads, rotations = k.scene_uploads(), hip.solr_hip_device_rotations()
        k.rotate_primitives((0.0, 0.0, 0.0), (0.0, 0.05, 0.0))
        assert k.pending_moves() == 1 and hip.solr_hip_device_rotations() == rotations + 1, "the rotation took the host route"
        frame = copy_frame(gpu_frame(k))
        assert k.scene_uploads() == uploads
        opp, oids, orgb, _, status = oracle_frame(k, oracle)      # catches the host store up
        assert status == 0 and k.pending_moves() == 0
        assert_parity(compare_frames(*frame, opp, oids, orgb))
        solr.scenes.animation_step(k, 2)                # a further round trip through another frame
        gpu_frame(k)
        solr.scenes.animation_step(k, 1)
        again = copy_frame(gpu_frame(k))
        assert k.scene_uploads() == uploads and hip.solr_hip_device_rotations() == rotations + 1
        assert same_frames(again, frame)
        opp, oids, orgb, _, status = oracle_frame(k, oracle)
        assert status == 0
        assert_parity(compare_frames(*again, opp, oids, orgb))
        k.check(0, "a rotation on a resumed frame")
    finally:
        k.finalize()


def test_a_resume_the_engine_declines_drops_the_bank_on_both_sides(solr, oracle):
    """the engine's bank emptied behind the host's back: the frame that is entered is flattened and uploaded as ever, nothing
    stays parked here or there, and the bank fills again; the engine's limit is the host's, the 0 too"""
    hip = solr.hip_lib()
    k = _animation(solr, BANK)
    try:
        frames = _laps(solr, k, 1)
        assert k.parked_frames() == hip.solr_hip_parked_scenes() == K - 1
        hip.solr_hip_drop_parked_scenes(-1)
        uploads, switches = k.scene_uploads(), k.frame_switches()
        solr.scenes.animation_step(k, 1)
        again = copy_frame(gpu_frame(k))
        assert (k.scene_uploads() - uploads, k.frame_switches() - switches) == (1, 0)
        assert k.parked_frames() == hip.solr_hip_parked_scenes() == 0
        assert same_frames(again, frames[1])
        opp, oids, orgb, _, status = oracle_frame(k, oracle)
        assert status == 0
        assert_parity(compare_frames(*again, opp, oids, orgb))
        solr.scenes.animation_step(k, 2)
        gpu_frame(k)
        solr.scenes.animation_step(k, 1)
        assert same_frames(copy_frame(gpu_frame(k)), frames[1])
        assert (k.scene_uploads() - uploads, k.frame_switches() - switches) == (2, 1)
        k.set_frame_bank(0)
        assert k.parked_frames() == hip.solr_hip_parked_scenes() == 0
        solr.scenes.animation_step(k, 2)
        gpu_frame(k)
        assert hip.solr_hip_park_scene(9) == 0, "the engine's limit is not the host's 0"
        k.check(0, "a declined resume")
    finally:
        k.finalize()


def _device(k, hip):
    out = {"primitives": k.device_primitives().tobytes(), "lights": k.device_lights().tobytes()}
    for which in LISTS:
        for what in (E.NODE_ROWS, E.LEAF_RECORDS):
            copy = E.list_copy(hip, which, what)
            out["list %d, copy %d" % (which, what)] = None if copy is None else copy.tobytes()
    return out


def _bank_figures(k, hip):
    return (k.parked_frames(), k.frame_switches(), hip.solr_hip_parked_scenes(), hip.solr_hip_parked_bytes(), hip.solr_hip_scene_switches())


@pytest.mark.parametrize("sequence", ["moves", "material sets"])
def test_the_bank_is_off_by_default(solr, sequence):
    """the sequences of tests/test_moves_gpu.py::test_moves_on_a_frame_that_is_not_the_resident_one_take_the_host_route and of
    tests/test_material_sets_gpu.py's case other_frame, bank never set: after the switch the device still holds the frame that
    was left, word for word, nothing is parked or counted, the request takes the host route, and the frame behind it is one
    upload of the frame that was entered"""
    hip = solr.hip_lib()
    if sequence == "moves":
        k = morph_cases.build(solr.Kernel(engine="hip", deterministic_seed=1), "sticks")
    else:
        k = material_set_cases.build(solr.Kernel(engine="hip", deterministic_seed=1), "mix", size=(64, 48))
    try:
        for _ in range(3):
            gpu_frame(k)
        before = _device(k, hip)
        served = (hip.solr_hip_device_rotations(), hip.solr_hip_device_material_sets())
        uploads = (k.scene_uploads(), hip.solr_hip_scene_uploads())
        assert uploads[0] == uploads[1] == 1 and _bank_figures(k, hip) == (0, 0, 0, 0, 0)
        flat = k.flat_scene()
        k.set_frame(0)
        assert _device(k, hip) == before, "the device does not hold the frame that was left any more"
        assert _bank_figures(k, hip) == (0, 0, 0, 0, 0)
        if sequence == "moves":
            k.rotate_primitives((10.0, -20.0, 30.0), (0.11, -0.07, 0.05))
        else:
            rod = material_set_cases.first_of_type(flat, solr.ptCylinder)
            assert k.set_primitive_materials([rod], [material_set_cases.other_wall(flat, rod)]) == 0
        assert k.pending_moves() == 0, "a request on frame 0 was offered to an engine whose resident scene is frame 1"
        assert (hip.solr_hip_device_rotations(), hip.solr_hip_device_material_sets()) == served
        assert _device(k, hip) == before
        gpu_frame(k)                                    # uploads frame 0
        assert (k.scene_uploads(), hip.solr_hip_scene_uploads()) == (2, 2)
        assert _device(k, hip) != before and _bank_figures(k, hip) == (0, 0, 0, 0, 0)
        k.check(0, sequence)
    finally:
        k.finalize()
