"""The post-processing kernels of solr_post.hip held to the oracle on the synthetic frames of
tests/post_processing_cases.py - depths drawn per pixel from eight levels, random buffers that put the taps exactly on
pixels, on one side, beyond int's range - instead of rendered Cornell boxes, whose smooth depths hide a misplaced tap.

One driver.  A Cornell box of the case's size is rendered once (scene and frame are then on the device); the case's
random buffer, strip, frame buffer, ids and depth halo go in through the C ABI; solr_hip_render runs a refinement pass,
in which the camera kernel skips every pixel (ids.y = ids.w = 0, CRT:454-458) and the post-processing kernel sees
exactly what was uploaded.  The frame buffer and the ids must come back bit for bit, and the bitmap must be the
oracle's over the same buffers, byte for byte: the effects are + * / and comparisons in binary32, and the count of
k_ambientOcclusion is an integer.  No tolerance anywhere.  tests/test_post_processing_cases.py (CPU) shows that the
oracle agrees with the text model on such inputs, that the inputs tell a misplaced tap, and that the ambient-occlusion
cases reach every path of the kernel.

k_packDepthRows has no entry point of its own: tests/test_multi_rank_gpu.py reaches it through the RCCL halo exchange."""
import ctypes as C

import numpy as np
import pytest

import post_processing_cases as PC

pytestmark = pytest.mark.gpu
VARIANT_AO_FIXED_STRIDE = 9


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Engine:
    """the resident scene of a W x H frame, one frame in flight, and the case runner"""

    def __init__(self, solr, W, H, background=False):
        self.solr, self.hip = solr, solr.hip_lib()
        self.W, self.H, self.background = W, H, background
        self.k = None
        self.uploaded = None

    def __enter__(self):
        try:
            self.k = PC.stage(self.solr, self.W, self.H, engine="hip", background=self.background)
            self.k.render()
            self.flat = self.k.flat_scene()
            self.base = np.array(self.flat.randoms, copy=True)
            self.objects = self.solr.Vec4i(len(self.flat.boxes), len(self.flat.primitives), self.flat.nb_lamps,
                                           len(self.flat.lights))
        except BaseException:
            self.__exit__(None, None, None)
            raise
        return self

    def __exit__(self, *exc):
        """whatever happened: the knobs back, the one engine of the process finalized"""
        try:
            self.hip.solr_hip_set_variant(0)
            self.hip.solr_hip_set_depth_halo(None, 0, None, 0)
            self.hip.solr_hip_set_strip(0, -1)
        finally:
            if self.k is not None:
                self.k.finalize()

    def randoms(self, kind):
        rnd = PC.randoms(self.base, kind)
        if self.uploaded != kind:
            self.hip.solr_hip_h2d_randoms_sized(C.c_void_p(rnd.ctypes.data), len(rnd))
            self.k.check(0, "solr_hip_h2d_randoms_sized")
            self.uploaded = kind
        return rnd

    def run(self, c, pp, ids, rnd, variant=0):
        """case c over the whole-frame buffers (pp, ids): the engine gets the strip's rows and the halo's depths.
        -> (pp, ids, image) of the case's rows, read back, and the frame's parameters"""
        hip, k, W = self.hip, self.k, self.W
        first, count = c["strip"] if c["strip"] else (0, self.H)
        above, below = PC.halo_of(c, rnd)
        params = PC.parameters(k, c)
        si, ppi, eye, direction, angles = params
        try:
            if c["strip"]:
                hip.solr_hip_set_strip(first, count)
            spp, sids = np.ascontiguousarray(pp[first:first + count]), np.ascontiguousarray(ids[first:first + count])
            hip.solr_hip_h2d_postprocessing(C.c_void_p(spp.ctypes.data), C.c_void_p(sids.ctypes.data))
            k.check(0, "solr_hip_h2d_postprocessing")
            if above or below:
                rows_above = np.ascontiguousarray(pp[first - above:first, :, 3])
                rows_below = np.ascontiguousarray(pp[first + count:first + count + below, :, 3])
                hip.solr_hip_set_depth_halo(_fp(rows_above) if above else None, above,
                                            _fp(rows_below) if below else None, below)
                k.check(0, "solr_hip_set_depth_halo")
            hip.solr_hip_set_variant(variant)
            hip.solr_hip_render(C.byref(si), C.byref(self.objects), C.byref(ppi), _fp(eye), _fp(direction), _fp(angles))
            k.check(0, "solr_hip_render")
            gpp = np.zeros((count, W, 8), np.float32)
            hip.solr_hip_d2h_postprocessing(C.c_void_p(gpp.ctypes.data))
            gids, image = np.zeros((self.H, W, 4), np.int32), np.zeros((self.H, W, 3), np.uint8)
            hip.solr_hip_d2h(C.byref(si), C.c_void_p(image.ctypes.data), C.c_void_p(gids.ctypes.data))
            k.check(0, "solr_hip_d2h")
        finally:
            hip.solr_hip_set_variant(0)
            hip.solr_hip_set_depth_halo(None, 0, None, 0)
            if c["strip"]:
                hip.solr_hip_set_strip(0, -1)
        return gpp, gids[first:first + count], image[first:first + count], params

    def hold(self, oracle, c, variants=(0,)):
        """case c on the engine and in the oracle: the buffers untouched, the image the oracle's, byte for byte"""
        name = "%s %s" % (PC.EFFECT_NAMES[c["effect"]], PC.case_id(c))
        pp, ids = PC.case_frame(c)
        rnd = self.randoms(c["randoms"])
        first, count = c["strip"] if c["strip"] else (0, self.H)
        want = None
        for variant in variants:
            gpp, gids, image, params = self.run(c, pp, ids, rnd, variant)
            if want is None:
                want = PC.expected(oracle, self.flat, params, c, pp, ids, rnd)
            opp, oids, orgb = want
            if c["iteration"] <= 10:
                assert np.array_equal(gpp.view(np.uint32), pp[first:first + count].view(np.uint32)), \
                    name + ": the refinement pass changed the frame buffer"
                assert np.array_equal(gids, ids[first:first + count]), name + ": the refinement pass changed the ids"
            else:
                # the precondition of an accumulation pass: the sample it added is the same float on both sides
                assert np.array_equal(gpp.view(np.uint32)[..., :7], opp.view(np.uint32)[..., :7]), \
                    name + ": the frame buffers differ after the pass - the scene is not all background?"
                assert np.array_equal(gids, oids), name + ": the ids differ after the pass"
            if not np.array_equal(image, orgb):
                bad = np.argwhere((image != orgb).any(axis=-1))
                y, x = int(bad[0][0]), int(bad[0][1])
                where = ""
                if c["effect"] == PC.ppe_ambientOcclusion:
                    above, below = PC.halo_of(c, rnd)
                    paths = PC.ao_paths(c["W"], c["H"], first, count, above, below, rnd, c["param2"], heavy_first=variant == 0)
                    where = ", path %s (pipelined %s, ordered %s)" % (PC.AO_PATHS[paths["paths"][y, x]], paths["pipelined"],
                                                                      paths["ordered"])
                pytest.fail("%s, variant %d: %d of %d pixels differ, the first at x %d, row %d of the strip (frame row %d): "
                            "engine %s, oracle %s%s" % (name, variant, len(bad), count * c["W"], x, y, first + y,
                                                        image[y, x].tolist(), orgb[y, x].tolist(), where))


@pytest.mark.parametrize("c", PC.AO_CASES, ids=PC.case_id)
def test_ambient_occlusion_on_synthetic_frames(solr, oracle, c):
    """every row of AO_CASES, in the order the kernel takes its tiles by default and with a fixed stride of tiles per
    workgroup (solr_hip_set_variant(9)): the same image, the oracle's"""
    with Engine(solr, c["W"], c["H"]) as engine:
        engine.hold(oracle, c, variants=(0, VARIANT_AO_FIXED_STRIDE))


OTHER_EFFECTS = (PC.ppe_depthOfField, PC.ppe_radiosity, PC.ppe_filter, PC.ppe_cartoon)


@pytest.mark.parametrize("W,H,strip", PC.OTHER_FRAMES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("effect", OTHER_EFFECTS, ids=lambda e: PC.EFFECT_NAMES[e].replace(" ", "_"))
def test_the_other_effects_on_synthetic_frames(solr, oracle, effect, W, H, strip):
    """depth of field, radiosity, filter and cartoon over their parameter grids (OTHER_CASES) on one frame or strip: random
    indices that wrap at W H and at the strip's size, filters whose every tap wraps, param3 beyond W H, a depth that is
    param1 exactly, non-finite depths into the conversion to int, the random index shifted by the pass"""
    cases = [c for c in PC.OTHER_CASES if (c["effect"], c["W"], c["H"], c["strip"]) == (effect, W, H, strip)]
    assert cases
    with Engine(solr, W, H) as engine:
        for c in sorted(cases, key=lambda c: c["randoms"]):        # (one upload per random buffer)
            engine.hold(oracle, c)


@pytest.mark.parametrize("effect", (PC.ppe_ambientOcclusion,) + OTHER_EFFECTS, ids=lambda e: PC.EFFECT_NAMES[e].replace(" ", "_"))
def test_accumulation_pass_on_synthetic_frames(solr, oracle, effect):
    """pass 12: every effect but the cartoon divides by pathTracingIteration - 9.  The pixels are active there, so the scene is all
    background - the camera turned away from the box, no gradient, no skybox - and the sample the pass adds is the same
    float on the engine and in the oracle: first the frame buffers after the pass are the same bits, then the bitmaps"""
    W, H = 33, 9
    cases = {PC.ppe_ambientOcclusion: [PC._ao(W, H, "half", 10.0), PC._ao(W, H, "default", 2000.0)],
             PC.ppe_depthOfField: [PC._other(effect, W, H, None, "half", 7.0, 20.0, 16)],
             PC.ppe_radiosity: [PC._other(effect, W, H, None, "half", 0.0, 8.0, 12)],
             PC.ppe_filter: [PC._other(effect, W, H, None, "half", 0.0, 0.0, f) for f in (0, 3, 5)],
             PC.ppe_cartoon: [PC._other(effect, W, H, None, "half", 9000.0, 0.0, 0, view_distance=2000.0)]}[effect]
    with Engine(solr, W, H, background=True) as engine:
        for c in cases:
            engine.hold(oracle, dict(c, iteration=12))
