"""The cases of tests/test_mode_content_cases.py (CPU) and tests/test_mode_content_gpu.py: the modes that only the two
F_FULL rows of the renderer carry (renderer.h ROWS: the five-ray, anaglyph, fish-eye and 3D-vision cameras, global
illumination, the box-debug view) and the modes every row carries (fog, the gradient background, random illumination),
each over every KIND of scene - not the closed Cornell room alone, in which no ray ever misses and nothing but spheres and
axis planes is hit.

Every frame is 76 x 44 (10 x 6 tiles of 8 x 8, the last column and the last row 4 pixels wide), every case passes
maxPathTracingIterations = 40 and the post-processing record POST, with which the depth-of-field jitter of the accumulation
passes (CRT:470-479: param1), the fish-eye jitter (CRT:741-813: param2) and the 3D-vision depth (param1) are all non-zero.

The scenes are the builders the other tests use, two of them made plain: with the textured sphere and the textured skybox
the oracle marks hundreds of the frame's pixels as having gone through a mis-rounded atan2f / asinf, and a frame with a
quarter of its pixels excused is a weak test (tests/test_gpu_parity.py::test_textures keeps covering those maps)."""
import importlib

import cuda_text_cases as T          # (for two_lamps_and_a_sky only)
import scenes_extra as X

solr = importlib.import_module("sol-r_amd")

W, H = 76, 44
TILE = 8
MAX_PATH_TRACING_ITERATIONS = 40
POST = dict(type=solr.ppe_none, param1=9000.0, param2=0.002, param3=0)
# the pixels of a pass that the oracle may mark as behind a mis-rounded libm result - the only ones an engine frame may
# show outside the bar: 2 % of the frame
MARKED_CAP = 2 * W * H // 100
assert MARKED_CAP == 66
# Every scene's background (open_room's of the matrix): where a ray misses, the frame shows it - a lane that missed and was
# forgotten, or a gradient flag that was ignored (rt_device.h launchRayTracing multiplies THIS colour: CRT:278-286), would
# not show against the default, which is black.
BACKGROUND = (0.3, 0.5, 0.7, 0.2)


def _plain_material(k, index, r, g, b, reflection=0.0, specValue=0.1, specPower=200.0):
    """material `index` again, as an untextured, non-procedural one (the SolR_SetMaterial call of
    test_gpu_parity.py::test_every_primitive_type_without_the_procedural_sphere)"""
    view = k.info["viewDistance"]
    k.L.SolR_SetMaterial(index, r, g, b, 0.0, reflection, 0.0, 0, 0, 0, 0.0, 0.0, -1, -1, -1, -1, -1, -1, -1, specValue,
                         specPower, 0.0, 0.0, view * 10, view, 0)


def mix_plain(k, **info):
    """every primitive type, glass, mirror, wireframe, noise; no transcendental but pow"""
    info.setdefault("timestamp", 0)
    X.primitives_mix(k, width=W, height=H, **info)
    _plain_material(k, 3, 0.3, 0.8, 0.3, specValue=0.4, specPower=30.0)      # the procedural sphere's


def tex_flat(k, **info):
    """the texture tier on planes and triangles, Mandelbrot and Julia; no atan2f / asinf UVs"""
    X.textured(k, width=W, height=H, skybox=False, **info)
    _plain_material(k, 1, 1.0, 1.0, 1.0, reflection=0.3, specValue=0.5, specPower=40.0)   # the sphere's: a plain mirror


def triangles(k, **info):
    """the lean sphere + triangle row; with F_FULL, the row of the special cameras"""
    X.triangles_only(k, width=W, height=H, **info)


def sticks(k, **info):
    """the lean sphere + cylinder row; with F_FULL, the row of the special cameras"""
    X.sticks(k, width=W, height=H, **info)


def open_sky(k, **info):
    """a plain-coloured skybox (but for the gradient modes: build), two lamps, glass, a cone, an emissive sphere; two primary
    rays in five miss"""
    T.two_lamps_and_a_sky(k, width=W, height=H, **info)


def open_room(k, **info):
    """spheres and planes with the room taken away"""
    info.setdefault("iterations", 3)
    solr.scenes.cornell(k, width=W, height=H, room=False, **info)


SCENES = {"mix_plain": mix_plain, "tex_flat": tex_flat, "triangles": triangles, "sticks": sticks, "open_sky": open_sky,
          "open_room": open_room}

CAMERA_PASSES = (0, 1, 2, 10, 11, 12)
GI_PASSES = (0, 1, 10, 11, 12, 13)

# name -> (SceneInfo changes, passes, the scenes it runs on: None for all)
# skybox=False is no SceneInfo field: build() takes the scene's skybox away (open_sky has one), because the skybox arm comes
# before the gradient arm and the gradient would never be computed under it
MODES = {
    "anaglyph": (dict(cameraType=solr.ctAnaglyph, eyeSeparation=350.0), CAMERA_PASSES, None),
    "3d-vision": (dict(cameraType=solr.ctVR, eyeSeparation=380.0), CAMERA_PASSES, None),
    "fish-eye": (dict(cameraType=solr.ctPanoramic), CAMERA_PASSES, None),
    "five-ray": (dict(cameraType=solr.ctAntialiazed), CAMERA_PASSES, None),
    "gi-basic": (dict(advancedIllumination=solr.aiBasic), GI_PASSES, None),
    "gi-full": (dict(advancedIllumination=solr.aiFull), GI_PASSES, None),
    "gi-full-gradient": (dict(advancedIllumination=solr.aiFull, gradientBackground=1, skybox=False), GI_PASSES, None),
    "random-illumination": (dict(advancedIllumination=solr.aiRandomIllumination, timestamp=7), (0, 10, 11), None),
    "boxes": (dict(renderBoxes=1), (0,), None),
    "fog": (dict(atmosphericEffect=solr.aeFog, viewDistance=30000.0), (0,), None),
    "gradient": (dict(gradientBackground=1, skybox=False), (0,), None),
    # the whole colour stack in LDS, in the rows that have no F_STACK form
    "anaglyph-10-bounces": (dict(cameraType=solr.ctAnaglyph, eyeSeparation=350.0, iterations=10), (0, 11),
                            ("mix_plain", "triangles")),
}
CAMERA_MODES = ("anaglyph", "3d-vision", "fish-eye", "five-ray", "anaglyph-10-bounces")
GI_MODES = ("gi-basic", "gi-full", "gi-full-gradient")
GRADIENT_MODES = ("gi-full-gradient", "gradient")
# the modes only an F_FULL row renders (solr_launch.hip fullFeatures); the others stay with the scene's own row
FULL_MODES = CAMERA_MODES + GI_MODES + ("boxes",)

CASES = [(scene, mode) for scene in SCENES for mode, (_, _, scenes) in MODES.items() if scenes is None or scene in scenes]


def case_id(case):
    return "%s-%s" % case


def passes_of(case):
    return MODES[case[1]][1]


def build(k, case, **changes):
    """the case's scene in kernel k (any engine), ready for pass 0; returns the case's passes.
    changes: SceneInfo changes on top of the mode's (gradientBackground=0: a gradient case's twin without the flag)"""
    scene, mode = case
    info, passes, _ = MODES[mode]
    info = dict(info, **changes)
    info.setdefault("bgColor", BACKGROUND)
    skybox = info.pop("skybox", True)
    k.set_post_processing(**POST)
    SCENES[scene](k, maxPathTracingIterations=MAX_PATH_TRACING_ITERATIONS, **info)
    if not skybox:
        k.set_scene_info(skyboxMaterialId=solr.MATERIAL_NONE)
    return passes
