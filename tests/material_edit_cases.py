"""Cases and the numpy model for the tests of materials edited under a resident scene (tests/test_material_edit_cases.py,
tests/test_material_edits_gpu.py): SolR_SetMaterial between two frames, followed by the HIP engine in place
(solr_hip_edit_materials, k_retagMaterials: sol-r_amd/csrc/solr_materials.hip) when Kernel.set_material_edits is on.

The scenes are material_set_cases' (mesh, sticks, mix, plane_lamp at 64 x 48, with the three materials nobody has) and `quad`,
the textured model of tests/golden/textures with a second texture of another size loaded.  The model of a tag, a kind and a
colour key is material_set_cases' too, by import.

  a step       ("edit", material index, keyword changes): the material set anew with its values as they are and the changes
               on top (Kernel.set_material resets every value, as SolR_SetMaterial does); ("grow",): a material added
  a frame      the steps made before one frame is rendered
  a case       scene, prepare (steps made before the first frame, part of the scene), frames, and per frame what the engine
               has to do with it: "served", or why it has to decline - "kind" (a primitive of an edited material would be of
               another kind), "table" (the table has grown), "contained" (primsContained would flip)

served_model says from kind_model alone which frames change a kind; retags_model which served frames have to launch the
kernel (the facts or the colour key of a changed material differ); three_words_model what tag and colour key every primitive
has under a table."""
import ctypes as C
import importlib
import os

import numpy as np

import material_set_cases as sets
from material_set_cases import build, facts_model, key_model, kind_model, tag_model  # noqa: F401

solr = importlib.import_module("sol-r_amd")

SIZE = (64, 48)
TEXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "textures")
QUAD = os.path.join(TEXTURES, "quad.obj")
SECOND_TEXTURE = os.path.join(TEXTURES, "422_33x9.jpg")       # (the model's own is 24 x 17)
WALLS = 6                                                      # materials 0 ... 5 of morph_cases: plain, shared by the types


def keywords_of(record):
    """Kernel.set_material's keywords for a material record (MATERIAL_DTYPE) as GPUKernel::setMaterial laid it out"""
    a, t, at = record["attributes"], record["textureIds"], record["advancedTextureIds"]
    ii, sp, c = record["innerIllumination"], record["specular"], record["color"]
    return dict(r=float(c[0]), g=float(c[1]), b=float(c[2]), noise=float(ii[3]), reflection=float(record["reflection"]),
                refraction=float(record["refraction"]), procedural=bool(a[1]), wireframe=bool(a[2] != 0),
                wireframeWidth=int(a[3]), transparency=float(record["transparency"]), opacity=float(record["opacity"]),
                diffuseTextureId=int(t[0]), normalTextureId=int(t[1]), bumpTextureId=int(t[2]), specularTextureId=int(t[3]),
                reflectionTextureId=int(at[0]), transparencyTextureId=int(at[1]), ambientOcclusionTextureId=int(at[2]),
                specValue=float(sp[0]), specPower=float(sp[1]), specCoef=float(sp[3]), innerIllumination=float(ii[0]),
                illuminationDiffusion=float(ii[1]), illuminationPropagation=float(ii[2]), fastTransparency=bool(a[0] == 1))


def table_pointer(k):
    """the host's table of materials as the engine is handed it: (address, number of materials)"""
    ptr, n = C.c_void_p(), C.c_int()
    k.L.SolRx_GetMaterials(C.byref(ptr), C.byref(n))
    return ptr.value, n.value


def materials_of(k):
    """the table as records of MATERIAL_DTYPE (a copy; the primitives' store is not looked at)"""
    address, n = table_pointer(k)
    raw = (C.c_char * (n * solr.MATERIAL_DTYPE.itemsize)).from_address(address)
    return np.frombuffer(raw, solr.MATERIAL_DTYPE, n).copy()


def apply(k, step):
    if step[0] == "grow":
        k.add_material(0.3, 0.4, 0.9, specValue=0.2, specPower=30.0)
        return
    _, material, changes = step
    values = keywords_of(materials_of(k)[material])
    values.update(changes)
    k.set_material(material, **values)


def changed_materials(before, after):
    """the ids whose records differ between two tables of one length, field by field"""
    assert len(before) == len(after)
    return [i for i in range(len(after))
            if any(not np.array_equal(np.ascontiguousarray(before[i][f]).view(np.uint8), np.ascontiguousarray(after[i][f]).view(np.uint8))
                   for f in after.dtype.names)]


def served_model(flat, before, after):
    """from kind_model alone: no primitive of the flattened scene is of another kind under table `after` than under
    `before` (tables of one length)"""
    p = flat.primitives
    for material in changed_materials(before, after):
        old, new = facts_model(before[material]), facts_model(after[material])
        for t in np.unique(p["type"][p["materialId"] == material]):
            if kind_model(t, old) != kind_model(t, new):
                return False
    return True


def retags_model(before, after):
    """a served edit has to rewrite tags or colour keys: the facts or the colour key of a changed material differ"""
    return any(facts_model(before[m]) != facts_model(after[m]) or
               np.float32(key_model(before[m])).view(np.int32) != np.float32(key_model(after[m])).view(np.int32)
               for m in changed_materials(before, after))


def three_words_model(flat, table):
    """per primitive of the flattened scene: (tag, material id, bits of the colour key) under that table"""
    p = flat.primitives
    out = np.zeros((len(p), 3), np.int32)
    for slot in range(len(p)):
        m = table[int(p["materialId"][slot])]
        out[slot] = (tag_model(p["type"][slot], m), int(p["materialId"][slot]), np.float32(key_model(m)).view(np.int32))
    return out


def edited_words_model(flat, before, after):
    """the three words an edit leaves: those of `before`, and for the primitives of a changed material those of `after`"""
    words = three_words_model(flat, before)
    fresh = three_words_model(flat, after)
    touched = np.isin(flat.primitives["materialId"], changed_materials(before, after))
    words[touched] = fresh[touched]
    return words


def most_used(flat):
    return int(np.bincount(flat.primitives["materialId"]).argmax())


def _quad(k):
    solr.scenes.obj_model(k, QUAD, width=SIZE[0], height=SIZE[1], iterations=2)
    assert k.load_texture(1, SECOND_TEXTURE)
    k.extra = {}
    return k


def build_case(k, case):
    """the case's scene in kernel k, flattened, its prepare steps made"""
    if case["scene"] == "quad":
        _quad(k)
    else:
        build(k, case["scene"], size=SIZE)
    for step in case.get("prepare", lambda k, flat: [])(k, None):
        apply(k, step)
    return k


def _colour(material, n=0):
    return ("edit", material, dict(r=0.15 + 0.2 * n, g=0.85 - 0.1 * n, b=0.4 + 0.1 * n))      # (another mean for every n)


def _textured_triangle_material(flat):
    p = flat.primitives
    textured = np.flatnonzero(flat.materials["textureIds"][:, 0] >= 0)
    return int(next(m for m in textured if ((p["materialId"] == m) & (p["type"] == solr.ptTriangle)).any()))


SERVED = {
    "colour_of_the_most_used": dict(
        scene="mesh", frames=lambda k, flat: [[_colour(most_used(flat))], [_colour(most_used(flat), 1)]],
        expect=["served", "served"]),
    "transparent_and_back": dict(
        scene="sticks", frames=lambda k, flat: [[("edit", 2, dict(transparency=0.5, refraction=1.1, opacity=0.1))],
                                               [("edit", 2, dict(transparency=0.0, refraction=0.0, opacity=0.0))]],
        expect=["served", "served"]),
    "reflection_only": dict(
        scene="mix", frames=lambda k, flat: [[("edit", 1, dict(reflection=0.5))], [("edit", 1, dict(reflection=0.0, specValue=0.9))]],
        expect=["served", "served"]),
    "two_materials_apart": dict(
        scene="sticks", frames=lambda k, flat: [[_colour(0), ("edit", 3, dict(r=0.9, g=0.1, b=0.6, transparency=0.4))]],
        expect=["served"]),
    # every material of the sticks at once - the six shared ones, the lamp's, the three nobody has: ten records, beyond the
    # eight k_retagMaterials looks through one after the other (a binary search per lane); then eight, the most it does
    "ten_materials_then_eight": dict(
        scene="sticks", frames=lambda k, flat: [[("edit", m, dict(r=0.1 + 0.08 * m, g=0.9 - 0.07 * m, b=0.3 + 0.02 * m)) for m in range(10)],
                                               [("edit", m, dict(r=0.9 - 0.05 * m, g=0.2 + 0.03 * m, b=0.5)) for m in range(8)]],
        expect=["served", "served"]),
    "a_material_nobody_has": dict(
        scene="mix", frames=lambda k, flat: [[("edit", k.extra["plain"], dict(r=0.5, g=0.25, b=0.125, transparency=0.3))]],
        expect=["served"]),
    "the_lamps_colour": dict(
        scene="plane_lamp", frames=lambda k, flat: [[("edit", sets.emissive(flat), dict(r=1.0, g=0.6, b=0.3))]],
        expect=["served"]),
    "wireframe_width": dict(
        scene="sticks", frames=lambda k, flat: [[("edit", 4, dict(wireframe=True, wireframeWidth=2))],
                                               [("edit", 4, dict(wireframeWidth=5))]],
        expect=["served", "served"]),
    "texture_swapped": dict(
        scene="quad", frames=lambda k, flat: [[("edit", _textured_triangle_material(flat), dict(diffuseTextureId=1))],
                                             [("edit", _textured_triangle_material(flat), dict(diffuseTextureId=0))]],
        expect=["served", "served"]),
}

DECLINED = {
    # (walls 1, 2 and 0 of the mix: the unmovable sphere and a YZ plane, a YZ plane and the ellipsoid, the XY plane)
    "sphere_procedural": dict(scene="mix", frames=lambda k, flat: [[("edit", 1, dict(procedural=True))]], expect=["kind"]),
    "yz_plane_emissive": dict(scene="mix", frames=lambda k, flat: [[("edit", 2, dict(innerIllumination=1.0))]], expect=["kind"]),
    "plane_textured": dict(scene="mix", frames=lambda k, flat: [[("edit", 0, dict(diffuseTextureId=0))]], expect=["kind"]),
    # the table grown by a material: uploaded whole; the edit behind that upload is served again
    "table_grown": dict(scene="sticks", frames=lambda k, flat: [[("grow",), _colour(1)], [_colour(1, 1)]],
                        expect=["table", "served"]),
    # spheres whose material keeps them of the general kind (fast transparency): turned procedural they stay of that kind
    # and stop lying inside their leaves' boxes, in a scene where everything did
    "contained_flips": dict(scene="plane_lamp", prepare=lambda k, flat: [("edit", 1, dict(fastTransparency=True))],
                            frames=lambda k, flat: [[("edit", 1, dict(procedural=True))]], expect=["contained"]),
}

CASES = dict(SERVED, **DECLINED)
