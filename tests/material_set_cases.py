"""Cases and the numpy model for the tests of materials set on primitives (tests/test_material_sets_host.py,
tests/test_material_sets_gpu.py): GPUKernel::setPrimitiveMaterials on the host and on the resident scene
(solr_hip_set_primitive_materials, k_setPrimitiveMaterials).

  build          the scenes of move_cases (mesh, sticks, mix, plane_lamp) with three materials more, which no primitive has
                 at first: `procedural`, `clear` (transparent) and `plain`; k.extra names them
  facts_model    materialTag (sol-r_amd/csrc/solr_uploads.hip) restated over a record of MATERIAL_DTYPE: the bits of a
                 primitive's tag that come from its material
  kind_model     the kind rule of retagPrimitives (engine.h primitiveKind) restated: type and facts to PrimKind
  tag_model      the tag word: type | facts | kind << 24
  key_model      the colour key: (r + g) + b over 3, every step binary32
  steps          ("materials", (indices, material ids)) next to edit_cases' steps; apply() runs one through the new call,
                 by_setter() through the setter that was there before, one record at a time, then compactBoxes(false)

The model is what the GPU tests hold the three words of a served primitive to; which batches the engine has to serve and
which it has to decline is written down per case in the tests, and kind_changes() says the same from the model."""
import importlib

import numpy as np

import edit_cases
import move_cases

solr = importlib.import_module("sol-r_amd")

f32 = np.float32
NAMES = ("mesh", "sticks", "mix", "plane_lamp")
# scene_layout.h
PRIM_FAST0, PRIM_FAST1, PRIM_PROCEDURAL, PRIM_TRANSPARENT = 1 << 8, 1 << 9, 1 << 10, 1 << 11
PRIM_WIRE1, PRIM_WIRE2, PRIM_EMISSIVE, PRIM_TEXTURED = 1 << 12, 1 << 13, 1 << 14, 1 << 15
PRIM_WIDTH_SHIFT, PRIM_KIND_SHIFT = 16, 24
KIND_GENERAL, KIND_SPHERE, KIND_PLANE_XY, KIND_PLANE_YZ, KIND_PLANE_XZ, KIND_TRIANGLE, KIND_CYLINDER = range(7)
TEXTURE_NONE = solr.TEXTURE_NONE
PLANES = (solr.ptXYPlane, solr.ptYZPlane, solr.ptXZPlane)


def build(k, name, size=None):
    """scene `name` of move_cases in kernel k, flattened, with the three materials nobody has yet; size: (width, height) of
    its frames where morph_cases' 96 x 64 is not wanted"""
    import morph_cases
    usual = morph_cases.WIDTH, morph_cases.HEIGHT
    try:
        if size is not None:
            morph_cases.WIDTH, morph_cases.HEIGHT = size
        move_cases.build(k, name)
    finally:
        morph_cases.WIDTH, morph_cases.HEIGHT = usual
    k.extra = dict(procedural=k.add_material(0.7, 0.3, 0.2, procedural=True, specValue=0.5, specPower=60.0),
                   clear=k.add_material(0.8, 0.9, 1.0, refraction=1.1, transparency=0.5, opacity=0.1, specValue=1.0,
                                        specPower=120.0),
                   plain=k.add_material(0.15, 0.8, 0.35, specValue=0.4, specPower=40.0))
    return k


def facts_model(m):
    """materialTag: the facts of material record m (MATERIAL_DTYPE) the walks need in a primitive's tag"""
    a = [int(v) for v in m["attributes"]]
    facts = 0
    if a[0] == 0:
        facts |= PRIM_FAST0
    if a[0] == 1:
        facts |= PRIM_FAST1
    if a[1] != 0:
        facts |= PRIM_PROCEDURAL
    if f32(m["transparency"]) != 0:
        facts |= PRIM_TRANSPARENT
    if a[2] == 1:
        facts |= PRIM_WIRE1
    if a[2] == 2:
        facts |= PRIM_WIRE2
    if f32(m["innerIllumination"][0]) != 0:
        facts |= PRIM_EMISSIVE
    diffuse = int(m["textureIds"][0])
    # (a diffuse texture id that was never loaded keeps the "computed texture" mapping: untextured on the device)
    if diffuse >= 0 and int(m["textureMapping"][0]) == 40000 and int(m["textureMapping"][1]) == 40000 and int(m["textureOffset"][0]) == 0:
        diffuse = TEXTURE_NONE
    if diffuse != TEXTURE_NONE:
        facts |= PRIM_TEXTURED
    facts |= (min(max(a[3], -1), 100) + 1) << PRIM_WIDTH_SHIFT
    return facts


def kind_model(kind_of_primitive, facts):
    """the short path the walks may take through a primitive of that type whose material has those facts"""
    t = int(kind_of_primitive)
    if not facts & PRIM_FAST0:
        return KIND_GENERAL
    if t == solr.ptSphere and not facts & PRIM_PROCEDURAL:
        return KIND_SPHERE
    if t in PLANES and not facts & (PRIM_TEXTURED | PRIM_WIRE2) and not (t == solr.ptYZPlane and facts & PRIM_EMISSIVE):
        return {solr.ptXYPlane: KIND_PLANE_XY, solr.ptYZPlane: KIND_PLANE_YZ, solr.ptXZPlane: KIND_PLANE_XZ}[t]
    if t == solr.ptTriangle:
        return KIND_TRIANGLE
    if t in (solr.ptCylinder, solr.ptCone):
        return KIND_CYLINDER
    return KIND_GENERAL


def tag_model(kind_of_primitive, m):
    facts = facts_model(m)
    return int(kind_of_primitive) | facts | (kind_model(kind_of_primitive, facts) << PRIM_KIND_SHIFT)


def key_model(m):
    c = m["color"].astype(f32)
    return f32(f32(f32(c[0] + c[1]) + c[2]) / f32(3.0))


def three_words_model(flat, indices, material_ids):
    """per record of a batch that names no index twice: (slot, tag, material id, colour key) as a served batch leaves them"""
    slot_of = {int(index): slot for slot, index in enumerate(flat.primitives["index"])}
    out = []
    for index, material in zip(indices, material_ids):
        slot = slot_of[int(index)]
        m = flat.materials[int(material)]
        out.append((slot, tag_model(flat.primitives["type"][slot], m), int(material), key_model(m)))
    return out


def kind_changes(flat, index, material):
    """would primitive `index` of the flattened scene be of another kind with that material"""
    slot = int(np.flatnonzero(flat.primitives["index"] == index)[0])
    t = flat.primitives["type"][slot]
    old = flat.materials[int(flat.primitives["materialId"][slot])]
    return kind_model(t, facts_model(old)) != kind_model(t, facts_model(flat.materials[int(material)]))


def slots_of(flat, indices):
    slot_of = {int(index): slot for slot, index in enumerate(flat.primitives["index"])}
    return np.array([slot_of[int(i)] for i in indices], np.int32)


def first_of_type(flat, ptype, nth=0, material=None):
    """the index of the nth primitive of that type behind the lamps in the flattened order (of that material, if given)"""
    p = flat.primitives
    found = [s for s in range(flat.nb_lamps, len(p))
             if int(p["type"][s]) == ptype and (material is None or int(p["materialId"][s]) == material)]
    return int(p["index"][found[nth]])


def leaf_first_and_other(flat, strict=True):
    """the indices of two primitives of one leaf behind the lamps' cell: its first primitive - whose record the leaf record
    copies - and one that is not first.  Not strict: where every leaf holds one primitive, the primitives of the last two"""
    b = flat.boxes
    for node in range(1, len(b)):
        if b["nbPrimitives"][node] >= 2:
            start = int(b["startIndex"][node])
            return int(flat.primitives["index"][start]), int(flat.primitives["index"][start + 1])
    assert not strict, "no leaf of two primitives"
    return int(flat.primitives["index"][-1]), int(flat.primitives["index"][-2])


def other_wall(flat, index, walls=6):
    """a wall material (ids 0 ... 5 of morph_cases, all plain) other than the one primitive `index` has"""
    slot = int(np.flatnonzero(flat.primitives["index"] == index)[0])
    return (int(flat.primitives["materialId"][slot]) + 1) % walls


def emissive(flat):
    """the id of the scene's lamp material"""
    return int(np.flatnonzero(flat.materials["innerIllumination"][:, 0] != 0)[0])


def apply(k, step, lamps):
    what, arg = step
    if what == "materials":
        assert k.set_primitive_materials(*arg) == 0
    else:
        edit_cases.apply(k, step, lamps)


def by_setter(k, step, lamps):
    """the step through the calls that were there before set_primitive_materials: the setter one record at a time, in
    order, then compactBoxes(false)"""
    what, arg = step
    if what == "materials":
        for index, material in zip(*arg):
            k.L.SolR_SetPrimitiveMaterial(int(index), int(material))
        k.compact_boxes(False)
    else:
        edit_cases.apply(k, step, lamps)


def recolour_all(flat, walls=6):
    """every primitive behind the lamps, last slot first, each to the next wall material: more records than one block of
    k_setPrimitiveMaterials has threads on the mesh (289 = 256 + 33)"""
    p = flat.primitives
    slots = list(range(flat.nb_lamps, len(p)))[::-1]
    return [int(p["index"][s]) for s in slots], [(int(p["materialId"][s]) + 1) % walls for s in slots]


def mixed_steps(flat, extra):
    """material sets of the sticks among rotations, translations, a lamp move and batches of edits: one journal, in order.
    The second batch of edits names primitives the material sets before it touched: its records carry the material the
    primitive has by then"""
    p = flat.primitives
    sphere, rod = first_of_type(flat, solr.ptSphere, 2), first_of_type(flat, solr.ptCylinder, 1)
    edits = edit_cases.batches(flat, "sticks")
    first = ([sphere, rod], [extra["plain"], other_wall(flat, rod)])
    second = recolour_all(flat)
    after = dict(zip(*first))
    after.update(dict(zip(*second)))
    last = edits[1].copy()
    for r in last:
        r["materialId"] = after[int(r["index"])]
    assert not np.array_equal(last["materialId"], edits[1]["materialId"])
    return [("materials", first), ("rotate", edit_cases.TURNS[0]), ("edit", edits[0]), ("translate", edit_cases.TRANSLATIONS[0]),
            ("lamp", (0, edit_cases.LAMP_THERE)), ("materials", second), ("rotate", edit_cases.TURNS[1]), ("edit", last),
            ("materials", ([sphere], [emissive(flat)]))]
