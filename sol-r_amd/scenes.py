"""Synthetic scenes for the configurations named in BASELINE.json / SURVEY.md section 8(d).

Every scene is built through the same flat API a reference host would use
(SolR_AddMaterial / SolR_SetMaterial / SolR_AddPrimitive / SolR_SetPrimitive /
SolR_CompactBoxes), so the box tree and primitive order are the ones the
reference's builder produces for these calls.  All randomness comes from a
32-bit LCG with a fixed seed (the reference uses rand()).
"""
import math

from . import (ptSphere, ptCylinder, ptTriangle, ptXYPlane, ptYZPlane, ptXZPlane, glFull)


class LCG:
    """Numerical Recipes LCG; deterministic stand-in for the reference's rand()."""

    def __init__(self, seed):
        self.state = seed & 0xFFFFFFFF

    def next(self):
        self.state = (self.state * 1664525 + 1013904223) & 0xFFFFFFFF
        return self.state >> 8

    def uniform(self, lo=0.0, hi=1.0):
        return lo + (hi - lo) * (self.next() % 100000) / 100000.0


def _wall_color(rng):
    # createRandomMaterials: 0.2 + rand() % 600 / 1000 (apps/scenes/Scene.cpp:386-388)
    return [0.2 + (rng.next() % 600) / 1000.0 for _ in range(3)]


def add_light(k, position=(8000.0, 8000.0, -8000.0), radius=10.0, intensity=2.0):
    """Emissive sphere with the reference's DEFAULT_LIGHT_MATERIAL parameters
    (apps/scenes/Scene.cpp:628-633): white, innerIllumination = (2, 10*viewDistance, viewDistance)."""
    m = k.add_material(1.0, 1.0, 1.0, innerIllumination=intensity)
    return k.add_primitive(ptSphere, position, size=(radius, 0, 0), material=m, movable=0)


def add_room(k, rng, center=(0.0, 15000.0, 0.0), half=(20000.0, 20000.0, 20000.0)):
    """Six axis-aligned rectangles, the primitives GPUKernel::addRectangle emits
    (solr/engines/GPUKernel.cpp:1711-1739), one material per wall.  Floor at y = -5000
    like the viewer's ground height (CornellBoxScene.cpp:40)."""
    x, y, z = center
    w, h, d = half
    mats = [k.add_material(*_wall_color(rng), specValue=0.1, specPower=200.0) for _ in range(6)]
    ids = [
        k.add_primitive(ptXYPlane, (x, y, z + d), size=(w, h, d), material=mats[0]),
        k.add_primitive(ptXYPlane, (x, y, z - d), size=(w, h, d), material=mats[1]),
        k.add_primitive(ptYZPlane, (x - w, y, z), size=(w, h, d), material=mats[2]),
        k.add_primitive(ptYZPlane, (x + w, y, z), size=(w, h, d), material=mats[3]),
        k.add_primitive(ptXZPlane, (x, y + h, z), size=(w, h, d), material=mats[4]),
        k.add_primitive(ptXZPlane, (x, y - h, z), size=(w, h, d), material=mats[5]),
    ]
    return ids


def cornell(k, width=512, height=512, iterations=1, extra_spheres=16, glass=2, seed=2017, room=True, **scene_info):
    """BASELINE configs[0]/[1]: Cornell box, about 30 primitives (spheres + planes).

    Four reflective spheres of radius 2000 at (+-2200, 0, 0), (0, +-2200, 0)
    (apps/scenes/experiments/CornellBoxScene.cpp:42-50), a ring of small spheres and two
    glass spheres, a six-plane room, one emissive sphere.  Camera as the viewer's default
    (apps/solrViewer.cpp:178-181): eye (0, 0, -15000), look-at origin, angles (0,0,0,6400)."""
    rng = LCG(seed)
    scene_info.setdefault("graphicsLevel", glFull)
    k.initialize(width=width, height=height, nbRayIterations=iterations, **scene_info)
    for cx, cy in ((2200.0, 0.0), (-2200.0, 0.0), (0.0, 2200.0), (0.0, -2200.0)):
        c = _wall_color(rng)
        m = k.add_material(c[0], c[1], c[2], reflection=0.5, specValue=1.0, specPower=234.0)
        k.add_primitive(ptSphere, (cx, cy, 0.0), size=(2000.0, 0, 0), material=m)
    for i in range(extra_spheres):
        a = 2.0 * math.pi * i / max(extra_spheres, 1)
        c = _wall_color(rng)
        m = k.add_material(c[0], c[1], c[2], reflection=0.25 if i % 2 else 0.0, specValue=0.5, specPower=100.0)
        k.add_primitive(ptSphere, (9000.0 * math.cos(a), -4400.0, 9000.0 * math.sin(a)), size=(600.0, 0, 0),
                        material=m)
    for i in range(glass):
        m = k.add_material(0.9, 0.95, 1.0, reflection=1.0, refraction=1.1, transparency=0.7, specValue=1.0,
                           specPower=200.0)
        k.add_primitive(ptSphere, (-5000.0 + 10000.0 * i, 3500.0, -6000.0), size=(1200.0, 0, 0), material=m)
    if room:
        add_room(k, rng)
    add_light(k)
    k.compact_boxes(True)
    k.set_camera((0.0, 0.0, -15000.0))
    return k


def height_field(k, n=224, width=1920, height=1080, iterations=2, seed=1234, **scene_info):
    """BASELINE configs[2]: triangle mesh with per-vertex normals, 2*n*n triangles
    (n = 224 -> 100 352), scaled to +-10000 like apps/scenes ObjScene, one light at
    (8000, 8000, -8000) (ObjScene.cpp:98-106)."""
    rng = LCG(seed)
    k.initialize(width=width, height=height, nbRayIterations=iterations, graphicsLevel=glFull, **scene_info)
    scale = 10000.0
    phase = [rng.uniform(0.0, 6.28) for _ in range(4)]

    def f(u, v):
        return 1500.0 * (math.sin(3.0 * u + phase[0]) * math.cos(2.0 * v + phase[1]) +
                         0.5 * math.sin(7.0 * u + 5.0 * v + phase[2]))

    def point(i, j):
        u = (i / n) * 2.0 - 1.0
        v = (j / n) * 2.0 - 1.0
        return (u * scale, f(u * 3.0, v * 3.0) - 3000.0, v * scale)

    def normal(i, j):
        e = 1.0
        a, b = point(i - e, j), point(i + e, j)
        c, d = point(i, j - e), point(i, j + e)
        tx = (b[0] - a[0], b[1] - a[1], b[2] - a[2])
        tz = (d[0] - c[0], d[1] - c[1], d[2] - c[2])
        nx = tz[1] * tx[2] - tz[2] * tx[1]
        ny = tz[2] * tx[0] - tz[0] * tx[2]
        nz = tz[0] * tx[1] - tz[1] * tx[0]
        return (nx, ny, nz)

    mats = [k.add_material(*_wall_color(rng), reflection=0.3 if m % 4 == 0 else 0.0, specValue=0.6, specPower=80.0)
            for m in range(8)]
    pts = [[point(i, j) for j in range(n + 1)] for i in range(n + 1)]
    nrm = [[normal(i, j) for j in range(n + 1)] for i in range(n + 1)]
    for i in range(n):
        for j in range(n):
            m = mats[((i // 28) + (j // 28)) % len(mats)]
            a, b, c, d = pts[i][j], pts[i + 1][j], pts[i + 1][j + 1], pts[i][j + 1]
            na, nb, nc, nd = nrm[i][j], nrm[i + 1][j], nrm[i + 1][j + 1], nrm[i][j + 1]
            t = k.add_primitive(ptTriangle, a, b, c, material=m)
            k.set_normals(t, na, nb, nc)
            t = k.add_primitive(ptTriangle, a, c, d, material=m)
            k.set_normals(t, na, nc, nd)
    add_light(k)
    k.compact_boxes(True)
    k.set_camera((0.0, 4000.0, -15000.0))
    return k


def molecule(k, atoms=50000, width=1920, height=1080, iterations=3, seed=4321, **scene_info):
    """BASELINE configs[3]: synthetic molecule - spheres of radius 30..60 (scaled) on a
    jittered helix plus half-bond cylinders of radius 10 as io/PDBReader.cpp:616-695 emits
    them, 119 flat element materials (PDBReader.cpp:57,392-399), light at
    (-5000, 5000, -15000) (apps/scenes/science/MoleculeScene.cpp:83-89)."""
    rng = LCG(seed)
    k.initialize(width=width, height=height, nbRayIterations=iterations, graphicsLevel=glFull, **scene_info)
    mats = [k.add_material(*_wall_color(rng), specValue=0.8, specPower=100.0) for _ in range(119)]
    scale = 2.0
    turns = max(atoms // 400, 1)
    prev = None
    for a in range(atoms):
        t = a / atoms
        ang = 2.0 * math.pi * turns * t
        rad = 3000.0 + 2500.0 * math.sin(9.0 * math.pi * t)
        p = (rad * math.cos(ang) + rng.uniform(-300, 300), (t - 0.5) * 16000.0 + rng.uniform(-300, 300),
             rad * math.sin(ang) + rng.uniform(-300, 300))
        e = rng.next() % 119
        r = (30.0 + (rng.next() % 31)) * scale
        k.add_primitive(ptSphere, p, size=(r, 0, 0), material=mats[e])
        if prev is not None and a % 2 == 0:
            mid = tuple((p[i] + prev[0][i]) * 0.5 for i in range(3))
            k.add_primitive(ptCylinder, prev[0], mid, size=(10.0 * scale, 0, 0), material=mats[prev[1]])
            k.add_primitive(ptCylinder, mid, p, size=(10.0 * scale, 0, 0), material=mats[e])
        prev = (p, e)
    add_light(k, position=(-5000.0, 5000.0, -15000.0))
    k.compact_boxes(True)
    k.set_camera((0.0, 0.0, -15000.0))
    return k


def irt_model(k, path, width=1920, height=1080, iterations=3, scale=5000.0, floor=True, **scene_info):
    """A scene around an .irt model file (reference: FileMarshaller::loadFromFile, the viewer's
    "load scene"): material slots for the file's ids first - the loader overwrites them - then the
    model scaled to `scale` units of height, a floor and the default light.  medias/irt/test.irt of the
    reference is the sample of the format."""
    k.initialize(width=width, height=height, nbRayIterations=iterations, graphicsLevel=glFull, **scene_info)
    for _ in range(64):                      # the ids a file may carry; test.irt uses 0..15
        k.add_material(0.5, 0.5, 0.5)
    ground = k.add_material(0.55, 0.5, 0.45, reflection=0.2, specValue=0.5, specPower=100.0)
    n = k.load_from_file(path, scale)
    if floor:
        k.add_primitive(ptXZPlane, (0.0, -0.5 * scale - 50.0, 0.0), size=(20000.0, 0.0, 20000.0), material=ground,
                        movable=0)
    add_light(k, position=(-6000.0, 9000.0, -9000.0))
    k.compact_boxes(True)
    k.set_camera((0.0, 0.3 * scale, -3.2 * scale), look_at=(0.0, 0.0, 0.0))
    return k


def obj_model(k, path, width=1920, height=1080, iterations=3, scale=5000.0, **scene_info):
    """A scene around a Wavefront OBJ model (reference: OBJReader::loadModelFromFile; the viewer's
    Cornell-box scene loads medias/obj/cornell.obj this way): the model auto-scaled to `scale` and
    centred, its MTL materials from id 0, one light inside."""
    k.initialize(width=width, height=height, nbRayIterations=iterations, graphicsLevel=glFull, **scene_info)
    for _ in range(64):                      # ids for the MTL file's materials, overwritten by the loader
        k.add_material(0.5, 0.5, 0.5)
    ground = k.load_obj_model(path, material_id=0, auto_scale=True, scale=scale, auto_center=True)
    add_light(k, position=(0.0, 0.35 * scale, -0.1 * scale), radius=0.02 * scale)
    k.compact_boxes(True)
    k.set_camera((0.0, 0.0, -1.6 * scale), look_at=(0.0, 0.0, 0.0))
    return ground


def swc_morphology(k, path, width=1920, height=1080, iterations=3, scale=40.0, **scene_info):
    """A scene around an SWC neuron morphology (reference: SWCReader::loadMorphologyFromFile, its SwcScene):
    spheres and cylinders along the sample points, one material, a light."""
    k.initialize(width=width, height=height, nbRayIterations=iterations, graphicsLevel=glFull, **scene_info)
    m = k.add_material(0.85, 0.75, 0.35, specValue=0.6, specPower=80.0)
    n = k.load_swc_morphology(path, scale=(scale, scale, scale, scale), material_id=m)
    add_light(k, position=(-6000.0, 9000.0, -12000.0))
    k.compact_boxes(True)
    k.set_camera((0.0, 2000.0, -16000.0), look_at=(0.0, 2000.0, 0.0))
    return n


def swc_walk(k, samples, lamp, light_material, step, state):
    """One frame of the reference's SwcScene::doAnimate (apps/scenes/science/SwcScene.cpp:66-89): the primitive marked by
    the frame before gets its material back, the primitive of sample `step % len(samples)` gets `light_material`, and the
    lamp - primitive `lamp`, SolR_GetLight(0) - is moved next to that sample, to (x, y, z - 50) in binary32; both requests
    flatten with compactBoxes(false).  samples: Kernel.swc_samples().  The reference looks the sample up by that number as
    its id; an id the morphology has none for reads as a sample of zeros there (primitive 0 at the origin), and so it does
    here.  state: a dict the caller keeps between the frames, empty before the first; it holds what is marked and, read once
    before anything is pending, the materials of the samples' primitives - valid while nobody else sets those.  With the HIP
    engine and an untouched resident scene both requests run on the device (Kernel.set_primitive_materials,
    Kernel.set_primitive_center).  Returns the index of the primitive that is marked now."""
    import numpy as np
    if "materials" not in state:
        state["by_id"] = {int(s["id"]): s for s in samples}
        state["materials"] = {p: k.get_primitive_material(p) for p in sorted({0} | {int(s["primitiveId"]) for s in samples})}
        state["marked"] = None
    sample = state["by_id"].get(step % max(len(samples), 1))
    primitive = int(sample["primitiveId"]) if sample is not None else 0
    x, y, z = (np.float32(sample[c]) if sample is not None else np.float32(0.0) for c in "xyz")
    indices, materials = [], []
    if state["marked"] is not None:
        indices.append(state["marked"])
        materials.append(state["materials"][state["marked"]])
    indices.append(primitive)
    materials.append(light_material)
    if k.set_primitive_materials(indices, materials) != 0:
        raise RuntimeError("swc_walk: primitive %s is not in the store" % indices)
    state["marked"] = primitive
    k.set_primitive_center(lamp, (float(x), float(y), float(np.float32(z - np.float32(50.0)))))
    return primitive


def material_pulse(k, material, timer, **values):
    """One frame of a host that edits one material per frame (SolR_SetMaterial): material `material` gets a colour along a
    sine of `timer` - a frame count - and, every other frame, transparency 0.5 with a refraction index, else 0: the colour
    alone changes the colour key of the primitives that have the material, the transparency what their tags carry of it, which
    is also another row of the renderer's launch table for a scene that had nothing transparent.  values: further keywords
    of Kernel.set_material, the same every frame.  With Kernel.set_material_edits(True) the HIP engine follows the edit on the
    resident scene.  Returns the keywords the material was set with."""
    step = int(timer)
    clear = step % 2 == 1
    edit = dict(values)
    edit.update(r=0.5 + 0.5 * math.sin(0.37 * timer), g=0.5 + 0.5 * math.sin(0.37 * timer + 2.1),
                b=0.5 + 0.5 * math.sin(0.37 * timer + 4.2), transparency=0.5 if clear else 0.0,
                refraction=1.1 if clear else 0.0, opacity=0.1 if clear else 0.0)
    k.set_material(material, **edit)
    return edit


def pdb_molecule(k, path, width=1920, height=1080, iterations=3, geometry_type=3, scale=200.0, **scene_info):
    """A scene around a PDB molecule (reference: PDBReader::loadAtomsFromFile as its MoleculeScene calls it:
    atom size 100, stick size 10, scale 200, materials by element; light at (-5000, 5000, -15000))."""
    k.initialize(width=width, height=height, nbRayIterations=iterations, graphicsLevel=glFull, **scene_info)
    for _ in range(1100):                    # ids the reader writes or refers to (0..118, 1000, 1010)
        k.add_material(0.5, 0.5, 0.5, specValue=1.0, specPower=100.0)
    k.load_molecule(path, geometry_type=geometry_type, atom_size=100.0, stick_size=10.0, material_type=0, scale=scale)
    add_light(k, position=(-5000.0, 5000.0, -15000.0), radius=1.0)
    k.compact_boxes(True)
    k.set_camera((0.0, 0.0, -15000.0), look_at=(0.0, 0.0, 0.0))
    return k


def metaball_positions(timer, count=50, amplitude=(50.0, 50.0, 50.0), ratio=0.1):
    """(count, 4) float32 of x, y, z, squared radius: squared radius 5 + i (MetaballsScene.cpp:147) and the trajectories
    of apps/scenes/animation/MetaballsScene.cpp:214-241 about the origin - the branch that moves the balls with its
    skeleton centre at 0, its ratio 0.1 and the plain build's amplitude size / 3 (:49)."""
    import numpy as np
    out = np.zeros((count, 4), np.float32)
    ax, ay, az = amplitude
    for i in range(count):
        t = i * 3 + timer * 40.0
        c = 2.0 * math.cos(t / 600)
        z = abs(ratio * az * math.sin(math.cos(t / ((500, 400, 450, 450)[i % 4] + i))) - c)
        if i % 4 == 0:
            x = -ratio * ax * math.cos(t / (740 + i * count)) - c
            y = ratio * ay * math.sin(t / (620 + i * count)) - c
        elif i % 4 == 1:
            x = ratio * ax * math.sin(t / (420 + i * count)) + c
            y = -ratio * ay * math.cos(t / (340 + i * count)) - c
        elif i % 4 == 2:
            x = ratio * ax * math.cos(t / (820 + count)) - 0.2 * math.sin(t / 600)
            y = ratio * ay * math.sin(t / (512 + count)) - 0.2 * math.sin(t / 400)
        else:
            x = ratio * ax * math.cos(t / (1200 + count)) - 0.4 * math.sin(t / 1250)
            y = ratio * ay * math.sin(t / (2120 + count)) - 0.4 * math.sin(t / 640)
        out[i] = (x, y, z, 5.0 + i)
    return out


def metaballs(k, timer=0.0, width=512, height=512, iterations=3, balls=None, grid_size=50, count=50, size=150.0,
              scale=40.0, center=(0.0, 0.0, -2500.0), threshold=1.0, seed=2017, **scene_info):
    """One frame of the reference's MetaballsScene (apps/scenes/animation/MetaballsScene.cpp:150-419), geometry made anew
    every frame: resetFrame, the iso-surface of the balls as triangles (Kernel.add_metaballs: grid 50, 50 balls of squared
    radius 5 + i, size 150, scale 40, centre (0, 0, -2500)), the Cornell box, the lamp at (-10000, 10000, -10000) of radius
    500, compactBoxes(true).  Call it again with the next timer value (the reference steps it by 1.5) for the next
    frame; the first call initialises the kernel and makes the materials.

    In the reference's plain build the balls never leave the origin: only its Kinect and Leap branches move them.  This
    scene moves them on the trajectories of :214-241 about the origin (metaball_positions); `balls` overrides them.
    Returns the number of triangles of the surface."""
    metaballs_begin(k, width=width, height=height, iterations=iterations, seed=seed, **scene_info)
    m = k.metaballs_materials
    if balls is None:
        balls = metaball_positions(timer, count=count, amplitude=(size / 3.0,) * 3)
    k.reset_frame()
    n = k.add_metaballs(balls, grid_size=grid_size, size=(size,) * 3, threshold=threshold, center=center,
                        scale=(scale,) * 3, material=m["surface"])
    metaballs_surroundings(k)
    k.compact_boxes(True)
    return n


def metaballs_begin(k, width=512, height=512, iterations=3, seed=2017, **scene_info):
    """what comes before the first frame: the kernel initialised, the materials, the camera (nothing on later calls)"""
    if k.initialized and getattr(k, "metaballs_materials", None):
        return
    rng = LCG(seed)
    scene_info.setdefault("graphicsLevel", glFull)
    k.initialize(width=width, height=height, nbRayIterations=iterations, **scene_info)
    c = _wall_color(rng)
    k.metaballs_materials = dict(
        surface=k.add_material(c[0], c[1], c[2], reflection=0.3, specValue=1.0, specPower=100.0),
        walls=[k.add_material(*_wall_color(rng), specValue=0.1, specPower=200.0) for _ in range(6)],
        lamp=k.add_material(1.0, 1.0, 1.0, innerIllumination=2.0))
    k.set_camera((0.0, 0.0, -15000.0))


def metaballs_surroundings(k):
    """what MetaballsScene.cpp:403-413 adds after the surface: the Cornell box (six rectangles) and the lamp"""
    m = k.metaballs_materials
    x, y, z, w, h, d = 0.0, 15000.0, 0.0, 20000.0, 20000.0, 20000.0
    walls = ((ptXYPlane, (x, y, z + d)), (ptXYPlane, (x, y, z - d)), (ptYZPlane, (x - w, y, z)),
             (ptYZPlane, (x + w, y, z)), (ptXZPlane, (x, y + h, z)), (ptXZPlane, (x, y - h, z)))
    for (ptype, p0), material in zip(walls, m["walls"]):
        k.add_primitive(ptype, p0, size=(w, h, d), material=material)
    k.add_primitive(ptSphere, (-10000.0, 10000.0, -10000.0), size=(500.0, 0, 0), material=m["lamp"], movable=0)


def _animation_depth(count):
    """the depth GPUKernel::compactBoxes(true) gives a tree of `count` primitives (GPUKernel.cpp:1062-1071 of the reference)"""
    depth = 0
    while True:
        depth += 1
        count //= 4
        if count <= 2:
            return depth


def animation(k, frames=4, cells=5, width=203, height=131, iterations=2, seed=2019, **scene_info):
    """The reference's AnimationScene restated (apps/scenes/animation/AnimationScene.cpp:55-109): `frames` frames, each a
    mesh of its own - there one OBJ file per frame, here a height field of (cells + frame) x (cells + frame) cells, so every
    frame has another primitive count and another tree - with the reference's Cornell box and lamp sphere, and
    compactBoxes(true) per frame.  A displayed frame is animation_step.  compactBoxes(false) flattens with the depth of the
    tree built last, here as in the reference, so the frames must all come to the same depth: ValueError otherwise.
    Leaves frame 0 current; k.animation holds the number of frames, the primitives per frame and the lamp's material."""
    rng = LCG(seed)
    counts = [2 * (cells + f) ** 2 + 7 for f in range(frames)]
    if len({_animation_depth(c) for c in counts}) != 1:
        raise ValueError("animation: frames of %s primitives come to trees of different depths" % counts)
    scene_info.setdefault("graphicsLevel", glFull)
    k.initialize(width=width, height=height, nbRayIterations=iterations, **scene_info)
    surface = k.add_material(*_wall_color(rng), reflection=0.3, specValue=1.0, specPower=100.0)
    walls = [k.add_material(*_wall_color(rng), specValue=0.1, specPower=200.0) for _ in range(6)]
    lamp = k.add_material(1.0, 1.0, 1.0, innerIllumination=2.0)
    k.set_nb_frames(frames)
    x, y, z, w, h, d = 0.0, 15000.0, 0.0, 20000.0, 20000.0, 20000.0
    box = ((ptXYPlane, (x, y, z + d)), (ptXYPlane, (x, y, z - d)), (ptYZPlane, (x - w, y, z)),
           (ptYZPlane, (x + w, y, z)), (ptXZPlane, (x, y + h, z)), (ptXZPlane, (x, y - h, z)))
    for f in range(frames):
        k.set_frame(f)
        n = cells + f
        phase = 0.7 * f

        def point(i, j):
            u, v = (i / n) * 2.0 - 1.0, (j / n) * 2.0 - 1.0
            return (u * 7000.0, 1500.0 * math.sin(3.0 * u + phase) * math.cos(2.0 * v - phase) - 2500.0, v * 7000.0)

        for i in range(n):
            for j in range(n):
                a, b, c, e = point(i, j), point(i + 1, j), point(i + 1, j + 1), point(i, j + 1)
                k.add_primitive(ptTriangle, a, b, c, material=surface)
                k.add_primitive(ptTriangle, a, c, e, material=surface)
        for (ptype, p0), material in zip(box, walls):
            k.add_primitive(ptype, p0, size=(w, h, d), material=material)
        k.add_primitive(ptSphere, (-10000.0, 10000.0, -10000.0), size=(500.0, 0, 0), material=lamp, movable=0)
        k.compact_boxes(True)
    k.set_frame(0)
    k.set_camera((0.0, 3000.0, -15000.0))
    k.animation = dict(frames=frames, counts=counts, lamp_material=lamp)
    return k


def animation_step(k, i):
    """One displayed frame of the reference's AnimationScene::doAnimate: setFrame(i mod frames), compactBoxes(false).  With the
    frame bank on (Kernel.set_frame_bank) a frame the engine was given before comes back with no flatten and no upload."""
    frame = i % k.animation["frames"]
    k.set_frame(frame)
    k.compact_boxes(False)
    return frame


WATER_CELLS = 24


def water_edits(timer, first=0, material=0, cells=WATER_CELLS, scale=(4000.0, 1200.0, 4000.0)):
    """One frame of the reference's torus animation (apps/scenes/animation/WaterScene.cpp: a torus of cells x cells cells whose
    height follows sin(u + timer) + cos(t + 2 timer)) as a batch for Kernel.set_primitives: 2 cells^2 records of EDIT_DTYPE -
    1152 triangles at 24 x 24 - with per-vertex normals and texture coordinates, for the primitives first, first + 1 ... in
    cell order.  The vertices are worked out here, in binary64 and rounded once, so whoever takes the batch - the three
    setters one record at a time, or set_primitives on either route - gets the same floats."""
    import numpy as np
    from . import EDIT_DTYPE, EDIT_NORMALS, EDIT_TEXTURE_COORDINATES
    step = 2.0 * math.pi / cells
    grid = -math.pi + step * np.arange(cells + 1)
    t, u = np.meshgrid(grid, grid, indexing="ij")

    def surface(t, u):
        ring = scale[0] + scale[1] * np.cos(u)
        return np.stack([np.cos(t) * ring, scale[1] * (np.sin(u + timer) + np.cos(t + 2.0 * timer)),
                         np.sin(t) * (scale[2] + scale[1] * np.cos(u))], axis=-1)

    points = surface(t, u)
    e = 1.0e-3
    normals = np.cross(surface(t, u + e) - surface(t, u - e), surface(t + e, u) - surface(t - e, u))
    uv = np.stack([(t + math.pi) / (2.0 * math.pi), (u + math.pi) / (2.0 * math.pi)], axis=-1)
    batch = np.zeros(2 * cells * cells, EDIT_DTYPE)
    batch["index"] = first + np.arange(len(batch))
    batch["materialId"] = material
    batch["flags"] = EDIT_NORMALS | EDIT_TEXTURE_COORDINATES
    # per cell the triangles (a, b, c) and (a, c, d) of its corners a (i, j), b (i + 1, j), c (i + 1, j + 1), d (i, j + 1)
    corners = {"a": (slice(0, -1), slice(0, -1)), "b": (slice(1, None), slice(0, -1)), "c": (slice(1, None), slice(1, None)),
               "d": (slice(0, -1), slice(1, None))}
    for half, names in enumerate(("abc", "acd")):
        for vertex, name in enumerate(names):
            at = corners[name]
            batch["p%d" % vertex][half::2] = points[at].reshape(-1, 3)
            batch["n%d" % vertex][half::2] = normals[at].reshape(-1, 3)
            batch["vt%d" % vertex][half::2] = uv[at].reshape(-1, 2)
    return batch


def water(k, timer=0.0, width=1920, height=1080, iterations=2, seed=77, **scene_info):
    """The reference's WaterScene restated: the torus of water_edits at `timer` as 1152 textured triangles - the
    primitives k.water["first"] ... of material k.water["material"] -, a floor under it and one light.  A frame of the
    animation is k.set_primitives(water_edits(t, **k.water))."""
    import numpy as np
    rng = LCG(seed)
    k.initialize(width=width, height=height, nbRayIterations=iterations, graphicsLevel=glFull, **scene_info)
    k.set_texture(0, np.fromfunction(lambda y, x, c: ((x // 8 + y // 8) % 2) * 120 + 60 + 25 * c, (64, 64, 3)).astype(np.uint8))
    surface = k.add_material(*_wall_color(rng), reflection=0.2, specValue=1.0, specPower=100.0, diffuseTextureId=0)
    floor = k.add_material(*_wall_color(rng), specValue=0.1, specPower=200.0)
    batch = water_edits(timer, 0, surface)
    first = None
    for e in batch:
        t = k.add_primitive(ptTriangle, e["p0"], e["p1"], e["p2"], material=surface)
        k.set_normals(t, e["n0"], e["n1"], e["n2"])
        k.set_texture_coordinates(t, e["vt0"], e["vt1"], e["vt2"])
        first = t if first is None else first
    k.add_primitive(ptXZPlane, (0.0, -4000.0, 0.0), size=(12000.0, 0.0, 12000.0), material=floor)
    add_light(k)
    k.water = dict(first=first, material=surface)
    k.compact_boxes(True)
    k.set_camera((0.0, 5000.0, -14000.0))
    return k
