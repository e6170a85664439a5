"""A numpy float32 restatement of the iso-surface arithmetic of the reference's animated scene,
apps/scenes/animation/MetaballsScene.cpp, written from its text: the yardstick sol-r_amd/csrc/iso_surface.h is held to, bit
for bit, on both engines (tests/test_iso_surface.py, tests/test_iso_surface_gpu.py).  Every operation is one binary32
operation in the order of the source; nothing is summed in float64; the balls are added one after the other (the
reference's OpenMP loop over the balls, :265-296, shares its temporaries between threads and defines no order: the serial
loop is the definition).

The table of triangles per case is NOT the reference's (MetaballsScene.h:103-377, program text that is neither copied nor
recovered): case_table() below builds the project's own from the cube's geometry, a second time and independently of the
header's generator - in floating point, from corner coordinates - and the tests compare the two.
"""
import numpy as np

f4 = np.float32

# MetaballsScene.cpp:122-130: the corners of cube (i, j, k) as offsets (di, dj, dk)
CORNERS = [(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 1, 0)]
# MetaballsScene.h:100 (verticesAtEndsOfEdges): the ends of the twelve edges, first to second
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]


class Grid:
    def __init__(self, n, size=(10.0, 12.0, 14.0), threshold=1.0, center=(1.0, -2.0, 3.5), scale=(2.0, 3.0, 0.5),
                 texture_grid=40.0):
        self.n = int(n)
        self.size = [f4(s) for s in size]
        self.threshold = f4(threshold)
        self.center = [f4(c) for c in center]
        self.scale = [f4(s) for s in scale]
        self.texture_grid = f4(texture_grid)

    def struct(self, solr):
        return solr.iso_grid(self.n, [float(s) for s in self.size], float(self.threshold),
                             [float(c) for c in self.center], [float(s) for s in self.scale], float(self.texture_grid))

    def coordinates(self, axis):
        """:99-101: (i * size.x) / gridSize - size.x / 2.f"""
        index = np.arange(self.n + 1).astype(f4)
        return (index * self.size[axis]) / f4(self.n) - self.size[axis] / f4(2.0)


def case_table():
    """[(triangles, crossed edges, loop lengths, A.d of every loop)] for the 256 cases; a triangle is three cube edges.
    The construction: crossed edges have ends that differ in their bit; a face with two crossed edges gets one segment,
    a face with four gets two, each round a corner whose bit is set; the segments close into loops, taken by lowest
    edge and begun there, turned so that (area vector) . (sum of clear end - set end) > 0, and fanned from the first edge."""
    faces = []
    for axis in range(3):
        for side in (0, 1):
            corners = [c for c in range(8) if CORNERS[c][axis] == side]
            faces.append((corners, [e for e, (a, b) in enumerate(EDGES) if a in corners and b in corners]))
    table = []
    for case in range(256):
        bit = [(case >> c) & 1 for c in range(8)]
        crossed = [e for e, (a, b) in enumerate(EDGES) if bit[a] != bit[b]]
        link = {e: [] for e in crossed}
        for corners, edges in faces:
            on = [e for e in edges if e in link]
            assert len(on) in (0, 2, 4)
            segments = []
            if len(on) == 2:
                segments = [tuple(on)]
            elif len(on) == 4:
                segments = [tuple(e for e in edges if c in EDGES[e]) for c in corners if bit[c]]
                assert len(segments) == 2
            for a, b in segments:
                link[a].append(b)
                link[b].append(a)
        assert all(len(v) == 2 for v in link.values())
        seen, triangles, lengths, dots = set(), [], [], []
        for first in crossed:
            if first in seen:
                continue
            loop, previous, current = [first], None, first
            seen.add(first)
            while True:
                a, b = link[current]
                following = b if a == previous else a
                if following == first:
                    break
                assert following not in seen
                loop.append(following)
                seen.add(following)
                previous, current = current, following
            middle = [(np.array(CORNERS[EDGES[e][0]], float) + np.array(CORNERS[EDGES[e][1]], float)) / 2 for e in loop]
            area = sum(np.cross(middle[n], middle[(n + 1) % len(loop)]) for n in range(len(loop)))
            outward = np.zeros(3)
            for e in loop:
                a, b = EDGES[e]
                inside, outside = (a, b) if bit[a] else (b, a)
                outward += np.array(CORNERS[outside], float) - np.array(CORNERS[inside], float)
            dot = float(area @ outward)
            if dot < 0:
                loop = [loop[0]] + loop[:0:-1]
            triangles += [(loop[0], loop[n], loop[n + 1]) for n in range(1, len(loop) - 1)]
            lengths.append(len(loop))
            dots.append(dot)
        table.append((triangles, crossed, lengths, dots))
    return table


_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = case_table()
    return _TABLE


def field(grid, balls):
    """:249-296: ((N+1)^3, 4) float32 of {normal x, y, z, value}, vertex (i, j, k) at (i * (N+1) + j) * (N+1) + k"""
    x, y, z = np.meshgrid(grid.coordinates(0), grid.coordinates(1), grid.coordinates(2), indexing="ij")
    value = np.zeros(x.shape, f4)
    normal = [np.zeros(x.shape, f4) for _ in range(3)]
    for ball in np.asarray(balls, f4).reshape(-1, 4):
        squared_radius = ball[3] / f4(4.0)                                      # :268
        d = [x - ball[0], y - ball[1], z - ball[2]]                             # :276-278
        squared_distance = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]              # :282-283
        squared_distance = np.where(squared_distance == f4(0.0), f4(0.0001), squared_distance).astype(f4)  # :284-285
        value = value + squared_radius / squared_distance                       # :288
        normal_scale = squared_radius / (squared_distance * squared_distance)   # :291
        normal = [normal[c] + d[c] * normal_scale for c in range(3)]            # :292-294
    out = np.stack(normal + [value], axis=-1).reshape(-1, 4)
    assert out.dtype == f4
    return out


def grid_edge(n, i, j, k, e):
    """axis * (N+1)^3 + index of the lower grid vertex of edge e of cube (i, j, k)"""
    a, b = (CORNERS[c] for c in EDGES[e])
    axis = [a[c] != b[c] for c in range(3)].index(True)
    lower = [min(a[c], b[c]) for c in range(3)]
    side = n + 1
    return axis * side ** 3 + ((i + lower[0]) * side + (j + lower[1])) * side + (k + lower[2])


def surface(solr, grid, fld):
    """:298-400 with the project's table: ISO_TRIANGLE_DTYPE records, cubes in index order, triangles in table order"""
    n, side = grid.n, grid.n + 1
    fld = np.asarray(fld, f4).reshape(side, side, side, 4)
    coordinates = [grid.coordinates(c) for c in range(3)]
    below = fld[..., 3] < grid.threshold                                                     # :309-324
    case = np.zeros((n, n, n), int)
    for c, (di, dj, dk) in enumerate(CORNERS):
        case |= below[di:di + n, dj:dj + n, dk:dk + n].astype(int) << c
    out = []
    t = table()
    for i, j, k in np.argwhere((case != 0) & (case != 255)):
        vertices = {}
        for e in t[case[i, j, k]][1]:
            at = [(i + CORNERS[c][0], j + CORNERS[c][1], k + CORNERS[c][2]) for c in EDGES[e]]
            v1, v2 = fld[at[0]], fld[at[1]]
            p1 = [coordinates[c][at[0][c]] for c in range(3)]
            p2 = [coordinates[c][at[1][c]] for c in range(3)]
            delta = (grid.threshold - v1[3]) / (v2[3] - v1[3])                               # :341
            p = [p1[c] + delta * (p2[c] - p1[c]) for c in range(3)]                          # :343-345
            normal = [v1[c] + delta * (v2[c] - v1[c]) for c in range(3)]                     # :347-349
            # :373 multiplies y by scale.x; the reference's scale is uniform, the engine uses scale.y
            position = [grid.center[c] + grid.scale[c] * p[c] for c in range(3)]
            vt = [p[0] / grid.texture_grid + f4(1.5), p[2] / grid.texture_grid + f4(1.5)]    # :371
            assert all(type(v) is f4 for v in p + normal + position + vt)
            vertices[e] = (position, normal, vt)
        for triangle in t[case[i, j, k]][0]:
            record = np.zeros((), solr.ISO_TRIANGLE_DTYPE)
            for v, e in enumerate(triangle):
                record["p"][v], record["n"][v], record["vt"][v] = vertices[e]
                record["edge"][v] = grid_edge(n, i, j, k, e)
            record["cube"] = (i * n + j) * n + k
            out.append(record)
    return np.array(out, solr.ISO_TRIANGLE_DTYPE) if out else np.zeros(0, solr.ISO_TRIANGLE_DTYPE)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- the grids the tests share ------------------------------------------------------------------------------------
def all_cases_field(seed=7):
    """N = 15: the 512 cubes at even coordinates have disjoint corners and take each of the 256 cases twice; values of
    set bits in [0.05, 0.95], of clear bits in [1.05, 3] (threshold 1); normals anything."""
    rng = np.random.RandomState(seed)
    fld = np.zeros((16, 16, 16, 4), f4)
    fld[..., :3] = rng.uniform(-1.0, 1.0, (16, 16, 16, 3)).astype(f4)
    number = 0
    for i in range(0, 16, 2):
        for j in range(0, 16, 2):
            for k in range(0, 16, 2):
                case = number % 256
                number += 1
                for c, (di, dj, dk) in enumerate(CORNERS):
                    lo, hi = (0.05, 0.95) if (case >> c) & 1 else (1.05, 3.0)
                    fld[i + di, j + dj, k + dk, 3] = f4(rng.uniform(lo, hi))
    return fld.reshape(-1, 4)


def random_field(n, seed):
    rng = np.random.RandomState(seed)
    fld = rng.uniform(-1.0, 1.0, ((n + 1) ** 3, 4)).astype(f4)
    fld[:, 3] = rng.uniform(0.0, 2.0, (n + 1) ** 3).astype(f4)
    return fld


def unbalanced_pairs(n, triangles):
    """Pairs of grid edges (x, y) that the triangles run x -> y and y -> x a different number of times, except where both
    edges lie in one boundary face of the grid (there the surface ends)."""
    side = n + 1

    def ends(edge):
        axis, vertex = divmod(int(edge), side ** 3)
        a = [vertex // (side * side), vertex // side % side, vertex % side]
        b = list(a)
        b[axis] += 1
        return a, b

    def boundary_faces(edge):
        a, b = ends(edge)
        return {(c, v) for c in range(3) for v in (0, n) if a[c] == v and b[c] == v}

    count = {}
    for e in triangles["edge"]:
        for x, y in ((e[0], e[1]), (e[1], e[2]), (e[2], e[0])):
            count[(int(x), int(y))] = count.get((int(x), int(y)), 0) + 1
    return [(x, y) for (x, y), c in count.items()
            if c != count.get((y, x), 0) and not (boundary_faces(x) & boundary_faces(y))]


def euler_characteristic(triangles):
    """vertices (distinct grid edges) - edges (distinct unordered pairs) + faces"""
    vertices = set(int(e) for e in triangles["edge"].ravel())
    edges = set()
    for e in triangles["edge"]:
        for x, y in ((e[0], e[1]), (e[1], e[2]), (e[2], e[0])):
            edges.add((min(int(x), int(y)), max(int(x), int(y))))
    return len(vertices) - len(edges) + len(triangles)


# ---- the cases of balls (grid of size 10 x 12 x 14 unless the case says otherwise) --------------------------------------
def ball_cases():
    rng = np.random.RandomState(3)
    five = np.concatenate([rng.uniform(-3.0, 3.0, (5, 3)), rng.uniform(4.0, 16.0, (5, 1))], axis=1)
    return {
        "one": dict(balls=[[0.3, -0.4, 0.2, 30.0]]),
        "merged": dict(balls=[[-1.5, 0.0, 0.1, 20.0], [1.5, 0.2, 0.0, 20.0]]),
        # size 10 puts the vertices of N = 5 at -5, -3, ... 5 and of N = 1, 2 at -5, (0,) 5: the ball sits on one of them
        "on_a_vertex": dict(balls=[[5.0, -5.0, 5.0, 25.0]], size=(10.0, 10.0, 10.0)),
        "five": dict(balls=five),
        "corner": dict(balls=[[4.0, 5.0, 6.0, 40.0]]),
        "through_the_boundary": dict(balls=[[0.3, -0.4, 0.2, 30.0]], threshold=0.2),
        "empty": dict(balls=[[0.3, -0.4, 0.2, 0.01]]),
        "no_balls": dict(balls=np.zeros((0, 4))),
    }

