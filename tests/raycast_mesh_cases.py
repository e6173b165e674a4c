"""Constructed scenes with triangle meshes, per-env hulls and per-env ids for the ray caster, in the style of
tests/raycast_cases.py; shared by tests/test_raycast_mesh.py (CPU: the reference alone) and tests/test_gpu_raycast_mesh.py
(the kernel against the reference).

  "meshes"  a ground plane; meshes of 1, 12 (a closed box, on a kinematic-style body row whose pose is tilted at random per
            env) and 17 triangles (a fan: one BVH node for the first two, two levels for the third); a sphere in front of
            the box; a per-env MESH slot (a tetrahedron, a square, or NONE, by env); a per-env CONVEX slot with two
            different hulls across envs and NONE in every third env; a sphere slot with per-env ids.
  "terrain" a heightfield of 13 x 13 cells, 338 triangles (three BVH levels), with a ball resting on it; cameras of
            32 x 24, 17 x 5 and 1 x 1.
  "inside"  a camera inside a closed box mesh (a room of 12 triangles whose winding faces outward: only back faces are
            seen) with a ball and a hull in the room.
  "many"    70 balls, then a mesh: 72 shapes, the mesh in the second staged chunk of 64 (MSSIM_RAYCAST_CHUNK).

CONFIGS lists the (scene, N) pairs. MEASURED_MESH is the largest difference between the float32 and the float64 run of the
reference (tests/raycast_mesh_reference.py) over the unambiguous pixels of every image of CONFIGS where both runs hit
something, measured on the CPU by test_raycast_mesh.py::test_float32_reference_within_measured; the GPU test allows the
kernel's float depth 4 x that (the MEASURED convention of raycast_cases.py).
"""
import functools

import numpy as np

from tests import raycast_cases as rcc
from tests import raycast_mesh_reference as rmr
from tests import raycast_reference as rr

# largest |t_f32 - t_f64| in metres (see above; 2.51e-6 measured): on the ground plane of "meshes" and "many" some 5 m away
# (their cameras' far limit), a few float32 roundings of a depth of that size
MEASURED_MESH = 2.6e-6
N_ROWS = rcc.N_ROWS

CONFIGS = (("meshes", 1), ("meshes", 3), ("meshes", 67), ("terrain", 3), ("inside", 1), ("inside", 3), ("many", 3))

_BOX_FACES = np.array([[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]])


def box_mesh(half):
    """the 12 triangles of a box about the origin, wound outward"""
    h = np.asarray(half, dtype=np.float64)
    verts = np.array([[(h if (i >> k) & 1 else -h)[k] for k in range(3)] for i in range(8)])
    return verts, _BOX_FACES


def fan_mesh(n=17, radius=0.22, rise=0.1):
    """n triangles about an apex above a ring: a shallow cone without its base"""
    ring = [(radius * np.cos(2 * np.pi * i / n), radius * np.sin(2 * np.pi * i / n), 0.0) for i in range(n)]
    verts = np.array([(0.0, 0.0, rise)] + ring)
    return verts, np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)])


def heightfield(cells=13, size=2.4, amplitude=0.12, seed=5):
    rng = np.random.default_rng(seed)
    g = np.linspace(-size / 2, size / 2, cells + 1)
    z = amplitude * rng.uniform(-1, 1, size=(cells + 1, cells + 1))
    verts = np.array([(g[i], g[j], z[i, j]) for i in range(cells + 1) for j in range(cells + 1)])
    idx = lambda i, j: i * (cells + 1) + j
    tris = []
    for i in range(cells):
        for j in range(cells):
            tris += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    return verts, np.array(tris)


class MeshTables(rcc.SceneTables):
    """SceneTables plus the triangle tables, per-env plane ranges and per-env ids"""

    def __init__(self, N):
        super().__init__(N)
        self.soup, self.nodes, self.env_planes, self.env_seg = [], [], {}, {}

    def mesh(self, verts, tris):
        """adds a mesh to the tables as model/compile.py does -> (first triangle, count, root node, radius about the origin)"""
        from maniskill_amd.model import mesh

        soup = mesh.triangle_soup(np.asarray(verts, dtype=np.float64), np.asarray(tris))
        nodes = mesh.build_bvh16(soup)
        refs = nodes[:, 96:].view(np.int32)
        n_nodes0, n_tri0 = sum(len(x) for x in self.nodes), sum(len(x) for x in self.soup)
        leaf = (refs < 0) & (refs != -2**31)
        refs[refs >= 0] += n_nodes0
        refs[leaf] = ~((~refs[leaf]) + n_tri0)
        self.soup.append(soup)
        self.nodes.append(nodes)
        return n_tri0, len(soup), n_nodes0, float(np.linalg.norm(np.asarray(verts), axis=1).max())

    def hull(self, planes):
        first = len(self.planes)
        self.planes.extend(np.asarray(planes).tolist())
        return first, len(planes)

    def add_mesh(self, row, frame, m, seg, env=None):
        self.add(rr.TRIMESH, row, frame, (m[0], m[1], m[2]), seg=seg, bound_r=m[3], env=env)

    def arrays(self):
        out = super().arrays()
        ne = len(self.env)
        out["tri_soup"] = np.ascontiguousarray(np.concatenate(self.soup)) if self.soup else np.zeros((0, 12), dtype=np.float32)
        out["tri_bvh"] = np.ascontiguousarray(np.concatenate(self.nodes)) if self.nodes else np.zeros((0, 112), dtype=np.float32)
        if self.env_planes:
            a = np.zeros((ne, 2, self.N), dtype=np.int32)
            for slot, ranges in self.env_planes.items():
                a[slot] = np.asarray(ranges, dtype=np.int32).T
            out["env_shape_planes"] = np.ascontiguousarray(a.reshape(2 * ne, self.N))
        if self.env_seg:
            a = np.zeros((ne, self.N), dtype=np.int16)
            for slot in range(ne):
                shape = self.rows["shape_env_slot"].index(slot)
                a[slot] = self.env_seg.get(slot, self.rows["shape_seg"][shape])
            out["env_shape_seg"] = a
        return out


def bvh_height(nodes, root):
    refs = nodes[root, 96:].view(np.int32)
    boxes = nodes[root, :96].reshape(16, 6)
    kids = [int(r) for r, b in zip(refs, boxes) if b[0] <= b[3] and r >= 0]
    return 1 + max((bvh_height(nodes, k) for k in kids), default=0)


@functools.lru_cache(maxsize=None)
def build(name, N):
    """-> dict(scene arrays, cameras [dict], rigid [N_ROWS * N, 13] float32, N, meshes: name -> (first, count, root, radius))"""
    rng = np.random.default_rng({"meshes": 21, "terrain": 22, "inside": 23, "many": 24}[name] * 1000 + N)
    T = MeshTables(N)
    meshes = {}
    e_idx = np.arange(N)
    if name == "meshes":
        T.add(rr.PLANE, -1, (0, 0, 0, *rcc.GROUND_Q), seg=1)
        meshes["one"] = T.mesh([(0, -0.2, -0.15), (0, 0.25, -0.1), (0.05, 0.0, 0.3)], [[0, 1, 2]])
        meshes["box"] = T.mesh(*box_mesh((0.12, 0.09, 0.06)))
        meshes["fan"] = T.mesh(*fan_mesh())
        meshes["tetra"] = T.mesh([(0.1, 0, -0.07), (-0.05, 0.09, -0.07), (-0.05, -0.09, -0.07), (0, 0, 0.1)], [[0, 1, 2], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
        meshes["square"] = T.mesh([(0, -0.1, -0.1), (0, 0.1, -0.1), (0, 0.1, 0.1), (0, -0.1, 0.1)], [[0, 1, 2], [0, 2, 3]])
        T.add_mesh(-1, (0.45, 0.5, 0.35, 1, 0, 0, 0), meshes["one"], seg=2)           # faces the camera
        T.add_mesh(0, rcc.IDENT, meshes["box"], seg=3)              # on body row 0: a random tilt per env
        T.add(rr.SPHERE, 1, rcc.IDENT, (0.07,), seg=4)               # in front of the box, seen from the camera
        T.add_mesh(-1, (0.2, -0.45, 0.12, 1, 0, 0, 0), meshes["fan"], seg=5)
        # a per-env mesh slot: a tetrahedron, a square or nothing
        kind = e_idx % 3
        frames = np.tile(np.array([[-0.1, 0.55, 0.2, *rcc.random_quat(rng)]]), (N, 1))
        own = [meshes["tetra"], meshes["square"], meshes["tetra"]]
        param = np.array([[*own[k][:3], (rr.TRIMESH + 1) if k < 2 else (rr.NONE + 1)] for k in kind], dtype=np.float64)
        bound = np.array([[*frames[e, :3], own[k][3]] for e, k in enumerate(kind)])
        T.add_mesh(-1, frames[0], meshes["tetra"], seg=6, env=dict(frame=frames, param=param, bound=bound))
        # a per-env hull slot: two hulls and nothing
        hulls = [rcc.hull_planes(rng, scale=0.08), rcc.hull_planes(rng, n_points=9, scale=0.1)]
        ranges = [T.hull(h[0]) for h in hulls]
        kind = (e_idx + 1) % 3
        frames = np.tile(np.array([[-0.35, -0.4, 0.25, *rcc.random_quat(rng)]]), (N, 1))
        param = np.array([[0, 0, 0, (rr.CONVEX + 1) if k < 2 else (rr.NONE + 1)] for k in kind], dtype=np.float64)
        bound = np.array([[*frames[e, :3], hulls[min(k, 1)][1]] for e, k in enumerate(kind)])
        slot = len(T.env)
        T.add(rr.CONVEX, -1, frames[0], seg=7, bound_r=hulls[0][1], env=dict(frame=frames, param=param, bound=bound))
        T.rows["shape_planes"][-1] = list(ranges[0])
        T.env_planes[slot] = [ranges[min(k, 1)] for k in kind]
        # a sphere whose id differs from env to env
        frames = np.tile(np.array([[0.0, 0.0, 0.75, 1, 0, 0, 0]]), (N, 1))
        param = np.tile(np.array([[0.06, 0, 0, rr.SPHERE + 1]]), (N, 1))
        slot = len(T.env)
        T.add(rr.SPHERE, -1, frames[0], (0.06,), seg=8, env=dict(frame=frames, param=param, bound=np.concatenate([frames[:, :3], param[:, :1]], axis=1)))
        T.env_seg[slot] = 20 + e_idx % 5
        rigid = rcc.body_poses(N, [(0.0, 0.05, 0.3), (-0.25, 0.05, 0.36), (0, 0, -50), (0, 0, -60)], rng)
        cams = [rcc.camera(32, 24, 1.2, pose=rcc.look_at((-1.3, 0.1, 0.9), (0, 0, 0.25), up=(0.1, -0.2, 1.0)), far=5.0)]
    elif name == "terrain":
        meshes["field"] = T.mesh(*heightfield())
        T.add_mesh(-1, (0, 0, 0, 1, 0, 0, 0), meshes["field"], seg=1)
        T.add(rr.SPHERE, 0, rcc.IDENT, (0.15,), seg=2)
        rigid = rcc.body_poses(N, [(0.1, -0.1, 0.25), (0, 0, -50), (0, 0, -60), (0, 0, -70)], rng)
        env_pose = np.stack([rcc.look_at((-1.6, 0.3, 1.1) + rng.uniform(-0.1, 0.1, size=3), (0, 0, 0), up=(0.2, 0.1, 1.0)) for _ in range(N)])
        cams = [rcc.camera(32, 24, 1.0, env_pose=env_pose),
                rcc.camera(17, 5, 1.1, pose=rcc.look_at((0.2, -1.3, 0.9), (0, 0, 0))),
                rcc.camera(1, 1, 0.6, pose=rcc.look_at((0.4, 0.5, 1.5), (0.3, 0.4, 0.0), up=(1, 0, 0)))]
    elif name == "inside":
        verts, tris = box_mesh((1.5, 1.2, 0.8))
        meshes["room"] = T.mesh(verts, tris)
        T.add_mesh(-1, (0, 0, 0.8, *rcc.random_quat(np.random.default_rng(2))), meshes["room"], seg=1)
        T.add(rr.SPHERE, 0, rcc.IDENT, (0.2,), seg=2)
        planes, radius = rcc.hull_planes(rng, scale=0.15)
        T.add(rr.CONVEX, 1, rcc.IDENT, seg=3, bound_r=radius, planes=planes)
        rigid = rcc.body_poses(N, [(0.6, 0.2, 0.7), (0.5, -0.4, 0.9), (0, 0, -50), (0, 0, -60)], rng)
        cams = [rcc.camera(32, 24, 1.4, pose=rcc.look_at((-0.4, 0.1, 0.8), (1.0, 0.0, 0.75), up=(0.1, 0.0, 1.0))),
                rcc.camera(17, 5, 1.2, pose=rcc.look_at((0.1, 0.0, 0.9), (-1.0, 0.5, 0.4)))]
    elif name == "many":
        T.add(rr.PLANE, -1, (0, 0, 0, *rcc.GROUND_Q), seg=1)
        k = 0
        for ix in range(10):
            for iy in range(7):
                T.add(rr.SPHERE, -1, (0.25 * ix - 0.4, 0.25 * iy - 0.75, 0.1 + 0.01 * ((3 * ix + 5 * iy) % 7), 1, 0, 0, 0), (0.06,), seg=2 + k % 50)
                k += 1
        meshes["fan"] = T.mesh(*fan_mesh(n=17, radius=0.3, rise=0.25))
        T.add_mesh(1, rcc.IDENT, meshes["fan"], seg=60)   # shape 71: in the second staged chunk
        rigid = rcc.body_poses(N, [(-1.0, 0.0, 1.0), (0.6, 0.0, 0.45), (0, 0, -50), (0, 0, -60)], rng, jitter=0.05)
        env_pose = np.stack([rcc.look_at((1.0, -1.6, 1.2) + rng.uniform(-0.1, 0.1, size=3), (0.7, 0, 0), up=(0.3, 0.1, 1.0)) for _ in range(N)])
        cams = [rcc.camera(32, 24, 1.3, env_pose=env_pose, far=5.0)]
    else:
        raise KeyError(name)
    return dict(scene=T.arrays(), cameras=cams, rigid=rigid, N=N, meshes=meshes)


@functools.lru_cache(maxsize=None)
def reference(name, N):
    """per camera, per env: (float64 render, ambiguous [H, W]) -- computed once, shared by the tests"""
    c = build(name, N)
    return [[rmr.ambiguous(c["scene"], cam, c["rigid"], N, e)[::-1] for e in range(N)] for cam in c["cameras"]]
