"""Constructed scenes for the ray caster, shared by tests/test_raycast.py (CPU: the reference alone) and
tests/test_gpu_raycast.py (the kernel against the reference).

Three scenes on four body rows put in front of the reference: every shape type, a per-env override (a sphere whose
radius differs from env to env, absent -- MSSIM_SHAPE_NONE -- in every third env), an occlusion (a box in front of a
sphere), a near-plane cut (a ball that the near plane cuts: its front is culled and what lies behind shows), a wall beyond
32.767 m ("nothing") next to one at 30 m, a camera mounted on a moving body, cameras of different sizes in one scene
(32 x 24, 17 x 5, 1 x 1), a per-env camera pose, and a scene of 72 shapes, more than one staged chunk of 64
(MSSIM_RAYCAST_CHUNK). Body poses are drawn per env from a seeded generator, so N = 1, 3 and 67 render different images.

CONFIGS lists the (scene, N) pairs both test files use. MEASURED is the largest difference between the float32 and the
float64 run of the reference over the unambiguous pixels (tests/raycast_reference.py `ambiguous`) of every image of
CONFIGS where both runs hit something, measured on the CPU by test_raycast.py::test_float32_reference_within_measured;
the GPU test allows the kernel's float depth 4 x that, the project's convention for its float32 kernels. The int16
components may differ by one count (truncation falls either side of a boundary).
"""
import functools

import numpy as np

from tests import raycast_reference as rr

# largest |t_f32 - t_f64| in metres (see above), on a pixel of the ground plane some 30 m away at a glancing angle, where a
# float32 rounding of the ray's direction moves the hit by t^2 / height times as much
MEASURED = 1.6e-4
MAX_AMBIGUOUS_SHARE = 0.05
N_ROWS = 4

CONFIGS = (("types", 1), ("types", 3), ("types", 67), ("near_far", 1), ("near_far", 3), ("many", 3))


def look_at(eye, target, up=(0, 0, 1)):
    """pose p, q(wxyz) of a SAPIEN-axes camera (x forward, y left, z up) at `eye` looking at `target`"""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    f = (target - eye) / np.linalg.norm(target - eye)
    l = np.cross(up, f)
    l /= np.linalg.norm(l)
    u = np.cross(f, l)
    return np.concatenate([eye, mat_to_quat(np.stack([f, l, u], axis=1))])


def mat_to_quat(R):
    w = np.sqrt(max(1.0 + R[0, 0] + R[1, 1] + R[2, 2], 1e-30)) / 2
    if w > 1e-3:
        return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    x = np.sqrt(max(1.0 + R[0, 0] - R[1, 1] - R[2, 2], 1e-30)) / 2
    if x > 1e-3:
        return np.array([(R[2, 1] - R[1, 2]) / (4 * x), x, (R[0, 1] + R[1, 0]) / (4 * x), (R[0, 2] + R[2, 0]) / (4 * x)])
    y = np.sqrt(max(1.0 - R[0, 0] + R[1, 1] - R[2, 2], 1e-30)) / 2
    if y > 1e-3:
        return np.array([(R[0, 2] - R[2, 0]) / (4 * y), (R[0, 1] + R[1, 0]) / (4 * y), y, (R[1, 2] + R[2, 1]) / (4 * y)])
    z = np.sqrt(max(1.0 - R[0, 0] - R[1, 1] + R[2, 2], 1e-30)) / 2
    return np.array([(R[1, 0] - R[0, 1]) / (4 * z), (R[0, 2] + R[2, 0]) / (4 * z), (R[1, 2] + R[2, 1]) / (4 * z), z])


GROUND_Q = (np.sqrt(0.5), 0.0, -np.sqrt(0.5), 0.0)  # the plane's +x normal turned to +z: the solid is z <= 0
IDENT = (0, 0, 0, 1, 0, 0, 0)


class SceneTables:
    """accumulates the arrays of a mssim_raycast_scene"""

    def __init__(self, N):
        self.N, self.rows = N, dict(shape_type=[], shape_row=[], shape_frame=[], shape_param=[], shape_bound=[], shape_seg=[], shape_planes=[], shape_env_slot=[])
        self.planes, self.env = [], []

    def add(self, type_, row, frame, param=(0, 0, 0), seg=0, bound_r=None, planes=None, env=None):
        r = self.rows
        param = list(param) + [0.0] * (4 - len(param))
        if bound_r is None:
            bound_r = {rr.PLANE: -1.0, rr.BOX: float(np.linalg.norm(param[:3])), rr.SPHERE: param[0], rr.CAPSULE: param[0] + param[1],
                       rr.CYLINDER: float(np.hypot(param[0], param[1]))}[type_]
        first = len(self.planes)
        if planes is not None:
            self.planes.extend(np.asarray(planes).tolist())
        r["shape_type"].append(type_); r["shape_row"].append(row); r["shape_frame"].append(list(frame)); r["shape_param"].append(param)
        r["shape_bound"].append([*frame[:3], bound_r]); r["shape_seg"].append(seg); r["shape_planes"].append([first, 0 if planes is None else len(planes)])
        r["shape_env_slot"].append(-1 if env is None else len(self.env))
        if env is not None:  # dict(frame [N, 7], param [N, 4] with [3] = type + 1, bound [N, 4])
            self.env.append(env)

    def arrays(self):
        r, ne = self.rows, len(self.env)
        out = dict(
            shape_type=np.asarray(r["shape_type"], dtype=np.int32), shape_row=np.asarray(r["shape_row"], dtype=np.int32),
            shape_frame=np.asarray(r["shape_frame"], dtype=np.float32).reshape(-1, 7), shape_param=np.asarray(r["shape_param"], dtype=np.float32).reshape(-1, 4),
            shape_bound=np.asarray(r["shape_bound"], dtype=np.float32).reshape(-1, 4), shape_seg=np.asarray(r["shape_seg"], dtype=np.int16),
            shape_planes=np.asarray(r["shape_planes"], dtype=np.int32).reshape(-1, 2), planes=np.asarray(self.planes, dtype=np.float32).reshape(-1, 4),
            n_env_shape=ne, shape_env_slot=np.asarray(r["shape_env_slot"], dtype=np.int32),
        )
        for key, width in (("frame", 7), ("param", 4), ("bound", 4)):  # [items][N], env fastest
            a = np.concatenate([np.asarray(e[key], dtype=np.float32).T for e in self.env]) if ne else np.zeros((0, self.N), dtype=np.float32)
            out["env_shape_" + key] = np.ascontiguousarray(a.reshape(width * ne, self.N))
        return out


def random_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def body_poses(N, centres, rng, jitter=0.03):
    """[N_ROWS * N, 13] float32: body row b of env e at centres[b] + jitter, a random orientation"""
    rigid = np.zeros((N_ROWS * N, 13), dtype=np.float32)
    rigid[:, 3] = 1.0
    for b, c in enumerate(centres):
        for e in range(N):
            rigid[b * N + e, :3] = np.asarray(c) + rng.uniform(-jitter, jitter, size=3)
            rigid[b * N + e, 3:7] = random_quat(rng)
    return rigid


def camera(width, height, fov, pose=None, env_pose=None, mount_row=-1, near=0.01, far=100.0):
    c = dict(width=width, height=height, near=near, far=far, mount_row=mount_row, **rr.intrinsics_from_fov(width, height, fov))
    if env_pose is not None:
        c["env_pose"] = np.ascontiguousarray(env_pose, dtype=np.float32)
    else:
        c["pose"] = np.asarray(pose, dtype=np.float32)
    return c


def hull_planes(rng, n_points=14, scale=0.12):
    from maniskill_amd.model.mesh import hull_face_planes

    pts = rng.normal(size=(n_points, 3)) * scale
    return hull_face_planes(pts - pts.mean(axis=0)), float(np.linalg.norm(pts - pts.mean(axis=0), axis=1).max())


@functools.lru_cache(maxsize=None)
def build(name, N):
    """-> dict(scene arrays, cameras [dict], rigid [N_ROWS * N, 13] float32, N)"""
    rng = np.random.default_rng({"types": 11, "near_far": 12, "many": 13}[name] * 1000 + N)
    T = SceneTables(N)
    if name == "types":
        T.add(rr.PLANE, -1, (0, 0, 0, *GROUND_Q), seg=1)
        T.add(rr.BOX, 0, IDENT, (0.12, 0.08, 0.05), seg=2)
        T.add(rr.SPHERE, 1, (0.02, 0, 0, 1, 0, 0, 0), (0.1,), seg=3)  # partly behind the box, seen from the camera
        T.add(rr.CAPSULE, 2, IDENT, (0.05, 0.12), seg=4)
        T.add(rr.CYLINDER, 3, IDENT, (0.07, 0.1), seg=5)
        planes, radius = hull_planes(rng)
        T.add(rr.CONVEX, -1, (0.1, -0.55, 0.2, *random_quat(rng)), seg=6, bound_r=radius, planes=planes)
        # a sphere whose radius differs from env to env and that every third env lacks; its shared entry is a box
        radii = 0.05 + 0.04 * rng.uniform(size=N)
        types = np.where(np.arange(N) % 3 == 2, rr.NONE + 1, rr.SPHERE + 1)
        frames = np.tile(np.array([[-0.3, 0.5, 0.15, 1, 0, 0, 0]], dtype=np.float64), (N, 1))
        T.add(rr.BOX, -1, frames[0], (0.05, 0.05, 0.05), seg=7, env=dict(
            frame=frames, param=np.stack([radii, 0 * radii, 0 * radii, types], axis=1), bound=np.concatenate([frames[:, :3], radii[:, None]], axis=1)))
        rigid = body_poses(N, [(-0.35, 0.05, 0.3), (-0.05, 0.0, 0.32), (0.1, 0.4, 0.25), (0.0, -0.2, 0.6)], rng)
        cams = [camera(32, 24, 1.2, pose=look_at((-1.3, 0.1, 0.9), (0, 0, 0.25), up=(0.1, -0.2, 1.0)))]
    elif name == "near_far":
        T.add(rr.PLANE, -1, (0, 0, 0, *GROUND_Q), seg=1)
        T.add(rr.SPHERE, 0, IDENT, (0.5,), seg=2)             # cut by the near plane: only a ring of it, entered behind `near`, shows
        T.add(rr.BOX, -1, (30.5, 6, 5, 1, 0, 0, 0), (0.5, 6, 5), seg=3)    # a wall whose face is 30 m away
        T.add(rr.BOX, -1, (40.5, -6, 5, 1, 0, 0, 0), (0.5, 6, 5), seg=4)   # and one at 40 m: beyond the int16 range
        T.add(rr.CYLINDER, 1, IDENT, (0.3, 0.4), seg=5)
        rigid = body_poses(N, [(1.0, 0.0, 1.0), (3.0, 1.2, 0.9), (0, 0, -50), (0, 0, -60)], rng, jitter=0.02)
        cams = [camera(32, 24, 1.0, pose=(0, 0, 1.0, 1, 0, 0, 0), near=0.6, far=100.0)]
    elif name == "many":
        T.add(rr.PLANE, -1, (0, 0, 0, *GROUND_Q), seg=1)
        k = 0
        for ix in range(10):
            for iy in range(7):  # 70 balls on the ground: with the plane 71 shapes, two staged chunks
                T.add(rr.SPHERE, -1, (0.25 * ix - 0.4, 0.25 * iy - 0.75, 0.1 + 0.01 * ((3 * ix + 5 * iy) % 7), 1, 0, 0, 0), (0.06,), seg=2 + k % 50)
                k += 1
        T.add(rr.BOX, 1, IDENT, (0.1, 0.1, 0.1), seg=60)
        rigid = body_poses(N, [(-1.0, 0.0, 1.0), (0.5, 0.0, 0.5), (0, 0, -50), (0, 0, -60)], rng, jitter=0.05)
        for e in range(N):  # body 0 carries camera 0: it looks down at the balls, a little differently in every env
            rigid[e, 3:7] = look_at(rigid[e, :3], (0.6, 0.0, 0.0) + rng.uniform(-0.1, 0.1, size=3))[3:]
        env_pose = np.stack([look_at((1.0, -1.6, 1.2) + rng.uniform(-0.1, 0.1, size=3), (0.7, 0, 0), up=(0.3, 0.1, 1.0)) for _ in range(N)])  # (rolled: the horizon crosses rows)
        cams = [camera(17, 5, 1.1, pose=(0.05, 0, 0.02, 1, 0, 0, 0), mount_row=0),
                camera(32, 24, 1.3, env_pose=env_pose),
                camera(1, 1, 0.6, pose=look_at((2.5, 0.4, 1.5), (0.5, 0.0, 0.4)))]
    else:
        raise KeyError(name)
    return dict(scene=T.arrays(), cameras=cams, rigid=rigid, N=N)


@functools.lru_cache(maxsize=None)
def reference(name, N):
    """per camera, per env: (float64 render, ambiguous [H, W]) -- computed once, shared by the tests"""
    c = build(name, N)
    out = []
    for cam in c["cameras"]:
        per_env = []
        for e in range(N):
            amb, R = rr.ambiguous(c["scene"], cam, c["rigid"], N, e)
            per_env.append((R, amb))
        out.append(per_env)
    return out
