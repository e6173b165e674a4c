"""The ray caster's definition for triangle meshes, per-env hulls and per-env ids (include/mssim_hip_tasks.h, "Ray-cast
camera observations"), on top of tests/raycast_reference.py, written from the definition and not from the kernel: a mesh's
hit is found by BRUTE FORCE over all its triangles -- the BVH is never read --, two-sided, as the point where the ray
meets the triangle's plane when that point's barycentric coordinates are all >= -slack; it is combined with the other
shapes' entries by the same minimum and tie rule. `dtype` selects the arithmetic as there (float64: the reference;
float32: the same computation in the kernel's precision, whose distance from the float64 run is
tests/raycast_mesh_cases.py MEASURED_MESH).

A scene is the dict of `maniskill_amd.model.compile.raycast_scene(..., meshes=True)`: the keys of raycast_reference plus
`tri_soup` [T, 12], `tri_bvh` (unused here), and optionally `env_shape_planes` [slots * 2, N] and `env_shape_seg` [slots, N].
"""
import numpy as np

from tests import raycast_reference as rr

TRIMESH = rr.TRIMESH
# barycentric slack of the inclusive edge tests: a ray through a shared edge must not fall between two roundings
SLACK = {np.float64: 1e-9, np.float32: 1e-5}
COPLANAR_TOL = 1e-6  # unit normals and plane offsets (metres) within this: the same plane


def resolved(scene, N, env):
    """the scene as env `env` has it, in the keys raycast_reference reads: the env's own plane ranges and ids in place of
    the shared ones"""
    n_es = int(scene.get("n_env_shape", 0))
    planes2, seg = np.array(scene["shape_planes"], dtype=np.int64).reshape(-1, 2), np.array(scene["shape_seg"], dtype=np.int64)
    if n_es:
        slots = np.asarray(scene["shape_env_slot"])
        ep = np.asarray(scene["env_shape_param"]).reshape(n_es, 4, N)
        for i in np.nonzero(slots >= 0)[0]:
            s = int(slots[i])
            t1 = int(ep[s, 3, env])
            type_ = t1 - 1 if t1 > 0 else int(scene["shape_type"][i])
            if scene.get("env_shape_planes") is not None and type_ == rr.CONVEX:
                planes2[i] = np.asarray(scene["env_shape_planes"]).reshape(n_es, 2, N)[s, :, env]
            if scene.get("env_shape_seg") is not None:
                seg[i] = int(np.asarray(scene["env_shape_seg"]).reshape(n_es, N)[s, env])
    out = dict(scene)
    out["shape_planes"], out["shape_seg"] = planes2, seg
    return out


def mesh_of(scene, i, N, env):
    """(first triangle, count) of shape i in env `env`, or None where it is no mesh there"""
    type_, param = int(scene["shape_type"][i]), scene["shape_param"][i]
    n_es = int(scene.get("n_env_shape", 0))
    slot = int(scene["shape_env_slot"][i]) if n_es else -1
    if slot >= 0:
        ep = np.asarray(scene["env_shape_param"]).reshape(n_es, 4, N)[slot, :, env]
        if ep[3] > 0:
            type_, param = int(ep[3]) - 1, ep
    return (int(param[0]), int(param[1])) if type_ == TRIMESH else None


def shape_pose(scene, i, rigid, N, env, dt):
    """(R, p): env frame <- shape frame of shape i in env `env`"""
    frame = scene["shape_frame"][i]
    n_es = int(scene.get("n_env_shape", 0))
    slot = int(scene["shape_env_slot"][i]) if n_es else -1
    if slot >= 0:
        frame = np.asarray(scene["env_shape_frame"]).reshape(n_es, 7, N)[slot, :, env]
    T = rr._mat(frame, dt)
    row = int(scene["shape_row"][i])
    if row >= 0:
        T = rr._mul(rr._mat(rigid[row * N + env, :7], dt), T)
    return T


def triangles_hit(soup, o, d, dt):
    """rays (o [3], d [..., 3]) against triangles soup [T, 12], all in one frame, arithmetic in `dt`:
    -> t [..., T], inf where the ray misses the triangle (or lies in its plane)"""
    soup = np.asarray(soup).astype(dt)
    A, B, C = (soup[:, :3] + soup[:, 3 + 3 * k : 6 + 3 * k] for k in range(3))  # corners [T, 3]
    n = np.cross(B - A, C - A).astype(dt)
    nn = (n * n).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        den = d @ n.T                                    # [..., T]
        t = (((A - o) * n).sum(-1) / den).astype(dt)
        P = o + t[..., None] * d[..., None, :]           # [..., T, 3]
        w = [(np.cross(Q - S, P - S) * n).sum(-1) / nn for S, Q in ((A, B), (B, C), (C, A))]
        inside = np.minimum(np.minimum(w[0], w[1]), w[2]) >= -dt(SLACK[dt])
    return np.where((den != 0) & inside & np.isfinite(t), t, np.inf).astype(dt)


def plane_classes(soup):
    """[T] int: triangles in one plane (either way round) share a class"""
    soup = np.asarray(soup, dtype=np.float64)
    A = soup[:, :3] + soup[:, 3:6]
    n = np.cross(soup[:, 6:9] - soup[:, 3:6], soup[:, 9:12] - soup[:, 3:6])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
    flip = np.where(n[:, 0] != 0, n[:, 0], np.where(n[:, 1] != 0, n[:, 1], n[:, 2])) < 0
    n[flip] *= -1
    key = np.round(np.concatenate([n, (A * n).sum(-1, keepdims=True)], axis=1) / COPLANAR_TOL).astype(np.int64)
    return np.unique(key, axis=0, return_inverse=True)[1].reshape(-1)


def entries(scene, camera, rigid, N, env, dtype=np.float64, du=0.0, dv=0.0):
    """-> (t [S, H, W] of every shape, meshes included; seg [S] of this env; x_cv, y_cv [H, W]; tri [S, H, W]: the global
    index of the mesh triangle hit first, -1 for other shapes and misses)"""
    dt = np.dtype(dtype).type
    S = resolved(scene, N, env)
    out, seg_of, xcv, ycv = rr.entries(S, camera, rigid, N, env, dtype, du, dv)
    tri = np.full(out.shape, -1, dtype=np.int64)
    Rc, pc = rr.camera_pose(camera, rigid, N, env, dt)
    d_env = np.stack([np.ones_like(xcv), -xcv, -ycv], axis=-1) @ Rc.T
    near, tmax = dt(camera["near"]), dt(min(float(camera["far"]), rr.MAX_DEPTH))
    for i in range(len(out)):
        m = mesh_of(scene, i, N, env)
        if m is None or m[1] == 0:
            continue
        Rs, ps = shape_pose(scene, i, rigid, N, env, dt)
        o, d = (Rs.T @ (pc - ps)).astype(dt), (d_env @ Rs).astype(dt)
        t = triangles_hit(np.asarray(scene["tri_soup"])[m[0] : m[0] + m[1]], o, d, dt)   # [H, W, T]
        t = np.where((t >= near) & (t <= tmax), t, np.inf)  # (the mesh's hit is its smallest t WITHIN the range)
        k = np.argmin(t, axis=-1)
        out[i] = np.take_along_axis(t, k[..., None], axis=-1)[..., 0]
        tri[i] = np.where(np.isfinite(out[i]), m[0] + k, -1)
    return out, seg_of, xcv, ycv, tri


def render(scene, camera, rigid, N, env, dtype=np.float64, du=0.0, dv=0.0):
    """raycast_reference.render with meshes; additionally `shape` [H, W] (index of the shape hit, -1) and `tri` [H, W]"""
    dt = np.dtype(dtype).type
    all_t, seg_of, xcv, ycv, tri = entries(scene, camera, rigid, N, env, dtype, du, dv)
    near, tmax = dt(camera["near"]), dt(min(float(camera["far"]), rr.MAX_DEPTH))
    H, W = xcv.shape
    if len(all_t) == 0:
        best, seg, hit = np.zeros((H, W), dtype=dt), np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=bool)
        shape = tri_hit = np.full((H, W), -1, dtype=np.int64)
    else:
        valid = np.where((all_t >= near) & (all_t <= tmax), all_t, np.inf)
        k = np.argmin(valid, axis=0)  # (the first shape on an exact tie)
        best = np.take_along_axis(valid, k[None], axis=0)[0]
        hit = np.isfinite(best)
        seg = np.where(hit, seg_of[k], 0)
        shape = np.where(hit, k, -1)
        tri_hit = np.where(hit, np.take_along_axis(tri, k[None], axis=0)[0], -1)
        best = np.where(hit, best, 0).astype(dt)
    pos = np.stack([xcv * best, -(ycv * best), -best], axis=-1)
    pos_mm = np.trunc(np.clip(dt(1000) * pos, -32768, 32767)).astype(np.int64)
    return dict(t=best, seg=seg, hit=hit, pos_mm=pos_mm, all_t=all_t, shape_seg=seg_of, shape=shape, tri=tri_hit)


def ambiguous(scene, camera, rigid, N, env):
    """[H, W] bool (float64 throughout): raycast_reference.ambiguous's rules -- the id changes under a shift of the ray by
    +-AMBIG_SHIFT pixel, a second body's surface within AMBIG_DIST of the hit, the hit within AMBIG_DIST of near or the far
    limit -- plus: the shift moves the hit to a mesh triangle that is not coplanar with the current one (or to another
    shape's triangle), or turns a hit into a miss or a miss into a hit"""
    R = render(scene, camera, rigid, N, env)
    cls = plane_classes(scene["tri_soup"]) if scene.get("tri_soup") is not None and len(scene["tri_soup"]) else np.zeros(0, dtype=np.int64)

    def plane_of(r):  # -1 off the meshes
        return np.where(r["tri"] >= 0, cls[np.maximum(r["tri"], 0)] if len(cls) else -1, -1)

    amb = np.zeros(R["seg"].shape, dtype=bool)
    for du, dv in ((rr.AMBIG_SHIFT, 0), (-rr.AMBIG_SHIFT, 0), (0, rr.AMBIG_SHIFT), (0, -rr.AMBIG_SHIFT)):
        r = render(scene, camera, rigid, N, env, du=du, dv=dv)
        amb |= (r["seg"] != R["seg"]) | (r["hit"] != R["hit"])
        on_mesh = (r["tri"] >= 0) | (R["tri"] >= 0)
        amb |= on_mesh & ((r["shape"] != R["shape"]) | (plane_of(r) != plane_of(R)))
    near, tmax = float(camera["near"]), min(float(camera["far"]), rr.MAX_DEPTH)
    t = np.where(R["hit"], R["t"], np.nan)
    with np.errstate(invalid="ignore"):
        amb |= (np.abs(t - near) < rr.AMBIG_DIST) | (np.abs(t - tmax) < rr.AMBIG_DIST)
        other = R["shape_seg"][:, None, None] != R["seg"][None]
        amb |= (other & (np.abs(R["all_t"] - t[None]) < rr.AMBIG_DIST)).any(axis=0)
    return amb, R
