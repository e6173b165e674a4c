"""A numpy restatement of the ray caster's definition (include/mssim_hip_tasks.h, "Ray-cast camera observations"),
written from that definition and not from the kernel: rays are built in the env frame with rotation matrices and
carried into each shape's frame, whole images at a time. `dtype` selects the arithmetic: float64 is the reference,
float32 the same computation in the kernel's precision (their difference is the tolerance the GPU tests allow,
tests/raycast_cases.py MEASURED).

A scene is the dict of `maniskill_amd.model.compile.raycast_scene` (host arrays), a camera the dict that
`MssimSystem.raycast_create` takes (with `env_pose` as a numpy [N, 7] array), `rigid` the [R * N, 13] pose buffer.
"""
import numpy as np

PLANE, BOX, SPHERE, CAPSULE, CYLINDER, CONVEX, NONE, TRIMESH = range(8)
MAX_DEPTH = 32.767  # the int16 millimetre range
AMBIG_SHIFT = 0.01  # pixels
AMBIG_DIST = 1e-4   # metres


def intrinsics_from_fov(width, height, fov):
    f = height / (2.0 * np.tan(fov / 2.0))
    return dict(fx=f, fy=f, cx=width / 2.0, cy=height / 2.0)


def _rot(q, dt):
    q = np.asarray(q, dtype=dt)
    w, x, y, z = q / np.sqrt((q * q).sum(dtype=dt))
    one, two = dt(1), dt(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype=dt)


def _mat(pose7, dt):
    """(R, p) of a pose p, q(wxyz)"""
    pose7 = np.asarray(pose7)
    return _rot(pose7[3:7], dt), np.asarray(pose7[:3], dtype=dt)


def _mul(a, b):
    return a[0] @ b[0], a[0] @ b[1] + a[1]


def _slab(o, d, h, tin, tout):
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (-h - o) / d, (h - o) / d
    lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
    par = d == 0
    out = par & (np.abs(o) > h)
    lo = np.where(par, np.where(out, np.inf, -np.inf), lo)
    hi = np.where(par, np.where(out, -np.inf, np.inf), hi)
    return np.maximum(tin, lo), np.minimum(tout, hi)


def _ball(oc, d, r, dt):
    """interval of the line oc + t d inside |x| <= r (oc: [3] start relative to the centre, d: [..., 3])"""
    a = (d * d).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        tm = -(d * oc).sum(-1) / a
        l = oc + tm[..., None] * d
        h2 = r * r - (l * l).sum(-1)
        half = np.sqrt(np.maximum(h2, 0) / a)
    tin, tout = np.where(h2 < 0, np.inf, tm - half), np.where(h2 < 0, -np.inf, tm + half)
    inside = (oc * oc).sum() <= r * r  # a == 0: a line along a cylinder's axis
    tin = np.where(a == 0, -np.inf if inside else np.inf, tin)
    tout = np.where(a == 0, np.inf if inside else -np.inf, tout)
    return tin.astype(dt), tout.astype(dt)


def _cylinder(o, d, r, h, dt):
    mask = np.array([0, 1, 1], dtype=dt)
    tin, tout = _ball(o * mask, d * mask, r, dt)
    return _slab(o[0], d[..., 0], h, tin, tout)


def shape_entry(type_, param, planes, o, d, dt):
    """entry parameter [H, W] of the rays (o [3], d [H, W, 3]) into the shape, in the shape's frame; inf = missed"""
    inf = np.full(d.shape[:-1], np.inf, dtype=dt)
    if type_ == PLANE:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -o[0] / d[..., 0]
        return np.where(d[..., 0] < 0, t, np.inf).astype(dt)
    if type_ == BOX:
        tin, tout = -inf, inf
        for k in range(3):
            tin, tout = _slab(o[k], d[..., k], param[k], tin, tout)
    elif type_ == SPHERE:
        tin, tout = _ball(o, d, param[0], dt)
    elif type_ == CYLINDER:
        tin, tout = _cylinder(o, d, param[0], param[1], dt)
    elif type_ == CAPSULE:
        tin, tout = _cylinder(o, d, param[0], param[1], dt)
        best = np.where(tin <= tout, tin, np.inf)
        for sx in (-1, 1):
            c = np.array([sx * param[1], 0, 0], dtype=dt)
            bi, bo = _ball(o - c, d, param[0], dt)
            best = np.minimum(best, np.where(bi <= bo, bi, np.inf))
        return best.astype(dt)
    elif type_ == CONVEX:
        tin, tout = -inf, inf
        miss = np.zeros(d.shape[:-1], dtype=bool)
        for n4 in planes:
            n, off = n4[:3].astype(dt), dt(n4[3])
            nd, dist = d @ n, off - (n * o).sum(dtype=dt)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = dist / nd
            tin = np.where(nd < 0, np.maximum(tin, t), tin)
            tout = np.where(nd > 0, np.minimum(tout, t), tout)
            miss |= (nd == 0) & (dist < 0)
        tin = np.where(miss, np.inf, tin)
    else:
        return inf
    return np.where(tin <= tout, tin, np.inf).astype(dt)


def camera_pose(camera, rigid, N, env, dt):
    """(R, p): env frame <- camera, SAPIEN axes (x forward, y left, z up)"""
    local = camera["env_pose"][env] if camera.get("env_pose") is not None else camera["pose"]
    T = _mat(local, dt)
    row = int(camera.get("mount_row", -1))
    if row >= 0:
        T = _mul(_mat(rigid[row * N + env, :7], dt), T)
    return T


def entries(scene, camera, rigid, N, env, dtype=np.float64, du=0.0, dv=0.0):
    """-> (t [S, H, W] entry parameter of every shape, inf = missed or absent; seg [S]; rays' x_cv, y_cv [H, W])"""
    dt = np.dtype(dtype).type
    W, H = int(camera["width"]), int(camera["height"])
    u = (np.arange(W, dtype=dt) + dt(0.5) + dt(du) - dt(camera["cx"])) / dt(camera["fx"])
    v = (np.arange(H, dtype=dt) + dt(0.5) + dt(dv) - dt(camera["cy"])) / dt(camera["fy"])
    xcv, ycv = np.meshgrid(u, v)  # [H, W]
    Rc, pc = camera_pose(camera, rigid, N, env, dt)
    # OpenCV (x right, y down, z forward) -> SAPIEN camera axes: (z, -x, -y); then into the env frame
    d_env = np.stack([np.ones_like(xcv), -xcv, -ycv], axis=-1) @ Rc.T
    S = len(scene["shape_type"])
    n_es = int(scene.get("n_env_shape", 0))
    out = np.full((S, H, W), np.inf, dtype=dt)
    for i in range(S):
        type_, frame, param = int(scene["shape_type"][i]), scene["shape_frame"][i], scene["shape_param"][i][:3]
        slot = int(scene["shape_env_slot"][i]) if n_es else -1
        if slot >= 0:
            frame = scene["env_shape_frame"].reshape(n_es, 7, N)[slot, :, env]
            ep = scene["env_shape_param"].reshape(n_es, 4, N)[slot, :, env]
            if ep[3] > 0:
                type_ = int(ep[3]) - 1
            if type_ != CONVEX:
                param = ep[:3]
        if type_ == NONE:
            continue
        T = _mat(frame, dt)
        row = int(scene["shape_row"][i])
        if row >= 0:
            T = _mul(_mat(rigid[row * N + env, :7], dt), T)
        Rs, ps = T
        o = Rs.T @ (pc - ps)  # the camera's origin in the shape frame
        d = d_env @ Rs        # rows: Rs^T d
        first, count = (int(x) for x in scene["shape_planes"][i])
        out[i] = shape_entry(type_, np.asarray(param, dtype=dt), np.asarray(scene["planes"])[first : first + count], o.astype(dt), d.astype(dt), dt)
    return out, np.asarray(scene["shape_seg"]).astype(np.int64), xcv, ycv


def render(scene, camera, rigid, N, env, dtype=np.float64, du=0.0, dv=0.0):
    """one env's image: dict(t [H, W] z-depth, 0 = nothing; seg [H, W]; pos_mm [H, W, 3] int64 (OpenGL frame, truncated);
    hit [H, W] bool; all_t [S, H, W]; shape_seg [S])"""
    dt = np.dtype(dtype).type
    all_t, seg_of, xcv, ycv = entries(scene, camera, rigid, N, env, dtype, du, dv)
    near, tmax = dt(camera["near"]), dt(min(float(camera["far"]), MAX_DEPTH))
    H, W = xcv.shape
    if len(all_t) == 0:
        best, seg, hit = np.zeros((H, W), dtype=dt), np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=bool)
    else:
        valid = np.where((all_t >= near) & (all_t <= tmax), all_t, np.inf)
        k = np.argmin(valid, axis=0)  # (the first shape on an exact tie)
        best = np.take_along_axis(valid, k[None], axis=0)[0]
        hit = np.isfinite(best)
        seg = np.where(hit, seg_of[k], 0)
        best = np.where(hit, best, 0).astype(dt)
    pos = np.stack([xcv * best, -(ycv * best), -best], axis=-1)
    pos_mm = np.trunc(np.clip(dt(1000) * pos, -32768, 32767)).astype(np.int64)
    return dict(t=best, seg=seg, hit=hit, pos_mm=pos_mm, all_t=all_t, shape_seg=seg_of)


def ambiguous(scene, camera, rigid, N, env):
    """[H, W] bool (float64 throughout): the id changes under a shift of the ray by +-AMBIG_SHIFT pixel in u or v, or a
    second body's surface lies within AMBIG_DIST of the hit, or the hit lies within AMBIG_DIST of near or of the far limit"""
    R = render(scene, camera, rigid, N, env)
    amb = np.zeros(R["seg"].shape, dtype=bool)
    for du, dv in ((AMBIG_SHIFT, 0), (-AMBIG_SHIFT, 0), (0, AMBIG_SHIFT), (0, -AMBIG_SHIFT)):
        amb |= render(scene, camera, rigid, N, env, du=du, dv=dv)["seg"] != R["seg"]
    near, tmax = float(camera["near"]), min(float(camera["far"]), MAX_DEPTH)
    t = np.where(R["hit"], R["t"], np.nan)
    with np.errstate(invalid="ignore"):
        amb |= (np.abs(t - near) < AMBIG_DIST) | (np.abs(t - tmax) < AMBIG_DIST)
        other = R["shape_seg"][:, None, None] != R["seg"][None]
        amb |= (other & (np.abs(R["all_t"] - t[None]) < AMBIG_DIST)).any(axis=0)
    return amb, R


def project(camera, rigid, N, env, point):
    """(u, v, z): pixel coordinates (continuous; pixel (c, r) covers [c, c+1) x [r, r+1)) and z-depth of an env-frame point"""
    Rc, pc = camera_pose(camera, rigid, N, env, np.float64)
    s = Rc.T @ (np.asarray(point, dtype=np.float64) - pc)  # SAPIEN camera axes
    x, y, z = -s[1], -s[2], s[0]
    return camera["fx"] * x / z + camera["cx"], camera["fy"] * y / z + camera["cy"], z
