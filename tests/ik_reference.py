"""The iterative-IK block of the native action map (include/mssim_hip_tasks.h `set_ee_ik_map`, `ee_ik_solve`) restated
in float64 numpy, one env at a time. No torch, nothing imported from the package: the only things shared with the code
under test are the documented rules (and tests/action_reference.py's FK of the chain from the model's constant tables).

    q = q0[path]
    repeat at most max_iters (60):
      (pe, qe, J) = FK + geometric Jacobian of the link over the dofs on its path, in the ROOT frame
      err = tp - pe ; rows == 6: append the rotation vector of tq * conj(qe)
            (sign-normalised to w >= 0, angle = 2 atan2(|v|, w), v / max(|v|, 1e-9) * angle)
      if max|err| < tolerance (1e-5): stop                       <- this env only
      step = J^T (J J^T + damping I)^-1 err                      (damping 1e-3)
      step *= max_step / max(max|step|, max_step)                (max_step 0.3)
      q = min(max(q + step, lower), upper)                       (a NaN stays a NaN)

The iteration count is the number of steps taken (0: q0 already reaches the target; max_iters: the cap ended the loop).

Map form: the block's columns are clipped and scaled as tests/action_reference.ee_command does, then
    mode 0: p1 = lin,      q1 = euler_xyz(rot)        (identity with 3 rows)
    mode 1: p1 = p0 + lin, q1 = euler_xyz(rot) * q0   (q0 with 3 rows);   no renormalisation
with euler_xyz(a) the quaternion of Rx(a0) Ry(a1) Rz(a2); its sign is not pinned: compare rotations."""
import numpy as np

from tests import action_reference as ar

DEFAULTS = dict(max_iters=60, damping=1e-3, max_step=0.3, tolerance=1e-5)
EPS32 = 2.0 ** -23


def pose_error(A, link, path, q_path, tp, tq, rows):
    """-> (err [rows], J [rows, len(path)]) of one env"""
    n = len(A["dof_type"])
    q = np.zeros((1, n))
    q[0, path] = q_path
    pe, qe, J = ar.link_fk_jacobian(A, q, link)
    err = tp - pe[0]
    if rows == 6:
        d = ar._qmul(tq, qe[0] * np.array([1.0, -1.0, -1.0, -1.0]))
        if d[0] < 0:
            d = -d
        nv = np.linalg.norm(d[1:])
        err = np.concatenate([err, d[1:] / max(nv, 1e-9) * (2.0 * np.arctan2(nv, d[0]))])
    return err, J[0][:rows][:, path]


def solve_env(A, link, q0_path, tp, tq, rows, limits, max_iters=60, damping=1e-3, max_step=0.3, tolerance=1e-5):
    """one env: -> (q [len(path)], iterations, max|err| at the returned q, largest max|step| before the cap)"""
    path = ar.path_dofs(A, link)
    lo, hi = limits[path, 0], limits[path, 1]
    q, it, raw = np.array(q0_path, dtype=np.float64), 0, 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            err, J = pose_error(A, link, path, q, tp, tq, rows)
            if np.abs(err).max() < tolerance or it >= max_iters:  # (NaN < tolerance is False)
                break
            if np.isnan(err).any() or np.isnan(J).any():
                q = np.full_like(q, np.nan)  # what the arithmetic below gives: every entry of the solution is NaN
                it = max_iters
                err = np.full_like(err, np.nan)
                break
            step = J.T @ np.linalg.solve(J @ J.T + damping * np.eye(rows), err)
            m = np.abs(step).max()
            raw = max(raw, m)
            step = step * (max_step / max(m, max_step))
            q = np.minimum(np.maximum(q + step, lo), hi)
            it += 1
    return q, it, float(np.abs(err).max()), raw


def pose_error_batch(A, link, path, q_path, T, rows):
    """pose_error for many envs at once: the same arithmetic per env -> (err [M, rows], J [M, rows, len(path)])"""
    q = np.zeros((len(q_path), len(A["dof_type"])))
    q[:, path] = q_path
    pe, qe, J = ar.link_fk_jacobian(A, q, link)
    err = T[:, :3] - pe
    if rows == 6:
        d = ar._qmul(T[:, 3:], qe * np.array([1.0, -1.0, -1.0, -1.0]))
        d = np.where(d[:, :1] < 0, -d, d)
        nv = np.linalg.norm(d[:, 1:], axis=1, keepdims=True)
        err = np.concatenate([err, d[:, 1:] / np.maximum(nv, 1e-9) * (2.0 * np.arctan2(nv, d[:, :1]))], 1)
    return err, J[:, :rows][:, :, path]


def solve(A, link, q0, target_pose, rows, limits=None, **settings):
    """q0 [N, n_dof], target_pose [N, 7] (p, q wxyz; root frame) -> dict q [N, n_dof] f64 (dofs off the path copied),
    iters [N], err [N] (max|err| at the returned q), path (list), raw_step [N] (largest max|step| before the cap).
    `solve_env` for every env, evaluated for all envs that are still iterating at once: every env leaves at its own
    convergence and its arithmetic never sees another env (tests/test_ik_reference.py holds the two together)."""
    q0, T = np.asarray(q0, dtype=np.float64), np.asarray(target_pose, dtype=np.float64)
    limits = np.asarray(A["dof_limit"] if limits is None else limits, dtype=np.float64)
    path = ar.path_dofs(A, link)
    lo, hi = limits[path, 0], limits[path, 1]
    s = dict(DEFAULTS, **settings)
    N = len(q0)
    q, iters, errs, raw = q0[:, path].copy(), np.zeros(N, dtype=np.int64), np.zeros(N), np.zeros(N)
    active = np.ones(N, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for it in range(s["max_iters"] + 1):
            idx = np.flatnonzero(active)
            if idx.size == 0:
                break
            err, J = pose_error_batch(A, link, path, q[idx], T[idx], rows)
            m = np.abs(err).max(1)  # (NaN if any entry is)
            errs[idx] = m
            nan = np.isnan(m) & (it < s["max_iters"])  # every entry of the solution is NaN from here on
            q[idx[nan]], iters[idx[nan]] = np.nan, s["max_iters"]
            stop = (m < s["tolerance"]) | (it >= s["max_iters"]) | nan
            active[idx[stop]] = False
            idx, err, J = idx[~stop], err[~stop], J[~stop]
            if idx.size == 0:
                continue
            G = J @ J.transpose(0, 2, 1) + s["damping"] * np.eye(rows)
            step = (J.transpose(0, 2, 1) @ np.linalg.solve(G, err[:, :, None]))[:, :, 0]
            big = np.abs(step).max(1)
            raw[idx] = np.maximum(raw[idx], big)
            step = step * (s["max_step"] / np.maximum(big, s["max_step"]))[:, None]
            q[idx] = np.minimum(np.maximum(q[idx] + step, lo), hi)
            iters[idx] += 1
    out = q0.copy()
    out[:, path] = q
    return dict(q=out, iters=iters, err=errs, path=path, raw_step=raw)


def euler_xyz_quat(a):
    """quaternion (wxyz) of Rx(a0) Ry(a1) Rz(a2), a [N, 3]"""
    h = 0.5 * np.asarray(a, dtype=np.float64)
    z, o = np.zeros(len(h)), np.cos(h)
    s = np.sin(h)
    qx = np.stack([o[:, 0], s[:, 0], z, z], -1)
    qy = np.stack([o[:, 1], z, s[:, 1], z], -1)
    qz = np.stack([o[:, 2], z, z, s[:, 2]], -1)
    return ar._qmul(ar._qmul(qx, qy), qz)


def compose(ik, prev_pose, action):
    """ik = (link, column0, rows, mode, low, high, rot_scale, flags); prev_pose [N, 7], action [N, adim] -> the new
    target pose [N, 7] f64"""
    link, c0, rows, mode, low, high, rot_scale, flags = ik
    action, prev = np.asarray(action, dtype=np.float64), np.asarray(prev_pose, dtype=np.float64)
    f = lambda x: float(np.float32(x))
    cmd = ar.ee_command((link, c0, rows, f(low), f(high), f(rot_scale), flags), action)
    N = len(action)
    ident = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (N, 1))
    if mode == 0:
        p, q = cmd[:, :3], (euler_xyz_quat(cmd[:, 3:6]) if rows == 6 else ident)
    else:
        p, q = prev[:, :3] + cmd[:, :3], (ar._qmul(euler_xyz_quat(cmd[:, 3:6]), prev[:, 3:]) if rows == 6 else prev[:, 3:])
    return np.concatenate([p, q], 1)


def apply(ik, A, qpos, prev_pose, action, **settings):
    """the map form: -> dict pose [N, 7] (new target pose), q [N, n_dof] (joint targets on the path, qpos elsewhere),
    iters, err, path"""
    pose = compose(ik, prev_pose, action)
    out = solve(A, int(ik[0]), qpos, pose, int(ik[2]), **settings)
    out["pose"] = pose
    return out


def rotation_distance(qa, qb):
    """1 - |<qa, qb>| of unit-normalised quaternions, [N]"""
    qa, qb = ar._unit(np.asarray(qa, np.float64)), ar._unit(np.asarray(qb, np.float64))
    return 1.0 - np.abs((qa * qb).sum(-1))
