"""The two end-effector blocks of the native action map with HELD joints (include/mssim.h `set_action_map`, bit 64),
restated in float64 numpy on top of tests/ik_reference.py and tests/action_reference.py. No torch, nothing imported
from the package.

For one end-effector controller the active joints on the path root -> link are either SOLVED (the controller's own,
flagged 4) or HELD (another controller's, flagged 64). Held joints take part in the forward kinematics at their current
positions, contribute no Jacobian column and receive no target from the block:

  delta step   target[solved] = qpos[solved] + Js^T (Js Js^T + 1e-9 I)^-1 a,   Js = the solved joints' columns
  iterative    the loop of tests/ik_reference.py with J = Js; step, cap and limits act on the solved joints alone; the
               held positions are those of q0 throughout

With no held joint every function here performs the arithmetic of the module it is built on, operation for operation
(tests/test_held_ik_reference.py holds them together bit for bit)."""
import numpy as np

from tests import action_reference as ar
from tests import ik_reference as ik


def split_path(A, link, held):
    """-> (path, positions of the solved joints in the path, solved dofs)"""
    path = ar.path_dofs(A, link)
    assert set(held) <= set(path), "a held joint must be on the link's path"
    sel = [k for k, j in enumerate(path) if j not in held]
    return path, sel, [path[k] for k in sel]


def compose_prefix(A, dofs, q):
    """the joints `dofs` (a serial chain from the root) at positions q [len(dofs)] as one transform -> (p [3], quat [4]),
    with the arithmetic of action_reference.link_fk_jacobian"""
    p, r = np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])
    for j, qj in zip(dofs, q):
        frame = np.asarray(A["dof_frame"][j], dtype=np.float64)
        axis = np.asarray(A["dof_axis"][j], dtype=np.float64)
        jp, jq = p + ar._qrot(r, frame[:3]), ar._qmul(r, ar._unit(frame[3:]))
        if int(A["dof_type"][j]) == 0:
            p, r = jp, ar._qmul(jq, np.concatenate([[np.cos(0.5 * qj)], np.sin(0.5 * qj) * axis]))
        else:
            p, r = jp + ar._qrot(jq, axis) * qj, jq
    return p, r


def rooted_chain(A, link, held, q_held):
    """model tables of the solved chain alone, its first joint's frame carrying the held prefix composed at q_held: the
    chain tests/ik_reference.py solves when the held joints are frozen there. `held` must be the path's prefix."""
    path, sel, solved = split_path(A, link, held)
    assert path[: len(held)] == list(held)
    p, r = compose_prefix(A, held, q_held)
    B = {k: np.array(A[k], dtype=np.float64 if np.asarray(A[k]).dtype.kind == "f" else None, copy=True)
         for k in ("dof_frame", "dof_axis", "dof_type", "dof_parent", "dof_limit", "link_body", "link_frame")}
    first = solved[0]
    f = B["dof_frame"][first]
    B["dof_frame"][first] = np.concatenate([p + ar._qrot(r, f[:3]), ar._qmul(r, ar._unit(f[3:]))])
    B["dof_parent"][first] = -1
    return B


def solve(A, link, q0, target_pose, rows, held=(), limits=None, **settings):
    """ik_reference.solve with held joints: q0 [N, n_dof], target_pose [N, 7] -> dict q [N, n_dof] f64 (held and off-path
    dofs copied), iters, err, path, solved, raw_step"""
    q0, T = np.asarray(q0, dtype=np.float64), np.asarray(target_pose, dtype=np.float64)
    limits = np.asarray(A["dof_limit"] if limits is None else limits, dtype=np.float64)
    path, sel, solved = split_path(A, link, list(held))
    lo, hi = limits[solved, 0], limits[solved, 1]
    s = dict(ik.DEFAULTS, **settings)
    N = len(q0)
    q, iters, errs, raw = q0[:, path].copy(), np.zeros(N, dtype=np.int64), np.zeros(N), np.zeros(N)
    active = np.ones(N, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for it in range(s["max_iters"] + 1):
            idx = np.flatnonzero(active)
            if idx.size == 0:
                break
            err, J = ik.pose_error_batch(A, link, path, q[idx], T[idx], rows)
            J = J[:, :, sel]
            m = np.abs(err).max(1)
            errs[idx] = m
            nan = np.isnan(m) & (it < s["max_iters"])  # every solved entry is NaN from here on
            for k in sel:
                q[idx[nan], k] = np.nan
            iters[idx[nan]] = s["max_iters"]
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
            qs = q[idx][:, sel]
            q[np.ix_(idx, sel)] = np.minimum(np.maximum(qs + step, lo), hi)
            iters[idx] += 1
    out = q0.copy()
    out[:, solved] = q[:, sel]
    return dict(q=out, iters=iters, err=errs, path=path, solved=solved, raw_step=raw)


def residual(A, link, q, target, rows):
    """max|err| of one env at the full joint vector q [n_dof]"""
    path = ar.path_dofs(A, link)
    return float(np.abs(ik.pose_error(A, link, path, np.asarray(q, np.float64)[path], target[:3], target[3:], rows)[0]).max())


def apply(ikspec, A, qpos, prev_pose, action, held=(), **settings):
    """the iterative block's map form (ik_reference.apply with held joints)"""
    pose = ik.compose(ikspec, prev_pose, action)
    out = solve(A, int(ikspec[0]), qpos, pose, int(ikspec[2]), held=held, **settings)
    out["pose"] = pose
    return out


def apply_action(spec, A, qpos, prev_tq, prev_tv, action):
    """action_reference.apply_action where flags may carry bit 64: the joint-space rows as there (the bit does not speak
    to them), the end-effector block over the columns of the path joints NOT flagged 64. Same dict."""
    column, low, high, flags, ee = spec
    out = ar.apply_action((column, low, high, flags, None), A, qpos, prev_tq, prev_tv, action)
    if ee is None or ee[0] < 0:
        return out
    qpos, action = np.asarray(qpos, dtype=np.float64), np.asarray(action, dtype=np.float64)
    link, rows = int(ee[0]), int(ee[2])
    f = lambda x: float(np.float32(x))
    cmd = ar.ee_command((link, ee[1], rows, f(ee[3]), f(ee[4]), f(ee[5]), ee[6]), action)
    path = ar.path_dofs(A, link)
    cols = [j for j in path if not int(flags[j]) & 64]
    J = ar.link_fk_jacobian(A, qpos, link)[2][:, :rows][:, :, cols]
    G = J @ J.transpose(0, 2, 1) + ar.RIDGE * np.eye(rows)
    with np.errstate(invalid="ignore"):
        dq = np.einsum("nrj,nr->nj", J, np.linalg.solve(G, cmd[:, :, None])[:, :, 0])
    out["kappa"], out["kappa_j"], out["dq_inf"] = np.linalg.cond(G, 2), np.linalg.cond(J, 2), np.abs(dq).max(1)
    out["dq"], out["path"] = dq, cols
    for k, j in enumerate(cols):
        if int(flags[j]) & 4:
            out["tq"][:, j], out["wq"][j] = qpos[:, j] + dq[:, k], True
            out["ee_dofs"].append(j)
    return out
