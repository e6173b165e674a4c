"""The native action map (include/mssim.h `set_action_map`, `set_ee_action_map`, `apply_action`) restated in
float64 numpy: what the drive targets of one control step must be, given the map as the ABI receives it, the
model's constant tables, the joint positions the controllers read and the action. No torch, nothing imported
from the package: the only things shared with the code under test are the documented rules.

Joint-space rows (per dof j with column[j] >= 0):
    a = action[column[j]];  flags & 2: a = mid + half * clip(a, -1, 1), mid = (high + low) / 2, half = (high - low) / 2
    flags & 16 / & 32: a *= cos / sin(qpos[(flags >> 8) & 31])
    flags & 8: velocity target = a, else position target = (flags & 1 ? qpos[j] : 0) + a
End-effector block (rows 3 or 6): translation clipped + mapped like a joint row, rotation vector limited to norm 1
then times rot_scale; the dofs flagged 4 on the link's path get  qpos + J^T (J J^T + 1e-9 I)^-1 a  with J the
link's Jacobian over ALL joints on its path, in the root frame, from the module's own FK of the chain (which never
sees the root pose: the answer cannot depend on it).

Non-finite actions follow numpy.clip: NaN stays NaN, +-inf clips to the bound where the row is normalised."""
import numpy as np

RIDGE = 1e-9
EPS32 = 2.0 ** -23
KAPPA_CAP = 1e4  # end-effector entries are compared tightly only where kappa_2(J J^T + 1e-9 I) is at most this


def _qmul(a, b):
    aw, ax, ay, az = np.moveaxis(a, -1, 0)
    bw, bx, by, bz = np.moveaxis(b, -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def _qrot(q, v):
    w, u = q[..., :1], q[..., 1:]
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def _unit(q):
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def path_dofs(A, link):
    """dofs on the path root -> link, root side first (body b is moved by dof b)"""
    out, b = [], int(A["link_body"][link])
    while b >= 0:
        out.append(b)
        b = int(A["dof_parent"][b])
    return out[::-1]


def link_fk_jacobian(A, q, link):
    """q [N, n_dof] -> link position [N, 3], quaternion [N, 4] and geometric Jacobian [N, 6, n_dof] (rows linear then
    angular velocity of the link frame origin per unit joint velocity), all in the articulation's root frame"""
    q = np.asarray(q, dtype=np.float64)
    N, n = q.shape
    p = np.zeros((N, 3))
    r = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (N, 1))
    axes, anchors, path = [], [], path_dofs(A, link)
    for j in path:
        frame = np.asarray(A["dof_frame"][j], dtype=np.float64)
        axis = np.asarray(A["dof_axis"][j], dtype=np.float64)
        jp = p + _qrot(r, frame[:3])
        jq = _qmul(r, np.broadcast_to(_unit(frame[3:]), (N, 4)))
        a = _qrot(jq, axis)
        axes.append(a)
        anchors.append(jp)
        if int(A["dof_type"][j]) == 0:  # revolute
            h = 0.5 * q[:, j : j + 1]
            p, r = jp, _qmul(jq, np.concatenate([np.cos(h), np.sin(h) * axis], 1))
        else:  # prismatic
            p, r = jp + a * q[:, j : j + 1], jq
    tip = np.asarray(A["link_frame"][link], dtype=np.float64)
    pe = p + _qrot(r, tip[:3])
    qe = _qmul(r, np.broadcast_to(_unit(tip[3:]), (N, 4)))
    J = np.zeros((N, 6, n))
    for j, a, an in zip(path, axes, anchors):
        if int(A["dof_type"][j]) == 0:
            J[:, :3, j] = np.cross(a, pe - an)
            J[:, 3:, j] = a
        else:
            J[:, :3, j] = a
    return pe, qe, J


def clip_affine(a, low, high):
    with np.errstate(invalid="ignore"):
        return 0.5 * (high + low) + 0.5 * (high - low) * np.clip(a, -1.0, 1.0)


def ee_command(ee, action):
    """the end-effector tuple (link, column0, rows, low, high, rot_scale, flags) and the action -> [N, rows] command"""
    link, c0, rows, low, high, rot_scale, flags = ee
    lin = action[:, c0 : c0 + 3]
    if flags & 2:
        lin = clip_affine(lin, low, high)
    if rows == 3:
        return lin
    rot = action[:, c0 + 3 : c0 + 6]
    if flags & 2:
        with np.errstate(invalid="ignore", over="ignore"):
            nr = np.linalg.norm(rot, axis=1, keepdims=True)
            rot = np.where(nr > 1.0, rot / np.maximum(nr, 1e-12), rot) * rot_scale
    return np.concatenate([lin, rot], 1)


def apply_action(spec, A, qpos, prev_tq, prev_tv, action):
    """spec = (column, low, high, flags, ee) as handed to set_action_map / set_ee_action_map (low / high / rot_scale:
    the float32 values), qpos / prev_tq / prev_tv [N, n_dof], action [N, action_dim]. Returns a dict:
    tq, tv [N, n_dof] f64 (previous values where the map writes nothing), wq, wv [n_dof] bool (written or not),
    base [n_dof] bool (rows with a cos / sin factor), ee_dofs (list), kappa [N] (cond_2 of G; 1 without a block),
    dq_inf [N] (max |delta q| of the block), kappa_j [N] (cond_2 of J), dq [N, len(path)] (the block's delta itself)"""
    column, low, high, flags, ee = spec
    qpos, action = np.asarray(qpos, dtype=np.float64), np.asarray(action, dtype=np.float64)
    N, n = qpos.shape
    tq, tv = np.array(prev_tq, dtype=np.float64), np.array(prev_tv, dtype=np.float64)
    wq, wv, base = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    for j in range(n):
        if column[j] < 0:
            continue
        a, fl = action[:, column[j]], int(flags[j])
        if fl & 2:
            a = clip_affine(a, float(np.float32(low[j])), float(np.float32(high[j])))
        if fl & 48:
            yaw = qpos[:, (fl >> 8) & 31]
            a = a * (np.cos(yaw) if fl & 16 else np.sin(yaw))
            base[j] = True
        if fl & 8:
            tv[:, j], wv[j] = a, True
        else:
            tq[:, j], wq[j] = (qpos[:, j] if fl & 1 else 0.0) + a, True
    out = dict(tq=tq, tv=tv, wq=wq, wv=wv, base=base, ee_dofs=[], kappa=np.ones(N), dq_inf=np.zeros(N), kappa_j=np.ones(N))
    if ee is not None and ee[0] >= 0:
        link, rows = int(ee[0]), int(ee[2])
        cmd = ee_command((link, ee[1], rows, float(np.float32(ee[3])), float(np.float32(ee[4])), float(np.float32(ee[5])), ee[6]), action)
        path = path_dofs(A, link)
        J = link_fk_jacobian(A, qpos, link)[2][:, :rows][:, :, path]
        G = J @ J.transpose(0, 2, 1) + RIDGE * np.eye(rows)
        with np.errstate(invalid="ignore"):
            dq = np.einsum("nrj,nr->nj", J, np.linalg.solve(G, cmd[:, :, None])[:, :, 0])
        out["kappa"] = np.linalg.cond(G, 2)
        out["kappa_j"] = np.linalg.cond(J, 2)
        out["dq_inf"] = np.abs(dq).max(1)
        out["dq"], out["path"] = dq, path
        for k, j in enumerate(path):
            if int(flags[j]) & 4:
                tq[:, j], wq[j] = qpos[:, j] + dq[:, k], True
                out["ee_dofs"].append(j)
    return out


def joint_bound(spec, qpos, R):
    """derived float32 band of the joint-space entries, [N, n_dof]: four roundings (mid, half, product, sum; one more
    sum with the delta flag is covered by |q| and |target| both being in m), each at most half an ulp of a quantity
    no larger than m = max(|low|, |high|, |q|, |target|) -> 4 * 2^-23 * m; rows with a cos / sin factor twice that"""
    column, low, high, flags, _ = spec
    qpos = np.asarray(qpos, dtype=np.float64)
    t = np.where(R["wv"][None, :], R["tv"], R["tq"])
    m = np.maximum(np.maximum(np.abs(np.asarray(low, np.float64)), np.abs(np.asarray(high, np.float64)))[None, :], np.abs(t))
    m = np.maximum(m, np.where((np.asarray(flags) & 1).astype(bool)[None, :], np.abs(qpos), 0.0))
    return np.where(R["base"][None, :], 8.0, 4.0) * EPS32 * m


def ee_bound(K, qpos, R, K2=0.0):
    """float32 band of the end-effector entries, [N, 1]: K 2^-23 kappa_2(G) |dq|_inf (+ K2 2^-23 kappa_2(J) |dq|_inf)
    + 4 * 2^-23 |q| (per entry, added by the caller's broadcasting)"""
    return (K * R["kappa"] + K2 * R["kappa_j"])[:, None] * EPS32 * R["dq_inf"][:, None] + 4.0 * EPS32 * np.abs(np.asarray(qpos, np.float64))
