"""Constructed cases for the native action map, one per env (tests/action_reference.py states what must come out).

Env i holds base case b = i // 3 under root pose variant i % 3 (identity, displaced, displaced + seeded random
rotation): the three envs of a base case are twins -- same joints, same action, another root pose -- and the
reference's answer is the same for all three. A base case combines, by index arithmetic with coprime periods so that
every combination turns up within the 43 base cases of N = 128:
  * the arm pose set (b % 4): rest keyframe, rest +- 0.3, rest +- 1.0 and uniform within the limits (all clamped to
    the joint limits; unlimited joints are drawn from [-pi, pi]);
  * the action: column c takes VALUES[(b + c) % 17] -- the clip edges, far outside, signed zeros, the smallest normal
    float32 and seeded uniform values; columns of a map that is not normalised (`pd_joint_pos`) take values at and
    beyond the joint limits instead;
  * end-effector maps: the translation is zero, saturated or taken from VALUES ((b // 4) % 3) and the rotation
    vector is one of ROTATIONS (b % 11): norm 0, exactly 1, 1 -+ 1e-3, 10, along one axis and oblique, seeded;
  * Fetch: the yaw joint at 0, +-pi/2, pi, +-100 rad or seeded (b % 8), the forward column zero, saturated or from
    VALUES (b % 5).
The previous targets hold a pattern that names env and dof, so "left alone" is checkable bit for bit. `nonfinite=True`
(the stand-alone form only) puts NaN / +inf / -inf into every column of the LAST env's action."""
import numpy as np

from tests import action_reference as ref

SEED = 20261016
TINY = float(np.finfo(np.float32).tiny)
_U = None  # seeded uniform value, drawn per (base case, column)
VALUES = [-1.0, 1.0, 1.0 - 1e-3, 1.0 + 1e-3, -(1.0 - 1e-3), -(1.0 + 1e-3), 1.5, -1.5, 1e6, -1e6, 0.0, -0.0, TINY, -TINY, _U, _U, _U]
VALUE_NAMES = ["-1", "+1", "1-1e-3", "1+1e-3", "-(1-1e-3)", "-(1+1e-3)", "1.5", "-1.5", "1e6", "-1e6", "+0", "-0", "tiny", "-tiny", "u", "u", "u"]
_S3 = 1.0 / np.sqrt(3.0)
ROTATIONS = [("rot0", (0, 0, 0)), ("rot1x", (1, 0, 0)), ("rot1obl", (2 / 3, -2 / 3, 1 / 3)), ("rot1-", (0, 1 - 1e-3, 0)),
             ("rot1+obl", tuple((1 + 1e-3) * _S3 * s for s in (1, 1, -1))), ("rot1+z", (0, 0, -(1 + 1e-3))), ("rot10y", (0, 10, 0)),
             ("rot10obl", tuple(10 * _S3 * s for s in (-1, 1, 1))), ("rot1-obl", tuple((1 - 1e-3) * _S3 * s for s in (1, -1, 1))),
             ("rot_u_small", None), ("rot_u_big", None)]
POSE_SETS = ["rest", "rest03", "rest10", "uniform"]
YAWS = [0.0, np.pi / 2, -np.pi / 2, np.pi, 100.0, -100.0, None, None]
ENV_COUNTS = (128, 1, 17, 67)

# name -> (env id, gym.make keywords); the map itself is the controller's own fused_action_spec()
MAPS = {
    "panda:pd_joint_delta_pos": ("Empty-v1", dict(robot_uids="panda", control_mode="pd_joint_delta_pos")),
    "panda:pd_joint_pos": ("Empty-v1", dict(robot_uids="panda", control_mode="pd_joint_pos")),
    "panda:pd_joint_vel": ("Empty-v1", dict(robot_uids="panda", control_mode="pd_joint_vel")),
    "panda:pd_ee_delta_pos": ("Empty-v1", dict(robot_uids="panda", control_mode="pd_ee_delta_pos")),
    "panda:pd_ee_delta_pose": ("Empty-v1", dict(robot_uids="panda", control_mode="pd_ee_delta_pose")),
    "panda_stick:pd_joint_delta_pos": ("Empty-v1", dict(robot_uids="panda_stick", control_mode="pd_joint_delta_pos")),
    "fetch:pd_joint_delta_pos": ("Empty-v1", dict(robot_uids="fetch", control_mode="pd_joint_delta_pos")),
}
# two maps no robot produces, on the Panda (9 dofs): a dof without a column in the middle of the arm; two blocks of
# dofs sharing one column each, with their own bounds and flags
HAND_MAPS = {
    "panda:hole": ([0, 1, 2, -1, 3, 4, 5, 6, 6], [-0.1] * 3 + [0.0] + [-0.2] * 3 + [-0.01] * 2, [0.1] * 3 + [0.0] + [0.3] * 3 + [0.04] * 2,
                   [3, 3, 3, 0, 3, 3, 3, 2, 2], None),
    "panda:shared": ([0, 0, 0, 0, 1, 1, 1, 2, 2], [-0.1, -0.2, -0.3, -0.4, -1.0, -1.0, -1.0, -0.01, -0.01], [0.1, 0.2, 0.5, 0.4, 1.0, 2.0, 1.0, 0.04, 0.04],
                     [3, 3, 3, 3, 10, 10, 10, 2, 2], None),
}


def env_spec(name):
    return ("Empty-v1", dict(robot_uids="panda", control_mode="pd_joint_delta_pos")) if name in HAND_MAPS else MAPS[name]


def action_dim(spec):
    column, _, _, _, ee = spec
    return max(max(column) + 1, ee[1] + ee[2] if ee is not None else 0)


def pattern(N, n):
    """previous position / velocity targets: value names env and dof, exact in float32"""
    i, j = np.arange(N, dtype=np.float64)[:, None], np.arange(n, dtype=np.float64)[None, :]
    return (1000.0 + i + j / 32.0).astype(np.float32), (-(2000.0 + i + j / 32.0)).astype(np.float32)


def _quat_mul(a, b):
    return ref._qmul(np.asarray(a, np.float64), np.asarray(b, np.float64))


def build(name, spec, limits, rest, root0, N, nonfinite=False):
    """-> dict of float32 arrays qpos [N, n], root [N, 7], action [N, adim], prev_tq / prev_tv [N, n] and per env the
    label, the pose set and the base case index (twins share it)"""
    column, low, high, flags, ee = spec
    n, adim = len(column), action_dim(spec)
    rng = np.random.default_rng([SEED, sum(map(ord, name)), N])
    lim = np.asarray(limits, dtype=np.float64).copy()
    lim[lim[:, 0] < -1e30, 0], lim[lim[:, 1] > 1e30, 1] = -np.pi, np.pi
    rest = np.asarray(rest, dtype=np.float64)
    abs_col = {}  # column -> dof whose limits its values are drawn around (rows that are not normalised)
    for j in range(n):
        if column[j] >= 0 and not (int(flags[j]) & 2):
            abs_col.setdefault(column[j], j)
    fetch = name.startswith("fetch")
    qpos, root, action = np.zeros((N, n)), np.zeros((N, 7)), np.zeros((N, adim))
    labels, pose_set, base = [], [], []
    for b in range((N + 2) // 3):
        ps = POSE_SETS[b % 4]
        u = rng.uniform(-1.0, 1.0, n)
        q = {"rest": rest, "rest03": rest + 0.3 * u, "rest10": rest + 1.0 * u, "uniform": 0.5 * (lim[:, 0] + lim[:, 1]) + 0.5 * (lim[:, 1] - lim[:, 0]) * u}[ps]
        q = np.clip(q, lim[:, 0], lim[:, 1])
        a, names = np.zeros(adim), []
        for c in range(adim):
            k = (b + c) % len(VALUES)
            uc = rng.uniform(-1.0, 1.0)
            if c in abs_col:
                lo, hi = lim[abs_col[c]]
                lo32, hi32 = np.float32(lo), np.float32(hi)
                table = [lo, hi, lo - 0.25, hi + 0.25, float(np.nextafter(lo32, np.float32(-np.inf))), float(np.nextafter(hi32, np.float32(np.inf))),
                         0.5 * (lo + hi), 1e6, -1e6, -0.0, TINY, lo - 10.0, hi + 10.0] + [0.5 * (lo + hi) + 0.5 * (hi - lo) * uc] * 4
                a[c] = table[k]
                names.append(["lo", "hi", "lo-.25", "hi+.25", "lo-ulp", "hi+ulp", "mid", "1e6", "-1e6", "-0", "tiny", "lo-10", "hi+10", "u", "u", "u", "u"][k])
            else:
                a[c] = uc if VALUES[k] is None else VALUES[k]
                names.append(VALUE_NAMES[k])
        if ee is not None:
            c0, rows = ee[1], ee[2]
            tmode = (b // 4) % 3
            if tmode == 0:
                a[c0 : c0 + 3], names[c0 : c0 + 3] = 0.0, ["t0"] * 3
            elif tmode == 1:
                a[c0 : c0 + 3], names[c0 : c0 + 3] = [1.5, -1.5, 1.0], ["tsat"] * 3
            if rows == 6:
                rname, rv = ROTATIONS[b % len(ROTATIONS)]
                if rv is None:
                    rv = rng.uniform(-1.0, 1.0, 3) * (0.3 if rname == "rot_u_small" else 3.0)
                a[c0 + 3 : c0 + 6], names[c0 + 3 : c0 + 6] = rv, [rname] * 3
        if fetch:
            yaw = YAWS[b % len(YAWS)]
            q[2] = rng.uniform(-np.pi, np.pi) if yaw is None else yaw
            fcol = column[0]
            if b % 5 == 0:
                a[fcol], names[fcol] = 0.0, "fwd0"
            elif b % 5 == 1:
                a[fcol], names[fcol] = 1.5, "fwdsat"
            names.append(f"yaw={q[2]:.4g}")
        for r in range(3):
            i = 3 * b + r
            if i >= N:
                break
            pose = np.array(root0, dtype=np.float64)
            if r >= 1:
                pose[:3] += rng.uniform(-0.5, 0.5, 3) + np.array([0.0, 0.0, 1.0])
            if r == 2:
                rq = rng.normal(size=4)
                pose[3:] = _quat_mul(rq / np.linalg.norm(rq), pose[3:])
            qpos[i], root[i], action[i] = q, pose, a
            labels.append(f"{name} N={N} env {i}: case {b} {ps} root={('id', 'moved', 'tilted')[r]} a=[{' '.join(names)}]")
            pose_set.append(ps)
            base.append(b)
    if nonfinite:
        action[N - 1] = np.resize([np.nan, np.inf, -np.inf], adim)
        labels[N - 1] += " NONFINITE nan/+inf/-inf"
    ptq, ptv = pattern(N, n)
    f32 = np.float32
    return dict(qpos=qpos.astype(f32), root=root.astype(f32), action=action.astype(f32), prev_tq=ptq, prev_tv=ptv,
                labels=labels, pose_set=np.array(pose_set), base=np.array(base), nonfinite=nonfinite)


def write_state(base, C):
    """the case table into the simulation of an env (either backend): joints, root poses (row 0 of the body table),
    previous targets; velocities zero; FK refreshed and everything copied back out"""
    import torch

    px, N, dev = base.scene.px, base.num_envs, base.device
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    px.cuda_articulation_qpos.torch()[:] = t(C["qpos"])
    px.cuda_articulation_qvel.torch()[:] = 0
    px.cuda_rigid_body_data.torch()[:N, :7] = t(C["root"])
    px.cuda_rigid_body_data.torch()[:N, 7:] = 0
    px.cuda_articulation_target_qpos.torch()[:] = t(C["prev_tq"])
    px.cuda_articulation_target_qvel.torch()[:] = t(C["prev_tv"])
    px.gpu_apply_all()
    px.gpu_update_articulation_kinematics()
    px.gpu_fetch_all()


def tables(base):
    """(model arrays, joint limits, rest joint positions, initial root pose) of a freshly reset env"""
    A = base.scene.model.arrays
    return A, A["dof_limit"], base.agent.robot.get_qpos()[0].cpu().numpy(), base.scene.px.cuda_rigid_body_data.torch()[0, :7].cpu().numpy()


def reference(spec, A, C):
    """the float64 reference on a case table (inputs widened from the float32 values the kernels read)"""
    return ref.apply_action(spec, A, C["qpos"].astype(np.float64), C["prev_tq"], C["prev_tv"], C["action"].astype(np.float64))


def tight(spec, C, R):
    """envs whose end-effector entries are compared tightly: kappa_2(G) within the cap; the uniform-within-limits
    pose set only with 3 rows (with 6 rows 14 % of such poses are beyond the cap: it serves the finite / untouched
    assertions there)"""
    ok = R["kappa"] <= ref.KAPPA_CAP
    if spec[4] is not None and spec[4][2] == 6:
        ok &= C["pose_set"] != "uniform"
    return ok


def compare(spec, C, R, tq, tv, K, what):
    """tq / tv: the float32 targets of the code under test. Asserts untouched entries bit for bit, joint-space entries
    within their derived bound, end-effector entries within the band of K = (K, K2) where `tight`, everything finite where the
    action is finite, NaN exactly where the reference says NaN. Returns the largest ratio error / bound seen."""
    tq, tv = np.asarray(tq), np.asarray(tv)
    assert tq.dtype == np.float32 and tv.dtype == np.float32
    N, n = tq.shape
    bits = lambda x: np.ascontiguousarray(x, dtype=np.float32).view(np.int32)
    for got, prev, w, kind in ((tq, C["prev_tq"], R["wq"], "position"), (tv, C["prev_tv"], R["wv"], "velocity")):
        same = bits(got) == bits(prev)
        bad = np.argwhere(~same[:, ~w])
        assert bad.size == 0, f"{what}: {kind} target the map must not touch was written: {C['labels'][bad[0][0]]} dof {np.flatnonzero(~w)[bad[0][1]]}"
    jb = ref.joint_bound(spec, C["qpos"], R)
    eb = ref.ee_bound(K[0], C["qpos"], R, K[1])
    tight_env = tight(spec, C, R)
    worst = 0.0
    for j in range(n):
        for got, want, w in ((tq, R["tq"], R["wq"]), (tv, R["tv"], R["wv"])):
            if not w[j]:
                continue
            g, t = got[:, j].astype(np.float64), want[:, j]
            nan = np.isnan(t)
            nan = ~np.isfinite(t)  # (NaN, or +-inf handed through by a row that is not normalised: must come out as such)
            wrong = np.where(nan, ~((g == t) | (np.isnan(g) & np.isnan(t))), ~np.isfinite(g))
            assert not wrong.any(), f"{what}: dof {j} got {g[wrong][0]!r} want {t[wrong][0]!r}: {C['labels'][int(np.flatnonzero(wrong)[0])]}"
            if j in R["ee_dofs"]:
                sel, bound = ~nan & tight_env, eb[:, j]
            else:
                sel, bound = ~nan, jb[:, j]
            with np.errstate(invalid="ignore"):
                err = np.abs(g - t)
            over = sel & (err > bound)
            if over.any():
                i = int(np.flatnonzero(over)[np.argmax((err / np.maximum(bound, 1e-300))[over])])
                raise AssertionError(f"{what}: dof {j} got {g[i]!r} want {t[i]!r} |err| {err[i]:.3e} > bound {bound[i]:.3e} "
                                     f"(kappa {R['kappa'][i]:.3g}): {C['labels'][i]}")
            if sel.any():
                worst = max(worst, float((err[sel] / np.maximum(bound[sel], 1e-300)).max()))
    return worst


def twins_agree(spec, C, R, tq, K, what):
    """root-pose invariance: the end-effector entries of the envs of one base case differ by no more than the band"""
    if not R["ee_dofs"]:
        return
    eb, ok = ref.ee_bound(K[0], C["qpos"], R, K[1]), tight(spec, C, R) & ~np.isnan(R["tq"][:, R["ee_dofs"]]).any(1)
    for i in range(len(C["base"])):
        k = i - i % 3
        if k != i and ok[i] and ok[k]:
            d = np.abs(tq[i, R["ee_dofs"]].astype(np.float64) - tq[k, R["ee_dofs"]].astype(np.float64))
            assert (d <= eb[i, R["ee_dofs"]]).all(), f"{what}: answer changes with the root pose: {C['labels'][i]} vs {C['labels'][k]}: {d.max():.3e}"
