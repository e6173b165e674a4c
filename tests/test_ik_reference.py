"""The float64 iterative-IK reference (tests/ik_reference.py) and its cases (tests/ik_cases.py), checked on the CPU
before the HIP kernel is held to them (tests/test_gpu_ee_ik.py):

  1. the reference is self-consistent: on *near* every env converges below 60 iterations with max|err| < 1e-5; on every
     table the result respects the joint limits and no joint moves more than max_step per iteration; the vectorised
     evaluation equals the one-env-at-a-time statement;
  2. the band: a float32 numpy restatement of the kernel's own formula (FK of the chain, Gram matrix summed joint by
     joint, unpivoted Cholesky, every operation rounded to float32) against the reference, see MEASURED;
  3. the torch solver `Kinematics.compute_ik(..., use_delta_ik_solver=False)` on the f32 oracle backend, called ONE ENV
     AT A TIME (a batch of one: there the batch-wide exit is the per-env exit), agrees with the reference on *near*
     within the band: the native contract is the existing algorithm;
  4. the torch controllers of the three modes (`agent.set_action` on the f32 oracle backend) produce the reference's new
     target pose, position and rotation, within POSE_TOL;
  5. the surface: `fused_action_spec()` of the three modes, the header's declarations, the binding.

MEASURED: the largest |q32 - q_ref|_inf of the restatement over the committed tables (N = 128, 1, 17, 67) plus one table
of 3072 envs, per (set, form, rows); form "default" = the default settings (envs whose iteration count differs from the
reference's are compared by their residual instead, see below), "K1" / "K2" / "K5" = tolerance 0 and exactly K
iterations. Measured with `python -m tests.test_ik_reference`; the recorded value is the measurement rounded up to
two digits. The band used everywhere (here for the torch solver, on the GPU for the kernel) is 4 x the recorded value;
the test asserts that the restatement stays within the recorded value and reaches at least a fifth of it, so the band
is nowhere more than 20 x loose and cannot drift from what it was derived from.

Iteration counts (default settings, *near*): the restatement's count equals the reference's in at least 98 % of the
envs of every table and never differs by more than 1. Envs whose count differs sit at the tolerance threshold, where
one rounding decides whether another step is taken: they are compared by max|err| < 2e-5 at the returned q (the
reference's own residual evaluated in float64), not by q, and at most 2 % of any table may be excused this way."""
import os
import re

import numpy as np
import pytest
import torch

import maniskill_amd  # noqa: F401  (installs the gymnasium stand-in where the real module is absent)
from tests import action_cases as ac
from tests import action_reference as ar
from tests import ik_cases as ic
from tests import ik_reference as ik
from tests import oracle_backend as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA_N = ic.MAX_N
FORMS = [("near", "default")] + [(s, f"K{k}") for s in ("near", "wide") for k in ic.K_FORMS]
# largest |q32 - q_ref|_inf of the float32 restatement, per (set, form, rows); the band is 4 x this
MEASURED = {
    ("near", "default", 3): 2.1e-6, ("near", "default", 6): 2.4e-6,
    ("near", "K1", 3): 1.5e-6, ("near", "K1", 6): 2.0e-6,
    ("near", "K2", 3): 1.6e-6, ("near", "K2", 6): 2.1e-6,
    ("near", "K5", 3): 1.4e-6, ("near", "K5", 6): 3.2e-6,
    ("wide", "K1", 3): 1.8e-6, ("wide", "K1", 6): 2.2e-5,
    ("wide", "K2", 3): 3.1e-6, ("wide", "K2", 6): 3.1e-5,
    ("wide", "K5", 3): 7.6e-6, ("wide", "K5", 6): 1.6e-4,
}
# Target pose of one control step, float32 torch against the float64 reference. One quaternion product: each component
# is a sum of four products of entries at most 1 in magnitude -> 4 roundings of products + 3 of sums, each half an ulp
# of a quantity at most 2: 7 * 2^-24 * 2. The Euler quaternion goes through two more such stages in torch (the matrix
# product Rx Ry Rz, the matrix -> quaternion conversion), so three stages in all; the position is one sum of entries
# below 2 (half an ulp of 2) after the affine map of the columns (three roundings of quantities below 1).
EPS = 2.0 ** -24
QUAT_TOL = 3 * 7 * EPS * 2.0   # per component, after aligning the sign; also the bound on 1 - |<q, q_ref>|
POS_TOL = (2.0 + 3.0) * EPS
MODES = ["pd_ee_target_delta_pos", "pd_ee_target_delta_pose", "pd_ee_pose"]


def settings_of(form):
    return {} if form == "default" else dict(tolerance=0.0, max_iters=int(form[1:]))


def band(name, form, rows):
    return 4.0 * MEASURED[(name, form, rows)]


# ---------------------------------------------------------------- float32 restatement of the kernel's formula
def ik_f32(A, link, q0, target, rows, max_iters=60, damping=1e-3, max_step=0.3, tolerance=1e-5):
    """every operation rounded to float32, in the kernel's order -> (q [N, n_dof] f32, iters [N])"""
    f = np.float32
    path = ar.path_dofs(A, link)
    unit = lambda fr: np.concatenate([fr[:3], fr[3:] / np.linalg.norm(fr[3:])]).astype(f)  # normalised in double, as the host does
    frames = [unit(np.asarray(A["dof_frame"][j], np.float64)) for j in path]
    axes = [np.asarray(A["dof_axis"][j], f) for j in path]
    rev = [int(A["dof_type"][j]) == 0 for j in path]
    tip = unit(np.asarray(A["link_frame"][link], np.float64))
    lim = np.asarray(A["dof_limit"], f)[path]
    damping, max_step, tolerance = f(damping), f(max_step), f(tolerance)
    q0 = np.asarray(q0, f)
    N = len(q0)
    Q, T = q0[:, path].copy(), np.asarray(target, f)
    iters, active = np.zeros(N, np.int64), np.ones(N, bool)
    conj = np.array([1, -1, -1, -1], f)
    with np.errstate(invalid="ignore", over="ignore"):
        for it in range(max_iters + 1):
            idx = np.flatnonzero(active)
            if idx.size == 0:
                break
            q, M = Q[idx], len(idx)
            p, r = np.zeros((M, 3), f), np.tile(np.array([1, 0, 0, 0], f), (M, 1))
            ax, an = [], []
            for k in range(len(path)):
                jp = p + ar._qrot(r, frames[k][:3])
                jq = ar._qmul(r, np.broadcast_to(frames[k][3:], (M, 4)))
                a = ar._qrot(jq, axes[k])
                ax.append(a)
                an.append(jp)
                if rev[k]:
                    h = f(0.5) * q[:, k : k + 1]
                    p, r = jp, ar._qmul(jq, np.concatenate([np.cos(h), np.sin(h) * axes[k]], 1))
                else:
                    p, r = jp + a * q[:, k : k + 1], jq
            pe = p + ar._qrot(r, tip[:3])
            err = T[idx, :3] - pe
            if rows == 6:
                qe = ar._qmul(r, np.broadcast_to(tip[3:], (M, 4)))
                d = ar._qmul(T[idx, 3:], qe * conj)
                d = np.where(d[:, :1] < 0, -d, d)
                nv = np.sqrt((d[:, 1:2] * d[:, 1:2] + d[:, 2:3] * d[:, 2:3]) + d[:, 3:4] * d[:, 3:4])
                ang = f(2) * np.arctan2(nv, d[:, :1])
                err = np.concatenate([err, d[:, 1:] / np.maximum(nv, f(1e-9)) * ang], 1)
            assert err.dtype == f and pe.dtype == f
            stop = (np.abs(err).max(1) < tolerance) | (it >= max_iters)
            active[idx[stop]] = False
            idx, err = idx[~stop], err[~stop]
            if idx.size == 0:
                continue
            M = len(idx)
            J = np.zeros((M, rows, len(path)), f)
            G = np.zeros((M, rows, rows), f)
            G[:, np.arange(rows), np.arange(rows)] = damping
            for k in range(len(path)):
                a, anc = ax[k][~stop], an[k][~stop]
                J[:, :3, k] = np.cross(a, pe[~stop] - anc) if rev[k] else a
                if rows == 6 and rev[k]:
                    J[:, 3:, k] = a
                G = G + J[:, :, None, k] * J[:, None, :, k]
            L = np.zeros((M, rows, rows), f)
            for i in range(rows):
                for j in range(i + 1):
                    s = G[:, i, j].copy()
                    for m in range(j):
                        s = s - L[:, i, m] * L[:, j, m]
                    L[:, i, j] = np.sqrt(np.maximum(s, f(1e-20))) if i == j else s / L[:, j, j]
            z, y = np.zeros((M, rows), f), np.zeros((M, rows), f)
            for i in range(rows):
                s = err[:, i].copy()
                for m in range(i):
                    s = s - L[:, i, m] * z[:, m]
                z[:, i] = s / L[:, i, i]
            for i in range(rows - 1, -1, -1):
                s = z[:, i].copy()
                for m in range(i + 1, rows):
                    s = s - L[:, m, i] * y[:, m]
                y[:, i] = s / L[:, i, i]
            step = np.zeros((M, len(path)), f)
            for i in range(rows):
                step = step + J[:, i, :] * y[:, i : i + 1]
            big = np.abs(step).max(1)
            step = step * (max_step / np.maximum(big, max_step))[:, None]
            assert step.dtype == f and L.dtype == f
            Q[idx] = np.minimum(np.maximum(Q[idx] + step, lim[:, 0]), lim[:, 1])
            iters[idx] += 1
    out = q0.copy()
    out[:, path] = Q
    return out, iters


_REF = {}


def reference(A, rest, name, form, rows, N, nan=False):
    """the reference's result on a case table, computed once per table and shared (treat as read-only); carries
    "residual": (env, q [n_dof]) -> max|err| at q in float64"""
    key = (name, form, rows, N, nan)
    if key not in _REF:
        C = ic.build(A, rest, name, rows, N, nan=nan)
        R = ik.solve(A, ic.LINK, C["q0"], C["target"], rows, **settings_of(form))
        T, path = C["target"].astype(np.float64), R["path"]
        R["residual"] = lambda e, q: float(np.abs(ik.pose_error(A, ic.LINK, path, np.asarray(q, np.float64)[path], T[e, :3], T[e, 3:], rows)[0]).max())
        _REF[key] = (C, R)
    return _REF[key]


def _measure(A, rest, name, form, rows):
    worst = 0.0
    for N in ic.ENV_COUNTS + (EXTRA_N,):
        C, R = reference(A, rest, name, form, rows, N)
        q, iters = ik_f32(A, ic.LINK, C["q0"], C["target"], rows, **settings_of(form))
        worst = max(worst, ic.compare(C, R, q, iters, 0.0, f"restatement {name} {form} rows={rows} N={N}", measured=True))
    return worst


@pytest.fixture(scope="module")
def panda():
    return ic.panda_tables()


# ---------------------------------------------------------------- 1. self-consistency
@pytest.mark.parametrize("rows", ic.ROWS)
@pytest.mark.parametrize("name", list(ic.SETS))
def test_reference_is_self_consistent(panda, name, rows):
    A, rest = panda
    lim = np.asarray(A["dof_limit"], np.float64)
    for N in ic.ENV_COUNTS:
        C, R = reference(A, rest, name, "default", rows, N)
        path = R["path"]
        assert (R["q"][:, path] >= lim[path, 0]).all() and (R["q"][:, path] <= lim[path, 1]).all()
        off = [j for j in range(R["q"].shape[1]) if j not in path]
        assert np.array_equal(R["q"][:, off], C["q0"][:, off].astype(np.float64))
        if name == "near":
            assert (R["iters"] < 60).all() and (R["err"] < 1e-5).all(), (N, R["iters"].max(), R["err"].max())
        else:
            assert (R["iters"] <= 60).all()
    # the step cap: exactly one iteration moves no joint by more than max_step, although the raw step was larger somewhere
    C, R1 = reference(A, rest, "wide", "K1", rows, 128)
    moved = np.abs(R1["q"] - C["q0"].astype(np.float64)).max(1)
    assert (moved <= 0.3 + 1e-12).all() and (R1["raw_step"] > 0.3).any()
    # the vectorised evaluation is the one-env-at-a-time statement
    C, R = reference(A, rest, name, "default", rows, 17)
    for e in range(17):
        q, it, err, _ = ik.solve_env(A, ic.LINK, C["q0"][e, R["path"]].astype(np.float64), C["target"][e, :3].astype(np.float64),
                                     C["target"][e, 3:].astype(np.float64), rows, lim)
        assert it == R["iters"][e] and np.abs(q - R["q"][e, R["path"]]).max() <= 1e-12 and abs(err - R["err"][e]) <= 1e-12
    # a NaN in the last env's target: NaN on its path dofs, nowhere else
    C, R = reference(A, rest, name, "default", rows, 17, nan=True)
    assert np.isnan(R["q"][16, R["path"]]).all() and np.isfinite(np.delete(R["q"], 16, 0)).all() and np.isfinite(R["q"][16, 7:]).all()


def test_case_tables_are_prefixes_and_euler_angles_round_trip(panda):
    A, rest = panda
    for rows in ic.ROWS:
        big = ic.build(A, rest, "near", rows, 128)
        for N in (1, 17, 67):
            C = ic.build(A, rest, "near", rows, N)
            assert np.array_equal(C["q0"], big["q0"][:N]) and np.array_equal(C["target"], big["target"][:N])
    q = ar._unit(np.random.default_rng(3).normal(size=(64, 4)))
    assert ik.rotation_distance(ik.euler_xyz_quat(ic.quat_to_euler_xyz(q)), q).max() < 1e-12


# ---------------------------------------------------------------- 2. the band
@pytest.mark.parametrize("rows", ic.ROWS)
@pytest.mark.parametrize("name,form", FORMS)
def test_float32_restatement_stays_within_the_recorded_band(panda, name, form, rows):
    A, rest = panda
    worst = _measure(A, rest, name, form, rows)
    rec = MEASURED[(name, form, rows)]
    print(f"{name} {form} rows={rows}: largest |q32 - q_ref| {worst:.3e}, recorded {rec:.3e}")
    assert worst <= rec, (name, form, rows, worst)
    assert worst >= rec / 5.0, f"the band (4 x {rec:.3e}) is more than 20 x loose: the restatement reaches {worst:.3e}"


# ---------------------------------------------------------------- 3. the torch solver, one env at a time
def _make(mode, N, robot="panda", env_id="Empty-v1"):
    import gymnasium as gym

    import maniskill_amd.envs  # noqa: F401

    backend = ob.register("f32", "oracle_f32_env")
    env = gym.make(env_id, num_envs=N, sim_backend=backend, robot_uids=robot, control_mode=mode)
    env.reset(seed=0)
    return env


@pytest.mark.parametrize("rows", ic.ROWS)
def test_torch_solver_one_env_at_a_time_matches_reference(panda, rows):
    from maniskill_amd.utils.structs.pose import Pose

    A, rest = panda
    env = _make("pd_ee_target_delta_pose", 1)
    kin = env.unwrapped.agent.controller.controllers["arm"].kinematics
    assert kin.end_link_idx == ic.LINK and kin.active_ancestor_joint_idxs == ar.path_dofs(A, ic.LINK)
    N = 67
    C, R = reference(A, rest, "near", "default", rows, N)
    q = C["q0"].copy()
    for e in range(N):
        got = kin.compute_ik(Pose.create(torch.from_numpy(C["target"][e : e + 1])), torch.from_numpy(C["q0"][e : e + 1]), pos_only=rows == 3)
        q[e, R["path"]] = got[0].numpy()
    env.close()
    res = np.array([R["residual"](e, q[e]) for e in range(N)])
    # the torch loop does not report its count: an env is compared by q unless its residual says that it stopped an
    # iteration away from the reference (count conditions as for the restatement: at most 2 % of the table)
    dq = np.abs(q.astype(np.float64) - R["q"]).max(1)
    far = dq > band("near", "default", rows)
    assert far.sum() <= 0.02 * N and (res[far] < 2e-5).all(), (rows, dq.max(), res.max())
    assert (res < 2e-5).all()


# ---------------------------------------------------------------- 4. the torch controllers' target pose
def _controller_case(A, rest, base, N):
    spec = base.agent.controller.fused_action_spec()
    ikspec = spec[5]
    M = ic.build_map(A, rest, ikspec, N)
    action = np.zeros((N, base.agent.controller.single_action_space.shape[0]), np.float32)
    action[:, ikspec[1] : ikspec[1] + ikspec[2]] = M["columns"]
    return ikspec, M, action


def pose_close(got, want, scale, what):
    """position within scale * POS_TOL, rotation within scale * QUAT_TOL: 1 - |<q, q_ref>| and, sign aligned, per component"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    dp = np.abs(got[:, :3] - want[:, :3]).max()
    assert dp <= scale * POS_TOL * max(1.0, np.abs(want[:, :3]).max()), f"{what}: position off by {dp:.3e}"
    dot = (got[:, 3:] * want[:, 3:]).sum(1)
    assert (np.abs(1.0 - np.abs(dot)) <= scale * QUAT_TOL).all(), f"{what}: 1 - |<q, q_ref>| = {np.abs(1.0 - np.abs(dot)).max():.3e}"
    dq = np.abs(got[:, 3:] - np.sign(dot)[:, None] * want[:, 3:]).max()
    assert dq <= scale * QUAT_TOL, f"{what}: rotation off by {dq:.3e}"


@pytest.mark.parametrize("mode", MODES)
def test_torch_controllers_give_the_reference_target_pose(panda, mode):
    A, rest = panda
    N = 67
    env = _make(mode, N)
    base = env.unwrapped
    arm = base.agent.controller.controllers["arm"]
    ikspec, M, action = _controller_case(A, rest, base, N)
    from maniskill_amd.utils.structs.pose import Pose

    qpos = np.tile(base.agent.robot.get_qpos()[0].numpy(), (N, 1))
    qpos[:, :7] = M["q0"][:, :7]
    px = base.scene.px
    px.cuda_articulation_qpos.torch()[:] = torch.from_numpy(qpos)
    px.gpu_apply_all()
    px.gpu_update_articulation_kinematics()
    px.gpu_fetch_all()
    arm._target_pose = Pose.create(torch.from_numpy(M["prev_pose"].copy()))
    base.agent.set_action(torch.from_numpy(action))
    got = arm._target_pose.raw_pose.numpy().copy()
    tq = px.cuda_articulation_target_qpos.torch().numpy().copy()
    env.close()
    want = ik.compose(ikspec, M["prev_pose"], action)
    pose_close(got, want, 1.0, f"torch controller {mode}")
    # and its joint targets reach that pose (the batch-wide exit only iterates longer): residual below twice the tolerance
    T = want
    res = [np.abs(ik.pose_error(A, ic.LINK, list(range(7)), tq[e, :7].astype(np.float64), T[e, :3], T[e, 3:], ikspec[2])[0]).max() for e in range(N)]
    assert max(res) < 2e-5, max(res)


# ---------------------------------------------------------------- 5. the surface
@pytest.mark.parametrize("robot", ["panda", "panda_stick"])
@pytest.mark.parametrize("mode", MODES)
def test_fused_action_spec_names_the_ik_block(robot, mode):
    if robot == "panda_stick" and mode == "pd_ee_pose":
        return  # (the stick robot has no absolute pose mode)
    env = _make(mode, 2, robot=robot)
    base = env.unwrapped
    spec = base.agent.controller.fused_action_spec()
    assert spec is not None and len(spec) == 6 and spec[4] is None
    link, c0, rows, m, low, high, rot_scale, flags = spec[5]
    arm = base.agent.controller.controllers["arm"]
    assert link == arm.kinematics.end_link_idx and c0 == 0
    assert rows == (3 if mode.endswith("_pos") else 6) and m == (0 if mode == "pd_ee_pose" else 1)
    if mode != "pd_ee_pose":
        assert flags == 2 and abs(low + 0.1) < 1e-7 and abs(high - 0.1) < 1e-7 and (rows == 3 or abs(rot_scale + 0.1) < 1e-7)
    else:
        assert flags == 0
    assert [j for j, f in enumerate(spec[3]) if f == 4] == arm.kinematics.active_ancestor_joint_idxs
    target = base.agent.controller.fused_ik_target()
    assert target is arm._target_pose.raw_pose and tuple(target.shape) == (2, 7)
    env.close()


def test_fused_action_spec_is_none_for_fetch_and_interpolate():
    env = _make("pd_ee_delta_pos", 2, robot="fetch")
    assert env.unwrapped.agent.controller.fused_action_spec() is None
    env.close()
    env = _make("pd_ee_target_delta_pos", 2)
    arm = env.unwrapped.agent.controller.controllers["arm"]
    assert arm.fused_action_spec() is not None
    arm.config.interpolate = True
    try:
        assert arm.fused_action_spec() is None and env.unwrapped.agent.controller.fused_action_spec() is None
    finally:
        arm.config.interpolate = False
    env.close()


@pytest.mark.parametrize("name", list(ac.MAPS))
def test_fused_action_spec_of_the_existing_maps_is_unchanged(name):
    env_id, kw = ac.env_spec(name)
    env = _make(kw["control_mode"], 2, robot=kw["robot_uids"], env_id=env_id)
    spec = env.unwrapped.agent.controller.fused_action_spec()
    assert isinstance(spec, tuple) and len(spec) == 5 and env.unwrapped.agent.controller.fused_ik_target() is None
    assert (spec[4] is not None) == ("pd_ee_delta" in name)
    env.close()


def test_header_declares_and_native_binds_the_two_symbols():
    from maniskill_amd import native

    text = open(os.path.join(ROOT, "include", "mssim_hip_tasks.h")).read()
    assert re.search(r"int\s+mssim_set_ee_ik_map\s*\(\s*mssim_handle", text) and re.search(r"int\s+mssim_ee_ik_solve\s*\(\s*mssim_handle", text)
    assert "typedef struct mssim_ee_ik_map" in text
    fields = [n for n, _ in native.EeIkMap._fields_]
    assert fields == ["link_index", "column0", "rows", "mode", "low", "high", "rot_scale", "flags", "max_iters", "damping", "max_step", "tolerance"]
    assert callable(native.NativeSim.set_ee_ik_map) and callable(native.NativeSim.ee_ik_solve)
    if os.path.exists(native.NATIVE_LIB_PATH):
        lib = native.NativeLib.load()
        assert lib.set_ee_ik_map is not None and lib.ee_ik_solve is not None


if __name__ == "__main__":
    A, rest = ic.panda_tables()
    for (name, form) in FORMS:
        for rows in ic.ROWS:
            print(f'    ("{name}", "{form}", {rows}): {_measure(A, rest, name, form, rows):.3e},')
