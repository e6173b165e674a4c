"""The iterative-IK block of the HIP library (include/mssim_hip_tasks.h `set_ee_ik_map`, `ee_ik_solve`) against the
float64 reference (tests/ik_reference.py) on the case tables of tests/ik_cases.py, at env counts 128, 1, 17, 67:

  1. the stand-alone solve: tolerance 0 with exactly 1, 2, 5 iterations on *near* and *wide*, and the default settings
     on *near*, within the band measured on the CPU (tests/test_ik_reference.py: 4 x the float32 restatement's largest
     error); `iters_out` equals the reference's count wherever q is compared; a NaN target gives NaN on that env's path
     dofs and nothing else changes by a bit; dofs off the path are q0's bits; inputs are slices of NaN-filled tensors;
  2. the map form: `set_action_map` + `set_ee_ik_map` + `apply_action` for the three modes: the visible targets, the
     simulation's own copy and the in-place target pose; unmapped targets keep their pattern bits; the two
     end-effector blocks remove each other;
  3. batch independence: the first 17 envs of a 128-env run are bit-identical to the 17-env run;
  4. env level: PickCube-v1, 64 envs, 10 seeded steps per mode natively and with MS_FUSED=0; state, partial reset and a
     control-mode switch on the native path.
Nothing is stepped from a non-finite target."""
import numpy as np
import pytest
import torch

import maniskill_amd  # noqa: F401
from maniskill_amd.native import NativeError
from tests import action_cases as ac
from tests import action_reference as ar
from tests import ik_cases as ic
from tests import ik_reference as ik
from tests.test_action_reference import band_k
from tests.test_ik_reference import FORMS, MODES, band, pose_close, reference, settings_of

pytestmark = pytest.mark.gpu
BACKEND = "physx_cuda"
GUARD = 5
MODE_OF_ROWS = {3: "pd_ee_target_delta_pos", 6: "pd_ee_target_delta_pose"}


def _make(env_id, N, mode, robot="panda"):
    import gymnasium as gym

    import maniskill_amd.envs  # noqa: F401

    env = gym.make(env_id, num_envs=N, sim_backend=BACKEND, robot_uids=robot, control_mode=mode)
    env.reset(seed=0)
    return env


def _guarded(x, device):
    """x as rows GUARD .. GUARD + N of a tensor that is NaN everywhere else"""
    N, w = x.shape
    big = torch.full((N + 2 * GUARD, w), float("nan"), dtype=torch.float32, device=device)
    big[GUARD : GUARD + N] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)
    a = big[GUARD : GUARD + N]
    assert a.is_contiguous()
    return a


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _write(base, qpos, pose_buf=None, prev_pose=None):
    """joint positions into the simulation and the visible buffers, the pattern into the targets"""
    px, N, dev = base.scene.px, base.num_envs, base.device
    ptq, ptv = ac.pattern(N, qpos.shape[1])
    px.cuda_articulation_qpos.torch()[:] = torch.from_numpy(qpos).to(dev)
    px.cuda_articulation_qvel.torch()[:] = 0
    px.cuda_articulation_target_qpos.torch()[:] = torch.from_numpy(ptq).to(dev)
    px.cuda_articulation_target_qvel.torch()[:] = torch.from_numpy(ptv).to(dev)
    px.gpu_apply_all()
    px.gpu_update_articulation_kinematics()
    px.gpu_fetch_all()
    if pose_buf is not None:
        pose_buf[:] = torch.from_numpy(prev_pose).to(dev)
    return ptq, ptv


def _targets(px, what):
    """visible target buffers after the launch; the simulation's own copy (fetched) must be the same bits"""
    torch.cuda.synchronize()
    tq, tv = px.cuda_articulation_target_qpos.torch().cpu().numpy().copy(), px.cuda_articulation_target_qvel.torch().cpu().numpy().copy()
    px.gpu_fetch_articulation_target_qpos()
    px.gpu_fetch_articulation_target_qvel()
    torch.cuda.synchronize()
    for got, t in ((tq, px.cuda_articulation_target_qpos), (tv, px.cuda_articulation_target_qvel)):
        assert np.array_equal(_bits(got), _bits(t.torch().cpu().numpy())), f"{what}: visible targets differ from the simulation's"
    return tq, tv


def _solve(px, C, spec, form, dev, q0=True):
    buf = torch.zeros((len(C["q0"]), 7), dtype=torch.float32, device=dev)
    px.set_ee_ik_map(spec[5], buf, **settings_of(form))
    q, iters = px.ee_ik_solve(_guarded(C["target"], dev), _guarded(C["q0"], dev) if q0 else None, return_iters=True)
    torch.cuda.synchronize()
    return q.cpu().numpy(), iters.cpu().numpy()


# ---------------------------------------------------------------- 1. stand-alone solve
@pytest.mark.parametrize("N", ic.ENV_COUNTS)
@pytest.mark.parametrize("rows", ic.ROWS)
def test_stand_alone_solve_matches_reference(rows, N):
    env = _make("Empty-v1", N, MODE_OF_ROWS[rows])
    base = env.unwrapped
    px, dev = base.scene.px, base.device
    A, rest = ic.panda_tables()
    spec = base.agent.controller.fused_action_spec()
    assert spec is not None and spec[5][0] == ic.LINK and spec[5][2] == rows
    px.set_action_map(*spec[:4])
    off = [7, 8]
    for name, form in FORMS:
        what = f"stand-alone {name} {form} rows={rows} N={N}"
        C, R = reference(A, rest, name, form, rows, N)
        q, iters = _solve(px, C, spec, form, dev)
        assert q.dtype == np.float32
        worst = ic.compare(C, R, q, iters, band(name, form, rows), what)
        print(f"{what}: largest |dq| {worst:.3e}, band {band(name, form, rows):.3e}, iterations mean {iters.mean():.2f} max {iters.max()}")
        assert np.array_equal(_bits(q[:, off]), _bits(C["q0"][:, off])), f"{what}: dofs off the path were changed"
        if form != "default":
            assert (iters == int(form[1:])).all()
    # q0 = NULL reads the visible qpos buffer
    C, R = reference(A, rest, "near", "default", rows, N)
    q_explicit, it_explicit = _solve(px, C, spec, "default", dev)
    _write(base, C["q0"])
    q_visible, it_visible = _solve(px, C, spec, "default", dev, q0=False)
    assert np.array_equal(_bits(q_visible), _bits(q_explicit)) and np.array_equal(it_visible, it_explicit)
    # the NaN env: NaN on its seven path dofs, nowhere else; nobody else notices
    Cn, Rn = reference(A, rest, "near", "default", rows, N, nan=True)
    qn, itn = _solve(px, Cn, spec, "default", dev)
    assert np.isnan(qn[N - 1, :7]).all() and np.array_equal(_bits(qn[N - 1, off]), _bits(Cn["q0"][N - 1, off]))
    assert np.array_equal(_bits(qn[: N - 1]), _bits(q_explicit[: N - 1])) and np.array_equal(itn[: N - 1], it_explicit[: N - 1])
    ic.compare(Cn, Rn, qn, itn, band("near", "default", rows), f"NaN env rows={rows} N={N}")
    env.close()


# ---------------------------------------------------------------- 2. map form
def _map_case(base, mode, N, hole):
    """(joint map, ik tuple, case, action): `hole` = the gripper dofs have no column and the action holds the block's columns only"""
    A, rest = ic.panda_tables()
    spec = base.agent.controller.fused_action_spec()
    ikspec = spec[5]
    M = ic.build_map(A, rest, ikspec, N)
    if hole:
        jm = ([-1] * 9, [0.0] * 9, [0.0] * 9, [4] * 7 + [0, 0])
        action = M["columns"].copy()
    else:
        jm = spec[:4]
        action = np.zeros((N, base.agent.controller.single_action_space.shape[0]), np.float32)
        action[:, ikspec[1] : ikspec[1] + ikspec[2]] = M["columns"]
        action[:, -1] = np.linspace(-1.2, 1.2, N)
    return A, jm, ikspec, M, action


def _check_ik_targets(px, A, jm, ikspec, M, action, ptq, ptv, tq, tv, pose_after, what):
    rows, N = ikspec[2], len(action)
    R = ik.apply(ikspec, A, M["q0"], M["prev_pose"], action)
    assert (R["iters"] < 60).all(), f"{what}: the case table must converge"
    pose_close(pose_after, R["pose"], 1.0, what)
    # the solve alone on the pose the launch left behind: the same bits, and its iteration count
    q2, it2 = px.ee_ik_solve(torch.from_numpy(pose_after).to(px.device), torch.from_numpy(M["q0"]).to(px.device), return_iters=True)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(q2.cpu().numpy()[:, :7]), _bits(tq[:, :7])), f"{what}: the map form and the stand-alone solve differ"
    T = R["pose"]
    R["residual"] = lambda e, q: float(np.abs(ik.pose_error(A, ikspec[0], R["path"], np.asarray(q, np.float64)[R["path"]], T[e, :3], T[e, 3:], rows)[0]).max())
    got = M["q0"].copy()
    got[:, :7] = tq[:, :7]
    worst = ic.compare(M, R, got, it2.cpu().numpy(), band("near", "default", rows), what)
    print(f"{what}: largest |dq| {worst:.3e}, band {band('near', 'default', rows):.3e}")
    assert np.array_equal(_bits(tv), _bits(ptv)), f"{what}: velocity targets were written"
    col, lo, hi, fl = jm
    for j in (7, 8):
        if col[j] < 0:
            assert np.array_equal(_bits(tq[:, j]), _bits(ptq[:, j])), f"{what}: target of unmapped dof {j} was written"
        else:
            want = action[:, col[j]].astype(np.float64)
            if fl[j] & 2:
                want = ar.clip_affine(want, float(np.float32(lo[j])), float(np.float32(hi[j])))
            if fl[j] & 1:
                want = want + M["q0"][:, j]
            assert np.abs(tq[:, j] - want).max() <= 4 * ar.EPS32 * max(abs(lo[j]), abs(hi[j]), np.abs(want).max())


@pytest.mark.parametrize("N", ic.ENV_COUNTS)
@pytest.mark.parametrize("mode", MODES)
def test_map_form_matches_reference(mode, N):
    env = _make("Empty-v1", N, mode)
    base = env.unwrapped
    px, dev = base.scene.px, base.device
    hole = N in (17, 67)
    A, jm, ikspec, M, action = _map_case(base, mode, N, hole)
    rows = ikspec[2]
    what = f"map form {mode} N={N}"
    pose_big = torch.full((N + 2 * GUARD, 7), float("nan"), dtype=torch.float32, device=dev)
    pose = pose_big[GUARD : GUARD + N]
    px.set_action_map(*jm)
    px.set_ee_action_map(None)
    px.set_ee_ik_map(ikspec, pose)
    ptq, ptv = _write(base, M["q0"], pose, M["prev_pose"])
    px.apply_action(_guarded(action, dev))
    tq, tv = _targets(px, what)
    pose_after = pose.cpu().numpy().copy()
    assert torch.isnan(pose_big[:GUARD]).all() and torch.isnan(pose_big[GUARD + N :]).all()
    _check_ik_targets(px, A, jm, ikspec, M, action, ptq, ptv, tq, tv, pose_after, what)
    # a short action is refused and nothing is written
    ptq, ptv = _write(base, M["q0"], pose, M["prev_pose"])
    with pytest.raises(NativeError, match="columns"):
        px.apply_action(_guarded(action[:, :-1], dev))  # (hole: the block's last column is missing; else: the gripper's)
    tq_s, tv_s = _targets(px, what)
    assert np.array_equal(_bits(tq_s), _bits(ptq)) and np.array_equal(_bits(pose.cpu().numpy()), _bits(M["prev_pose"]))

    # ---- the two end-effector blocks exclude each other
    if hole and rows == 3:
        # the delta block with 6 rows removes the IK block: the delta map's targets come out, the pose is left alone
        ee = (ikspec[0], 0, 6, -0.1, 0.1, 0.1, 2)
        px.set_ee_action_map(ee)
        a6 = np.concatenate([action, 0.5 * action], 1)
        _write(base, M["q0"], pose, M["prev_pose"])
        px.apply_action(_guarded(a6, dev))
        tq_d, tv_d = _targets(px, what + " delta block")
        assert np.array_equal(_bits(pose.cpu().numpy()), _bits(M["prev_pose"])), "the IK block still ran"
        spec_d = (jm[0], jm[1], jm[2], jm[3], ee)
        C = dict(qpos=M["q0"], prev_tq=ptq, prev_tv=ptv, action=a6, labels=M["labels"], pose_set=np.array(["rest03"] * N))
        Rd = ac.reference(spec_d, A, C)
        ac.compare(spec_d, C, Rd, tq_d, tv_d, band_k(spec_d), what + " delta block")
        with pytest.raises(NativeError, match="columns"):
            px.apply_action(_guarded(action, dev))  # 3 columns: the 6-row block is the one in place
        # and the IK block removes the delta block: 3 columns are enough again, the IK targets come out
        px.set_ee_ik_map(ikspec, pose)
        ptq, ptv = _write(base, M["q0"], pose, M["prev_pose"])
        px.apply_action(_guarded(action, dev))
        tq_i, tv_i = _targets(px, what + " IK block again")
        assert np.array_equal(_bits(tq_i), _bits(tq)) and np.array_equal(_bits(pose.cpu().numpy()), _bits(pose_after))
        # removing the IK block leaves the joint map alone
        px.set_ee_ik_map(None)
        ptq, ptv = _write(base, M["q0"], pose, M["prev_pose"])
        px.apply_action(_guarded(action, dev))
        tq_n, _ = _targets(px, what + " no block")
        assert np.array_equal(_bits(tq_n), _bits(ptq))
    env.close()


def test_set_ee_ik_map_refuses_what_it_cannot_solve():
    env = _make("Empty-v1", 2, "pd_ee_target_delta_pos")
    base = env.unwrapped
    px = base.scene.px
    spec = base.agent.controller.fused_action_spec()
    pose = torch.zeros((2, 7), dtype=torch.float32, device=base.device)
    col, lo, hi, fl = (list(x) for x in spec[:4])
    fl[3] = 0  # a path dof that the joint map does not hand to the block
    px.set_action_map(col, lo, hi, fl)
    with pytest.raises(NativeError, match="flagged 4"):
        px.set_ee_ik_map(spec[5], pose)
    px.set_action_map(*spec[:4])
    with pytest.raises(NativeError, match="rows"):
        px.set_ee_ik_map(spec[5][:2] + (4,) + spec[5][3:], pose)
    px.set_ee_ik_map(spec[5], pose)
    env.close()
    env = _make("Empty-v1", 2, "pd_joint_delta_pos", robot="fetch")
    base = env.unwrapped
    px = base.scene.px
    n = base.scene.model.n_dof
    px.set_action_map([-1] * n, [0.0] * n, [0.0] * n, [4] * n)
    link = base.agent.robot.links.index(base.agent.robot.links_map["gripper_link"])
    with pytest.raises(NativeError, match="at most 8"):
        px.set_ee_ik_map((link, 0, 3, 1, -0.1, 0.1, 0.0, 2), torch.zeros((2, 7), dtype=torch.float32, device=base.device))
    env.close()


# ---------------------------------------------------------------- 3. batch independence
@pytest.mark.parametrize("rows", ic.ROWS)
def test_first_envs_of_a_large_batch_equal_the_small_batch(rows):
    A, rest = ic.panda_tables()
    out = {}
    for N in (128, 17):
        env = _make("Empty-v1", N, MODE_OF_ROWS[rows])
        base = env.unwrapped
        px, dev = base.scene.px, base.device
        spec = base.agent.controller.fused_action_spec()
        px.set_action_map(*spec[:4])
        C = ic.build(A, rest, "wide", rows, N)
        q, iters = _solve(px, C, spec, "default", dev)
        _, jm, ikspec, M, action = _map_case(base, MODE_OF_ROWS[rows], N, True)
        pose = torch.zeros((N, 7), dtype=torch.float32, device=dev)
        px.set_action_map(*jm)
        px.set_ee_ik_map(ikspec, pose)
        _write(base, M["q0"], pose, M["prev_pose"])
        px.apply_action(_guarded(action, dev))
        tq, _ = _targets(px, f"batch independence N={N}")
        out[N] = (q, iters, tq[:, :7], pose.cpu().numpy().copy())
        env.close()
    assert len(set(out[128][1][:17].tolist())) > 2, "the envs must leave the loop at different iterations"
    (q128, it128, tq128, pose128), (q17, it17, tq17, pose17) = out[128], out[17]
    assert np.array_equal(_bits(q128[:17]), _bits(q17)) and np.array_equal(it128[:17], it17)
    assert np.array_equal(_bits(tq128[:17]), _bits(tq17)) and np.array_equal(_bits(pose128[:17]), _bits(pose17))


# ---------------------------------------------------------------- 4. env level
SCALE = 0.3  # of the normalised columns: 3 cm / 0.03 rad per step, so that every env's target stays reachable (the reference converges)


def _env_actions(mode, N, steps, tcp_pose):
    rng = np.random.default_rng([ic.SEED, MODES.index(mode)])
    if mode != "pd_ee_pose":
        rows = 3 if mode.endswith("_pos") else 6
        a = rng.uniform(-1.0, 1.0, (steps, N, rows + 1))
        a[:, :, :rows] *= SCALE
    else:
        # absolute: a seeded reachable pose around the TCP's start, held with small changes
        a = np.zeros((steps, N, 7))
        e0 = ic.quat_to_euler_xyz(ar._unit(tcp_pose[:, 3:].astype(np.float64)))
        for t in range(steps):
            a[t, :, :3] = tcp_pose[:, :3] + 0.03 * rng.uniform(-1.0, 1.0, (N, 3))
            a[t, :, 3:6] = e0 + 0.05 * rng.uniform(-1.0, 1.0, (N, 3))
            a[t, :, 6] = rng.uniform(-1.0, 1.0, N)
    return a.astype(np.float32)


def _run_env(mode, N, steps, fused, monkeypatch):
    monkeypatch.setenv("MS_FUSED", "1" if fused else "0")
    env = _make("PickCube-v1", N, mode)
    base = env.unwrapped
    arm = base.agent.controller.controllers["arm"]
    px = base.scene.px
    acts = _env_actions(mode, N, steps, arm.ee_pose_at_base.raw_pose.cpu().numpy())
    log = []
    for t in range(steps):
        torch.cuda.synchronize()
        pre = dict(qpos=px.cuda_articulation_qpos.torch().cpu().numpy().copy(), pose=arm._target_pose.raw_pose.cpu().numpy().copy())
        a = torch.from_numpy(acts[t]).to(base.device)
        if fused:
            assert base._fused_action_ready(a), "the native IK block is not in use"
        env.step(a)
        torch.cuda.synchronize()
        log.append(dict(pre, action=acts[t], tq=px.cuda_articulation_target_qpos.torch().cpu().numpy().copy(),
                        pose_after=arm._target_pose.raw_pose.cpu().numpy().copy(), state=arm.get_state()))
    return env, log


@pytest.mark.parametrize("mode", MODES)
def test_env_steps_natively_and_agrees_with_the_torch_path(mode, monkeypatch):
    N, steps = 64, 10
    env, native_log = _run_env(mode, N, steps, True, monkeypatch)
    base = env.unwrapped
    A = base.scene.model.arrays
    ikspec = base.agent.controller.fused_action_spec()[5]
    rows = ikspec[2]
    arm = base.agent.controller.controllers["arm"]
    # ---- joint targets and controller state against the reference at the pre-step qpos
    for t, L in enumerate(native_log):
        what = f"env {mode} step {t}"
        R = ik.apply(ikspec, A, L["qpos"], L["pose"], L["action"])
        pose_close(L["pose_after"], R["pose"], 1.0, what)
        if mode != "pd_ee_pose":
            assert np.array_equal(_bits(L["state"]["target_pose"].cpu().numpy()), _bits(L["pose_after"]))
        else:
            assert L["state"] == {}
        T, path = R["pose"], R["path"]
        res = np.array([np.abs(ik.pose_error(A, ikspec[0], path, L["tq"][e, path].astype(np.float64), T[e, :3], T[e, 3:], rows)[0]).max() for e in range(N)])
        dq = np.abs(L["tq"][:, path].astype(np.float64) - R["q"][:, path]).max(1)
        far = dq > band("near", "default", rows)
        print(f"{what}: largest |dq| {dq.max():.3e} (band {band('near', 'default', rows):.3e}), {far.sum()} env(s) compared by residual, reference iterations max {R['iters'].max()}")
        assert (R["iters"] < 60).all(), f"{what}: the action sequence must keep every target reachable"
        assert far.sum() <= 0.02 * N and (res[far] < 2e-5).all(), (what, dq.max(), res[far])
    # ---- state: the same state and action give the same bits
    s, cs = env.get_state_dict(), base.agent.controller.get_state()
    a = torch.from_numpy(native_log[-1]["action"]).to(base.device)
    outs = []
    for _ in range(2):
        env.set_state_dict(s)
        base.agent.controller.set_state(cs)
        env.step(a)
        torch.cuda.synchronize()
        outs.append((base.scene.px.cuda_articulation_target_qpos.torch().cpu().numpy().copy(), arm._target_pose.raw_pose.cpu().numpy().copy()))
    assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0])) and np.array_equal(_bits(outs[0][1]), _bits(outs[1][1]))
    # ---- partial reset of envs {1, 5}. The controller's reset under the mask of those envs sets their target pose to
    # their current end-effector pose and leaves the other rows' bits alone, in the buffer the block is bound to ...
    buf = arm._target_pose.raw_pose
    before = buf.cpu().numpy().copy()
    with base.scene._narrow_reset_mask(torch.tensor([1, 5], device=base.device)):
        base.agent.controller.reset()
    torch.cuda.synchronize()
    after, here = arm._target_pose.raw_pose.cpu().numpy(), arm.ee_pose_at_base.raw_pose.cpu().numpy()
    keep = [e for e in range(N) if e not in (1, 5)]
    assert arm._target_pose.raw_pose.data_ptr() == buf.data_ptr()
    assert np.array_equal(_bits(after[keep]), _bits(before[keep])) and np.array_equal(_bits(after[[1, 5]]), _bits(here[[1, 5]]))
    assert not np.array_equal(_bits(after[[1, 5]]), _bits(before[[1, 5]]))
    # ... and `env.reset(options=dict(env_idx=...))` does what it does on the torch path: it resets the controller under
    # the all-envs mask (sapien_env.py `_reset_selected_envs`, as the reference), so every row becomes the current
    # end-effector pose; the buffer stays the one the block is bound to and the next step runs natively from it
    env.reset(options=dict(env_idx=[1, 5]))
    torch.cuda.synchronize()
    assert arm._target_pose.raw_pose.data_ptr() == buf.data_ptr()
    pose0, qpos0 = arm._target_pose.raw_pose.cpu().numpy().copy(), base.scene.px.cuda_articulation_qpos.torch().cpu().numpy().copy()
    assert np.array_equal(_bits(pose0), _bits(arm.ee_pose_at_base.raw_pose.cpu().numpy()))
    assert base._fused_action_ready(a)
    env.step(a)
    torch.cuda.synchronize()
    R = ik.apply(ikspec, A, qpos0, pose0, native_log[-1]["action"])
    pose_close(arm._target_pose.raw_pose.cpu().numpy(), R["pose"], 1.0, f"{mode} after the partial reset")
    env.close()
    # ---- the torch path (MS_FUSED=0): the same target-pose trajectory
    env, torch_log = _run_env(mode, N, steps, False, monkeypatch)
    env.close()
    for t, (Ln, Lt) in enumerate(zip(native_log, torch_log)):
        pose_close(Ln["pose_after"], Lt["pose_after"], 2.0 * (t + 1), f"{mode} target-pose trajectory step {t}")


def test_control_mode_switch_selects_the_right_block(monkeypatch):
    monkeypatch.setenv("MS_FUSED", "1")
    N = 64
    env = _make("PickCube-v1", N, "pd_ee_target_delta_pos")
    base = env.unwrapped
    px = base.scene.px
    A = base.scene.model.arrays
    rng = np.random.default_rng([ic.SEED, 99])

    def state():
        torch.cuda.synchronize()
        arm = base.agent.controller.controllers["arm"]
        return px.cuda_articulation_qpos.torch().cpu().numpy().copy(), arm.ee_pose_at_base.raw_pose.cpu().numpy().copy()

    def targets():
        torch.cuda.synchronize()
        return px.cuda_articulation_target_qpos.torch().cpu().numpy().copy()

    def check_ik(qpos, pose, action, what):
        ikspec = base.agent.controller.fused_action_spec()[5]
        R = ik.apply(ikspec, A, qpos, pose, action)
        tq = targets()
        dq = np.abs(tq[:, :7].astype(np.float64) - R["q"][:, :7]).max(1)
        far = dq > band("near", "default", 3)
        res = np.array([np.abs(ik.pose_error(A, ikspec[0], R["path"], tq[e, :7].astype(np.float64), R["pose"][e, :3], R["pose"][e, 3:], 3)[0]).max() for e in range(N)])
        assert far.sum() <= 0.02 * N and (res[far] < 2e-5).all(), (what, dq.max())
        arm = base.agent.controller.controllers["arm"]
        pose_close(arm._target_pose.raw_pose.cpu().numpy(), R["pose"], 1.0, what)

    a = (0.6 * rng.uniform(-1, 1, (N, 4))).astype(np.float32)
    qpos, pose = state()
    env.step(torch.from_numpy(a).to(base.device))
    check_ik(qpos, pose, a, "target mode, first")
    # -> pd_ee_delta_pos: the delta block's targets
    qpos, _ = state()
    env.step(dict(control_mode="pd_ee_delta_pos", action=torch.from_numpy(a).to(base.device)))
    spec = base.agent.controller.fused_action_spec()
    assert len(spec) == 5 and spec[4] is not None
    ptq = np.zeros_like(qpos)
    C = dict(qpos=qpos, prev_tq=ptq, prev_tv=ptq, action=a)
    Rd = ac.reference(spec, A, C)
    tq = targets()
    eb = ar.ee_bound(band_k(spec)[0], qpos, Rd, band_k(spec)[1])
    ok = Rd["kappa"] <= ar.KAPPA_CAP
    assert (np.abs(tq[:, :7] - Rd["tq"][:, :7])[ok] <= eb[:, :7][ok]).all(), "the delta block did not produce the targets after the switch"
    # -> back: the IK block again, from the end-effector pose the controller's reset reads
    qpos, pose = state()
    env.step(dict(control_mode="pd_ee_target_delta_pos", action=torch.from_numpy(a).to(base.device)))
    check_ik(qpos, pose, a, "target mode, after switching back")
    env.close()
