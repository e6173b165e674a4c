"""RollBall-v1 and PullCube-v1 on the HIP backend: the two native epilogues (k_task_roll, k_task_pull) against the float64
reference (tests/roll_pull_reference.py) on the case tables of tests/roll_pull_cases.py, in their two launch forms (the
standalone kernel k_task_*<false> and the one that first copies the state out, k_task_*<true>; these tasks never run at the
control-step kernel's tail), at env counts 128 and the ragged 1, 17, 67; the envs with the epilogue against the same envs
on the torch path; RollBall's latch through a partial reset; and a rolling ball against the oracle and 5/7 v0.

Flags equal the reference's with no env left out, observation entries (all copies or single subtractions) are bit-exact,
rewards agree within 4 x the difference measured between the torch path and the reference on the CPU (MEASURED in
tests/roll_pull_cases.py), the latch equals the reference's.

Measured on an MI355X (max |kernel - float64 reference| of the reward over the tables, all N and both forms; each test
prints its own): RollBall 9.3e-7 dense (tolerance 2.72e-6), 5.2e-8 normalised (2.12e-7); PullCube 1.5e-7 dense (2.88e-7),
3.8e-8 normalised (1.6e-7). No env is left out anywhere."""
import numpy as np
import pytest
import torch

from tests import oracle_backend as ob
from tests import roll_pull_cases as rc
from tests import roll_pull_reference as ref
from tests.test_gpu_stack_cube import _assert_same

pytestmark = pytest.mark.gpu
BACKEND = "physx_cuda"
GUARD = 8


def _alloc(task, base, N):
    D = 2 * base.agent.robot.max_dof + rc.OBS_EXTRA[task]
    dev = base.device
    return dict(obs=torch.full((N + GUARD, D), -77.0, device=dev), reward=torch.full((N + GUARD,), -77.0, device=dev),
                flags=torch.full((N + GUARD, 1), 0xAB, dtype=torch.uint8, device=dev))


def _latch(base, S, N):
    """RollBall's latch of the batch on the device, 8 guard entries behind it"""
    t = torch.full((N + GUARD,), -77.0, device=base.device)
    t[:N] = torch.from_numpy(S["reached"]).to(base.device)
    return t


def _call(task, base, P, out, latch=None):
    px = base.scene.px
    getattr(px, f"task_{task}_outputs")(rc.native_task(task, P, latch), out["obs"], out["reward"], out["flags"])
    torch.cuda.synchronize()


def _read(task, out, N, latch=None):
    """-> the `got` dict of rc.check; asserts that nothing behind row N was written"""
    for k, t in list(out.items()) + ([("reached", latch)] if latch is not None else []):
        assert bool((t[N:] == (0xAB if t.dtype == torch.uint8 else -77.0)).all()), (task, k, "guard rows written")
    fl = out["flags"][:N].cpu().numpy()
    assert ((fl == 0) | (fl == 1)).all()
    got = dict(obs=out["obs"][:N].cpu().numpy(), reward=out["reward"][:N].cpu().numpy(), flags=dict(success=fl[:, 0].astype(bool)))
    if latch is not None:
        got["reached"] = latch[:N].cpu().numpy()
    return got


def _standalone(task, base, S, P, labels, what):
    """k_task_*<false> on the case batch written into the user-visible buffers (nothing owed to the call)"""
    N = base.num_envs
    base.scene._gpu_fetch_all()
    rc.write_buffers(base, S)
    out = _alloc(task, base, N)
    latch = _latch(base, S, N) if task == "roll" else None
    _call(task, base, P, out, latch)
    got = _read(task, out, N, latch)
    R = ref.TASKS[task](S, P)
    diff, excluded = rc.check(task, got, R, labels, rc.tolerance(task, P), what=what)
    print(f"{what}: max |kernel - f64| reward {diff:.3e} (tolerance {rc.tolerance(task, P):.3e}), {excluded} envs left out")
    assert excluded == 0
    return got, R


def _copy_out(task, base, S, P, labels, what):
    """the case states applied to the simulation, the copy-out owed to the task call: k_task_*<true>; then the standalone
    form on the buffers that launch filled: the same outputs, bit for bit"""
    N = base.num_envs
    px = base.scene.px
    base.scene._gpu_fetch_all()
    rc.write_buffers(base, S)
    base.scene._gpu_apply_all()
    px.gpu_update_articulation_kinematics()
    stale = {**S, "rigid": np.full_like(S["rigid"], 5.0)}
    rc.write_buffers(base, stale)  # (the launch has to refill the buffers)
    t0 = px.tail_step_count()
    px.defer_fetch_all()
    out = _alloc(task, base, N)
    latch = _latch(base, S, N) if task == "roll" else None
    _call(task, base, P, out, latch)
    assert px.tail_step_count() == t0
    got = _read(task, out, N, latch)
    S1 = rc.snapshot(base, task)
    assert not np.array_equal(S1["rigid"], stale["rigid"]), "the copy-out did not run"
    S1["reached"] = S.get("reached")
    R = ref.TASKS[task](S1, P)
    diff, excluded = rc.check(task, got, R, labels, rc.tolerance(task, P), what=what)
    print(f"{what}: max |kernel - f64| reward {diff:.3e}, {excluded} envs left out")
    assert excluded == 0
    out2 = _alloc(task, base, N)
    latch2 = _latch(base, S, N) if task == "roll" else None
    _call(task, base, P, out2, latch2)
    got2 = _read(task, out2, N, latch2)
    for k in ("obs", "reward"):
        assert np.array_equal(got[k].view(np.uint32), got2[k].view(np.uint32)), (what, k, "differs from the standalone form")
    assert np.array_equal(got["flags"]["success"], got2["flags"]["success"])
    if task == "roll":
        assert np.array_equal(got["reached"], got2["reached"])
    return R


@pytest.mark.parametrize("N", [128, 1, 17, 67])
@pytest.mark.parametrize("task", ["roll", "pull"])
def test_epilogue_forms_match_reference(task, N, monkeypatch):
    monkeypatch.setenv("MS_FUSED", "1")
    env = rc.make_env(task, N, BACKEND)
    base = env.unwrapped
    tag = f"{task} N={N}"
    S0 = rc.snapshot(base, task)
    start = 1 if N == 1 else 0  # (a single env: RollBall's latch flip, PullCube's pull distance just inside)
    for normalized in (False, True):
        P = rc.params(task, base, normalized=normalized)
        S, labels = rc.build_batch(task, S0, P, start=start)
        got, R = _standalone(task, base, S, P, labels, f"{tag} standalone{' (normalised)' if normalized else ''}")
        if N >= 17:  # the table is complete: every tier of the reward
            lab = np.array(labels)
            assert R["flags"]["success"].any() and (~R["flags"]["success"]).any()
            if task == "roll":
                flip = np.isin(lab, rc.FLIPS)
                assert flip.any() and np.all(S["reached"][flip] == 0) and np.all(got["reached"][flip] == 1)
                assert np.all(got["reached"][~flip] == S["reached"][~flip])
            else:
                for reached in (False, True):
                    for inside in (False, True):
                        assert ((R["flags"]["reached"] == reached) & (R["flags"]["success"] == inside)).any()
    if task == "roll":
        # update_reached = 0 (the outputs of a reset): the latch is read and not written, also where it would flip
        P0 = dict(rc.params(task, base), update_reached=0)
        S, labels = rc.build_batch(task, S0, P0, start=start)
        got, R = _standalone(task, base, S, P0, labels, f"{tag} standalone, update_reached = 0")
        assert np.array_equal(got["reached"].view(np.uint32), S["reached"].view(np.uint32))
        flip = np.isin(np.array(labels), rc.FLIPS)
        assert flip.any() and np.all(R["flags"]["at_hit"][flip]) and np.all(got["reached"][flip] == 0)
    # the copy-out form: the cases that do not write link rows (nothing is stepped from here on)
    P = rc.params(task, base)
    S, labels = rc.build_batch(task, S0, P, start=5 if N == 1 else 0, link_rows=False)
    Rc = _copy_out(task, base, S, P, labels, f"{tag} copy-out")
    if N >= 17:
        assert Rc["flags"]["success"].any() and (~Rc["flags"]["success"]).any()
    env.close()


def test_roll_refuses_a_missing_latch(monkeypatch):
    from maniskill_amd import native

    monkeypatch.setenv("MS_FUSED", "1")
    env = rc.make_env("roll", 4, BACKEND)
    base = env.unwrapped
    out = _alloc("roll", base, 4)
    task = native.RollTask(**rc.params("roll", base), reached=None)
    with pytest.raises(native.NativeError, match=r"\(3\).*reached"):
        base.scene.px.task_roll_outputs(task, out["obs"], out["reward"], out["flags"])
    torch.cuda.synchronize()
    assert bool((out["reward"] == -77.0).all())
    env.close()


# ---------------------------------------------------------------------------------------------------------------------
ENV_N, ENV_STEPS = 67, 10


def _rollout(monkeypatch, env_id, fused):
    """(per step: obs, reward, terminated, info, truncated) of a seeded run with the same uniform random actions, RollBall's
    latch per step, and how many control steps ran with an epilogue at the kernel's tail"""
    import gymnasium as gym

    g = torch.Generator().manual_seed(3)
    acts = [2 * torch.rand(ENV_N, 8, generator=g) - 1 for _ in range(ENV_STEPS)]
    monkeypatch.setenv("MS_FUSED", fused)
    env = gym.make(env_id, num_envs=ENV_N, sim_backend=BACKEND, reward_mode="dense", max_episode_steps=8)  # truncation switches on at step 8
    base = env.unwrapped
    assert base._use_fused_callers == (fused == "1")
    obs, rinfo = env.reset(seed=5)
    if fused == "1":
        assert base._fused_ok() and base._fused_action_ready(acts[0].cuda()), "native action map / epilogue not in use"
    tail0 = base.scene.px.tail_step_count()
    z = torch.zeros(ENV_N)
    latch = lambda: base.reached_status.cpu().clone() if env_id == "RollBall-v1" else z
    traj = [(obs.cpu().clone(), z, z.bool(), {k: v.cpu().clone() for k, v in rinfo.items() if isinstance(v, torch.Tensor)}, z.bool())]
    latches = [latch()]
    for a in acts:
        obs, rew, term, trunc, info = env.step(a.cuda())
        traj.append((obs.cpu().clone(), rew.cpu().clone(), term.cpu().clone(), {k: v.cpu().clone() for k, v in info.items()}, trunc.cpu().clone()))
        latches.append(latch())
    tail = base.scene.px.tail_step_count() - tail0
    env.close()
    return traj, latches, tail


def _undecided(env_id, traj):
    """how many (step, env) pairs have a predicate of the task within 1e-4 of its threshold, from the observations; and the
    smallest distances seen"""
    n_und, min_goal, min_point = 0, np.inf, np.inf
    for obs, *_ in traj:
        o = obs.double()
        tcp, goal, body = o[:, 18:21], o[:, 25:28], o[:, 28:31]
        d_xy = (body[:, :2] - goal[:, :2]).norm(dim=1)
        if env_id == "RollBall-v1":
            away = body - goal
            point, thr = body + away / away.norm(dim=1, keepdim=True) * 0.085, 0.04
        else:
            point, thr = body + torch.tensor([0.03, 0.0, 0.0], dtype=torch.float64), 0.01
        d = (point - tcp).norm(dim=1)
        n_und += int((((d_xy - 0.1).abs() < 1e-4) | ((d - thr).abs() < 1e-4)).sum())
        min_goal, min_point = min(min_goal, float(d_xy.min())), min(min_point, float(d.min()))
    return n_und, min_goal, min_point


@pytest.mark.parametrize("env_id", ["RollBall-v1", "PullCube-v1"])
def test_env_with_epilogue_matches_torch_path(env_id, monkeypatch):
    """N = 67, 10 control steps: env.step with the native epilogue (the plain control step + k_task_*<true>, two launches)
    against the same env on the torch path; truncation switches on at step 8"""
    fused, latch_f, tail = _rollout(monkeypatch, env_id, "1")
    plain, latch_t, tail_t = _rollout(monkeypatch, env_id, "0")
    assert tail == 0 and tail_t == 0, "the new tasks never take the control-step kernel's tail"
    # Every predicate is decided in these steps. RollBall: from a reset the ball lies more than 1 m from the goal and the
    # tcp more than 0.15 m from the hit point (observed on the CPU, oracle backend, same seeds and actions: 1.2568 m and
    # 0.5273 m at the least over the 10 steps). PullCube: the goal lies 0.2 m from the cube, 0.1 m outside its radius, and the
    # tcp 0.516 m from the pull point.
    n_und, min_goal, min_point = _undecided(env_id, plain)
    print(f"{env_id}: min |body - goal|_xy {min_goal:.4f} m, min |tcp - point| {min_point:.4f} m, undecided {n_und}")
    if env_id == "RollBall-v1":
        assert min_goal > 1.0 and min_point > 0.15
    assert n_und == 0, "no env may be left out of the comparison"
    _assert_same(fused, plain)
    for step, (a, b) in enumerate(zip(latch_f, latch_t)):
        assert torch.equal(a, b), (step, "reached_status")
    assert plain[8][4].all() and not plain[7][4].any() and fused[8][4].all()  # truncated from step 8 on
    assert torch.equal(fused[-1][3]["elapsed_steps"], torch.full((ENV_N,), ENV_STEPS, dtype=fused[-1][3]["elapsed_steps"].dtype))


def test_pick_cube_still_takes_the_tail(monkeypatch):
    """a RollBall env and a PickCube env in one process: RollBall's steps leave the tail counter alone, PickCube's step is one
    launch with the epilogue at the kernel's tail"""
    import gymnasium as gym

    monkeypatch.setenv("MS_FUSED", "1")
    roll = gym.make("RollBall-v1", num_envs=ENV_N, sim_backend=BACKEND)
    pick = gym.make("PickCube-v1", num_envs=ENV_N, sim_backend=BACKEND)
    roll.reset(seed=0)
    pick.reset(seed=0)
    a = torch.zeros(ENV_N, 8, device="cuda")
    r0, p0 = roll.unwrapped.scene.px.tail_step_count(), pick.unwrapped.scene.px.tail_step_count()
    roll.step(a)
    pick.step(a)
    roll.step(a)
    torch.cuda.synchronize()
    assert roll.unwrapped.scene.px.tail_step_count() == r0 and pick.unwrapped.scene.px.tail_step_count() == p0 + 1
    roll.close()
    pick.close()


def test_partial_reset_clears_only_its_latches(monkeypatch):
    monkeypatch.setenv("MS_FUSED", "1")
    N = 17
    env = rc.make_env("roll", N, BACKEND)
    base = env.unwrapped
    assert base._fused_ok()
    storage = base.reached_status.data_ptr()
    base.reached_status[:] = 1.0
    idx = torch.tensor([0, 3], device=base.device)
    obs, _ = env.reset(options=dict(env_idx=idx))
    want = torch.ones(N)
    want[[0, 3]] = 0
    assert torch.equal(base.reached_status.cpu(), want) and base.reached_status.data_ptr() == storage
    # a reset's own observation does not move a latch, even with the tcp at the hit point: the tcp row of every env is
    # written there (into the user-visible buffers; nothing is owed) and the reset's outputs are computed again
    P = rc.params("roll", base)
    S, labels = rc.build_batch("roll", rc.snapshot(base, "roll"), P, start=1)
    S["reached"] = want.numpy().copy()  # (the table's states with the reset's latches)
    base.scene._gpu_fetch_all()
    rc.write_buffers(base, S)
    R = ref.roll(S, dict(P, update_reached=0))
    assert (R["flags"]["at_hit"] & (want.numpy() == 0)).any(), "an env whose latch a step would flip"
    obs, info = base._reset_outputs()
    torch.cuda.synchronize()
    assert torch.equal(base.reached_status.cpu(), want)
    assert np.array_equal(obs.cpu().numpy().view(np.uint32), R["obs"].astype(np.float32).view(np.uint32))
    # the step's epilogue does: the same buffers through the epilogue with update_reached = 1
    out = _alloc("roll", base, N)
    _call("roll", base, P, out, base.reached_status)
    assert torch.equal(base.reached_status.cpu(), torch.from_numpy(ref.roll(S, P)["reached_new"]).float())
    env.close()


def test_rolling_ball_matches_oracle_and_closed_form():
    """a ball of radius 0.035 on the table, the arm parked, pushed off at 0.5 m/s along -y without spin: it slips, friction
    spins it up, and it rolls on at 5/7 v0 (a solid sphere). The HIP ball against the f64 oracle env by env, and the oracle
    against the closed form."""
    import gymnasium as gym

    ob.register("f64", "oracle_f64_env")
    N, v0, R_BALL = 8, 0.5, 0.035
    outs, ref_state = [], None
    for backend in ("oracle_f64_env", BACKEND):
        env = gym.make("RollBall-v1", num_envs=N, sim_backend=backend)
        base = env.unwrapped
        env.reset(seed=5)
        dev = base.device
        if ref_state is None:
            ref_state = {k: {n: v.clone() for n, v in d.items()} for k, d in base.get_state_dict().items()}
        else:
            base.set_state_dict({k: {n: v.to(dev) for n, v in d.items()} for k, d in ref_state.items()})
        base.agent.controller.reset()
        base.ball.set_linear_velocity(torch.tensor([0.0, -v0, 0.0], device=dev).repeat(N, 1))
        base.ball.set_angular_velocity(torch.zeros(N, 3, device=dev))
        base.scene._gpu_apply_all()
        base.scene._gpu_fetch_all()
        base.scene.px.wake_all()
        a = torch.zeros(N, 8, device=dev)
        traj = []
        for _ in range(3):
            env.step(a)
            traj.append((base.ball.pose.p.cpu().clone(), base.ball.linear_velocity.cpu().clone(), base.ball.angular_velocity.cpu().clone()))
        outs.append(traj)
        env.close()
    cpu, gpu = outs
    # HIP against the oracle. tests/test_gpu_parity.py (per-env shape types) measured for its rolling sphere a drift of 0.1 mm
    # over the substeps after the landing and asserts 3e-4 m on the position: the same bound here, at every control step.
    for step, ((pc, vc, wc), (pg, vg, wg)) in enumerate(zip(cpu, gpu)):
        perr = (pc - pg).abs().max(dim=1).values
        print(f"control step {step}: max |p_hip - p_oracle| {float(perr.max()):.2e} m, |v| oracle {float(vc.norm(dim=1).mean()):.5f}, hip {float(vg.norm(dim=1).mean()):.5f}")
        assert torch.all(perr < 3e-4), (step, perr)
    # slipping has ended after the first control step on both sides: the contact point's velocity v_y + w_x R vanishes
    for p, v, w in (cpu[0], gpu[0]):
        assert torch.all((v[:, 1] + w[:, 0] * R_BALL).abs() < 1e-3)
        assert torch.all((p[:, 2] - R_BALL).abs() < 1e-4)
    # the oracle against 5/7 v0 right after the slip. Measured on the CPU (oracle f64, these 8 envs): max | |v_y| - 5/7 v0 |
    # = 7.2e-4 m/s after the first control step; asserted with a margin of 2 x
    dev_oracle = (cpu[0][1][:, 1].abs() - 5.0 / 7.0 * v0).abs().max()
    print(f"oracle: | |v_y| - 5/7 v0 | = {float(dev_oracle):.2e} m/s")
    assert dev_oracle < 2 * 7.2e-4
