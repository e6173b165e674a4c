"""PlugCharger-v1 on the HIP backend: the native epilogue k_task_plug against the float64 reference (tests/plug_reference.py)
on the case table of tests/plug_cases.py, in its two launch forms (the standalone kernel k_task_plug<false> and the one that
first copies the state out, k_task_plug<true>; the task never runs at the control-step kernel's tail), at env counts 128
and the ragged 1, 17, 67; the refusals; the env with the epilogue against the same env on the torch path (MS_FUSED=0) with a
partial reset on the way; the physics known answers of tests/test_plug_charger.py on the HIP step; and one control step of
the HIP step against the float64 oracle from the oracle's own inserted state.

Success equals the reference's on every env with none left out, observations (all copies) are bit-exact, the reward is zero,
and the two metric columns agree within 4 x the difference measured between the torch path and the reference on the CPU
(MEASURED in tests/plug_cases.py: 4 x 5.9e-7 = 2.36e-6). Output tensors carry 8 guard rows that must stay as they were.

Measured on an MI355X (each test prints its own): max |kernel - float64 reference| over the table, all N and both forms, dist
1.3e-8 m, angle 2.0e-7 rad (tolerance 2.36e-6). Against the torch path on the same state over the env rollout: info floats within
1.2e-7. After 20 zero-action steps the chargers teleported 0 / 2 / 8 / 12 mm short of the goal are 1.27 / 2.40 / 65.2 / 70.5 mm and
0.080 / 0.078 / 1.571 / 1.571 rad from it. One control step from the f64 oracle's inserted state: |HIP - f64| 5.6e-7 on the
charger's pose, |f32 oracle - f64| 4.5e-7 (bound 1.8e-6)."""
import numpy as np
import pytest
import torch

from tests import oracle_backend as ob
from tests import plug_cases as pc
from tests import plug_reference as ref

pytestmark = pytest.mark.gpu
BACKEND = "physx_cuda"
GUARD = 8


def _alloc(base, N):
    D = 2 * base.agent.robot.max_dof + pc.OBS_EXTRA
    dev = base.device
    return dict(obs=torch.full((N + GUARD, D), -77.0, device=dev), reward=torch.full((N + GUARD,), -77.0, device=dev),
                flags=torch.full((N + GUARD, 1), 0xAB, dtype=torch.uint8, device=dev), metrics=torch.full((N + GUARD, 2), -77.0, device=dev))


def _call(base, P, out):
    base.scene.px.task_plug_outputs(pc.native_task(P, base._goal_pose_raw), out["obs"], out["reward"], out["flags"], out["metrics"])
    torch.cuda.synchronize()


def _read(out, N):
    """-> the `got` dict of pc.check; asserts that nothing behind row N was written and that flags are 0 or 1"""
    for k, t in out.items():
        assert bool((t[N:] == (0xAB if t.dtype == torch.uint8 else -77.0)).all()), (k, "guard rows written")
    fl = out["flags"][:N].cpu().numpy()
    assert ((fl == 0) | (fl == 1)).all()
    return dict(obs=out["obs"][:N].cpu().numpy(), reward=out["reward"][:N].cpu().numpy(), success=fl[:, 0].astype(bool), metrics=out["metrics"][:N].cpu().numpy())


def _standalone(base, S, P, labels, what):
    """k_task_plug<false> on the case batch written into the user-visible buffers (nothing owed to the call)"""
    N = base.num_envs
    base.scene._gpu_fetch_all()
    pc.write_buffers(base, S)
    out = _alloc(base, N)
    _call(base, P, out)
    got = _read(out, N)
    R = ref.outputs(S, P)
    pc.check_margins(R, labels)
    d_dist, d_angle = pc.check(got, R, labels, np.inf, what)
    print(f"{what}: max |kernel - f64| dist {d_dist:.3e}, angle {d_angle:.3e} (tolerance {pc.tolerance():.3e})")
    pc.check(got, R, labels, pc.tolerance(), what)
    return got, R


def _copy_out(base, S, P, labels, what):
    """the case states applied to the simulation, the copy-out owed to the task call: k_task_plug<true>; then the standalone
    form on the buffers that launch filled: the same outputs, bit for bit"""
    N = base.num_envs
    px = base.scene.px
    base.scene._gpu_fetch_all()
    pc.write_buffers(base, S)
    base.scene._gpu_apply_all()
    px.gpu_update_articulation_kinematics()
    stale = {**S, "rigid": np.full_like(S["rigid"], 5.0)}
    pc.write_buffers(base, stale)  # (the launch has to refill the buffers; the stored goal is the env's, not the simulation's)
    t0 = px.tail_step_count()
    px.defer_fetch_all()
    out = _alloc(base, N)
    _call(base, P, out)
    assert px.tail_step_count() == t0
    got = _read(out, N)
    S1 = pc.snapshot(base)
    assert not np.array_equal(S1["rigid"], stale["rigid"]), "the copy-out did not run"
    R = ref.outputs(S1, P)
    d_dist, d_angle = pc.check(got, R, labels, np.inf, what)
    print(f"{what}: max |kernel - f64| dist {d_dist:.3e}, angle {d_angle:.3e} (tolerance {pc.tolerance():.3e})")
    pc.check(got, R, labels, pc.tolerance(), what)
    out2 = _alloc(base, N)
    _call(base, P, out2)
    assert px.tail_step_count() == t0
    got2 = _read(out2, N)
    for k in ("obs", "reward", "metrics"):
        assert np.array_equal(got[k].view(np.uint32), got2[k].view(np.uint32)), (what, k, "differs from the standalone form")
    assert np.array_equal(got["success"], got2["success"]), what
    return R


@pytest.mark.parametrize("N", [128, 1, 17, 67])
def test_epilogue_forms_match_reference(N, monkeypatch):
    monkeypatch.setenv("MS_FUSED", "1")
    env = pc.make_env(N, BACKEND)
    base = env.unwrapped
    P = pc.params(base)
    S0 = pc.snapshot(base)
    S, labels = pc.build_batch(S0, P)
    got, R = _standalone(base, S, P, labels, f"plug N={N} standalone")
    if N >= 67:  # the table is complete: all four combinations of the two predicates, the NaN pose in one env alone
        d_ok, a_ok = R["dist_ok"], R["angle_ok"]
        for sel in (d_ok & a_ok, d_ok & ~a_ok, ~d_ok & a_ok, ~d_ok & ~a_ok):
            assert sel.any()
        assert set(labels) == set(pc.LABELS)
    if N > pc.NAN_CASE:
        assert labels.count("nan pose") == 1 and np.isnan(got["metrics"][pc.NAN_CASE]).all() and not got["success"][pc.NAN_CASE]
        assert np.isfinite(np.delete(got["metrics"], pc.NAN_CASE, 0)).all()
    # the copy-out form: the states go through the simulation (the poses are re-read, the reference is evaluated on what the
    # launch copied out). No NaN enters the simulation state: here the NaN pose of env NAN_CASE is its stored goal's.
    S, labels = pc.build_batch(S0, P, nan="goal")
    Rc = _copy_out(base, S, P, labels, f"plug N={N} copy-out")
    if N > pc.NAN_CASE:
        assert np.isnan(Rc["metrics"][pc.NAN_CASE]).all() and not Rc["success"][pc.NAN_CASE]
    if N >= 17:
        assert Rc["success"].any() and (~Rc["success"]).any()
    assert base.scene.px.overflow_count() == 0
    env.close()


def test_refusals_launch_nothing(monkeypatch):
    from maniskill_amd import native

    monkeypatch.setenv("MS_FUSED", "1")
    env = pc.make_env(4, BACKEND)
    base = env.unwrapped
    px = base.scene.px
    out = _alloc(base, 4)
    P = pc.params(base)
    goal = base._goal_pose_raw
    args = (out["obs"], out["reward"], out["flags"])
    for row in (-1, base.scene.model.n_rows):
        with pytest.raises(native.NativeError, match=r"\(1\).*body row out of range"):
            px.task_plug_outputs(pc.native_task({**P, "charger_row": row}, goal), *args, out["metrics"])
    with pytest.raises(native.NativeError, match=r"\(3\).*metrics"):
        px.task_plug_outputs(pc.native_task(P, goal), *args, None)
    with pytest.raises(native.NativeError, match=r"\(3\).*goal poses"):
        px.task_plug_outputs(native.PlugTask(goal_pose=None, **P), *args, out["metrics"])
    # a second handle of the same model whose buffers were never bound
    with torch.cuda.device(base.device):
        sim = native.NativeSim(px._lib, base.scene.model, 4, px._dev_ordinal)
    with pytest.raises(native.NativeError, match=r"\(2\).*buffers not bound"):
        sim.task_plug_outputs(pc.native_task(P, goal), *[t.data_ptr() for t in args + (out["metrics"],)])
    sim.close()
    torch.cuda.synchronize()
    assert all(bool((t == (0xAB if t.dtype == torch.uint8 else -77.0)).all()) for t in out.values())
    env.close()


# ---------------------------------------------------------------------------------------------------------------------
ENV_N, ENV_STEPS, RESET_AT = 32, 25, 12
RESET_IDX = (1, 5, ENV_N - 1)


def _keep(d):
    return {k: v.cpu().clone() for k, v in d.items() if isinstance(v, torch.Tensor)}


def _torch_path(base, action):
    """what the env's step computes with MS_FUSED=0, on the state the env is in: get_info, get_obs, get_reward"""
    info = base.get_info()
    obs = base.get_obs(info)
    rew = base.get_reward(obs=obs, action=action, info=info) if action is not None else torch.zeros(base.num_envs)
    return obs.cpu().clone(), rew.cpu().clone(), info["success"].cpu().clone(), _keep(info)


def _rollout(monkeypatch, fused, N=ENV_N, steps=ENV_STEPS, reset_at=RESET_AT, **kw):
    """a seeded run with uniform random actions and a partial reset after step `reset_at` (tests/test_gpu_place_tool.py
    `_rollout`). -> per step (obs, reward, terminated, info, truncated) as the env returned them; per step the torch path's
    (obs, reward, success, info) on the very same state; the tail steps taken; the overflow count; (n_dof, n_free)"""
    import maniskill_amd.envs  # noqa: F401
    import gymnasium as gym

    g = torch.Generator().manual_seed(3)
    acts = [2 * torch.rand(N, 8, generator=g) - 1 for _ in range(steps)]
    monkeypatch.setenv("MS_FUSED", fused)
    env = gym.make(pc.ENV_ID, num_envs=N, sim_backend=BACKEND, reward_mode="dense", **kw)
    base = env.unwrapped
    assert base._use_fused_callers == (fused == "1")
    obs, rinfo = env.reset(seed=5)
    if fused == "1":
        assert base._fused_ok() and base._fused_action_ready(acts[0].cuda()), "native action map / epilogue not in use"
    px = base.scene.px
    tail0 = px.tail_step_count()
    px.overflow_count()
    z = torch.zeros(N)
    traj = [(obs.cpu().clone(), z, z.bool(), _keep(rinfo), z.bool())]
    same = [_torch_path(base, None)]
    for i, a in enumerate(acts):
        obs, rew, term, trunc, info = env.step(a.cuda())
        traj.append((obs.cpu().clone(), rew.cpu().clone(), term.cpu().clone(), _keep(info), trunc.cpu().clone()))
        same.append(_torch_path(base, a.cuda()))
        if i + 1 == reset_at:
            obs, rinfo = env.reset(options=dict(env_idx=torch.tensor(RESET_IDX, device=base.device)))
            traj.append((obs.cpu().clone(), z, z.bool(), _keep(rinfo), z.bool()))
            same.append(_torch_path(base, None))
    tail, overflow = px.tail_step_count() - tail0, px.overflow_count()
    model = base.scene.model
    env.close()
    return traj, same, tail, overflow, (int(model.n_dof), int(model.n_free))


def test_env_with_epilogue_matches_torch_path(monkeypatch):
    """32 envs, 25 random-action control steps, a partial reset after the 12th: env.step with the native epilogue (the plain
    one-row control step + k_task_plug<true>, two launches) against what the MS_FUSED=0 step computes (get_info, get_obs,
    get_reward) on that very state: observations bit for bit, integer and boolean info equal, the two info floats within the
    kernel's tolerance. The separate MS_FUSED=0 run is compared where it can be (tests/test_gpu_place_tool.py explains why):
    the step counter and `truncated` at every step; `terminated` and observations over the first two control steps."""
    fused, same, tail, overflow, (n_dof, n_free) = _rollout(monkeypatch, "1")
    plain, _, tail_t, _, _ = _rollout(monkeypatch, "0")
    assert tail == 0 and tail_t == 0, "PlugCharger never takes the control-step kernel's tail"
    assert overflow == 0
    # 9 + 6 = 15 velocity components: one row, k_solve16<9, 0, false, 1> (the receptacle is kinematic)
    assert (n_dof, n_free) == (9, 1)
    tol = pc.tolerance()
    assert len(fused) == len(same) == len(plain) == ENV_STEPS + 2
    d_met = max(float((a[3][k] - b[3][k]).abs().max()) for a, b in zip(fused, same) for k in a[3] if a[3][k].dtype.is_floating_point)
    print(f"PlugCharger-v1: max |epilogue - torch path on the same state| info floats {d_met:.3e} (tolerance {tol:.3e}); two runs: obs after the first step "
          f"{float((fused[1][0] - plain[1][0]).abs().max()):.3e}, after the last {float((fused[-1][0] - plain[-1][0]).abs().max()):.3e}")
    want_es = torch.zeros(ENV_N, dtype=torch.int64)
    for step, ((o1, r1, t1, i1, tr1), (o2, r2, t2, i2)) in enumerate(zip(fused, same)):
        is_reset = step == 0 or step == RESET_AT + 1
        if step == RESET_AT + 1:
            want_es[list(RESET_IDX)] = 0
        elif step > 0:
            want_es += 1
        assert torch.equal(i1["elapsed_steps"].long(), want_es) and torch.equal(i2["elapsed_steps"].long(), want_es), step
        assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)), (step, float((o1 - o2).abs().max()))
        assert list(i1.keys()) == list(i2.keys()) == ["elapsed_steps", "obj_to_goal_dist", "obj_to_goal_angle", "success"], step
        for k in i1:
            assert i1[k].shape == i2[k].shape and i1[k].dtype == i2[k].dtype, (step, k)
            if i1[k].dtype.is_floating_point:
                assert float((i1[k] - i2[k]).abs().max()) <= tol, (step, k, float((i1[k] - i2[k]).abs().max()))
            else:
                assert torch.equal(i1[k], i2[k]), (step, k)
        if not is_reset:
            assert torch.equal(t1, t2) and torch.equal(t1, i1["success"]) and tr1.dtype == torch.bool and not tr1.any(), step
            assert torch.all(r1 == 0) and torch.all(r2 == 0), step
    for step, ((o1, r1, t1, i1, tr1), (o2, r2, t2, i2, tr2)) in enumerate(zip(fused, plain)):
        assert torch.equal(tr1, tr2) and torch.equal(i1["elapsed_steps"], i2["elapsed_steps"]), step
        assert i1.keys() == i2.keys()
        if step <= 2:
            assert torch.equal(t1, t2), step
            assert torch.allclose(o1, o2, atol=1e-5), (step, float((o1 - o2).abs().max()))


def test_truncation_at_the_time_limit(monkeypatch):
    """a 2-env run on the native path with a limit of 5 steps: `truncated` switches on at step 5, as with MS_FUSED=0"""
    traj, _, tail, _, _ = _rollout(monkeypatch, "1", N=2, steps=6, reset_at=-1, max_episode_steps=5)
    plain, _, _, _, _ = _rollout(monkeypatch, "0", N=2, steps=6, reset_at=-1, max_episode_steps=5)
    assert all(torch.equal(a[4], b[4]) and torch.equal(a[3]["elapsed_steps"], b[3]["elapsed_steps"]) for a, b in zip(traj, plain))
    assert not traj[4][4].any() and traj[5][4].all() and traj[6][4].all() and tail == 0


# ---- physics ---------------------------------------------------------------------------------------------------------------
def _make(N, backend, seed=3):
    import maniskill_amd.envs  # noqa: F401
    import gymnasium as gym

    env = gym.make(pc.ENV_ID, num_envs=N, sim_backend=backend)
    env.reset(seed=seed)
    return env


def test_charger_rests_on_the_table():
    N = 4
    env = _make(N, BACKEND)
    base = env.unwrapped
    c0 = base.charger.pose.raw_pose.clone()
    base.scene.px.overflow_count()
    for _ in range(10):
        _, _, _, _, info = env.step(torch.zeros(N, 8, device=base.device))
    c = base.charger.pose.raw_pose
    assert torch.allclose(c[:, 2], torch.full((N,), 0.012, device=base.device), atol=2e-4) and torch.allclose(c[:, :2], c0[:, :2], atol=1e-3)
    assert torch.allclose(c[:, 3:], c0[:, 3:], atol=2e-3)
    assert float(torch.linalg.norm(base.charger.linear_velocity, dim=1).max()) < 1e-2 and not info["success"].any()
    assert base.scene.px.overflow_count() == 0
    env.close()


def test_pegs_hold_an_inserted_charger_and_a_short_one_tips_out():
    """the known answers of tests/test_plug_charger.py on the HIP step: 1.5 mm pegs in slots with 0.5 mm clearance per side"""
    env = _make(len(pc.SHORT), BACKEND)
    pc.teleport_short_of_goal(env.unwrapped)
    dist, angle = pc.check_plugged_rollout(env)
    assert float(dist[2]) > 0.06 and float(dist[3]) > 0.06 and abs(float(angle[2]) - np.pi / 2) < 0.05 and abs(float(angle[3]) - np.pi / 2) < 0.05
    env.close()


# max |f32 oracle - f64 oracle| over the charger's pose after the one control step below, measured on the CPU (4.47e-7: the
# quaternion; 7.5e-9 on the position). The test measures it again and prints it.
F32_ORACLE_STEP = 4.5e-7


def test_one_step_from_the_inserted_state_matches_oracle():
    """The float64 oracle settles two chargers at the goal and two 2 mm short of it (20 zero-action control steps). From that
    state, loaded into each backend, one more zero-action control step: the charger's pose on HIP lies within 4 x the
    difference between the float32 and the float64 oracle, the two being the same algorithm in two precisions."""
    ob.register("f64", "oracle_f64_env")
    ob.register("f32", "oracle_f32_env")
    N = 4
    env = _make(N, "oracle_f64_env")
    base = env.unwrapped
    pc.teleport_short_of_goal(base, (0.0, 2e-3, 0.0, 2e-3))
    for _ in range(20):
        _, _, _, _, info = env.step(torch.zeros(N, 8))
    assert info["success"].all()
    state = {k: {n: v.clone() for n, v in d.items()} for k, d in base.get_state_dict().items()}
    env.close()
    poses = {}
    for backend in ("oracle_f64_env", "oracle_f32_env", BACKEND):
        env = _make(N, backend)
        base = env.unwrapped
        base.set_state_dict({k: {n: v.to(base.device) for n, v in d.items()} for k, d in state.items()})
        base.agent.controller.reset()
        env.step(torch.zeros(N, 8, device=base.device))
        poses[backend] = base.charger.pose.raw_pose.cpu().clone()
        assert base.scene.px.overflow_count() == 0
        env.close()
    d32 = float((poses["oracle_f32_env"] - poses["oracle_f64_env"]).abs().max())
    dhip = float((poses[BACKEND] - poses["oracle_f64_env"]).abs().max())
    print(f"one control step from the inserted state: |f32 oracle - f64| {d32:.3e} (recorded {F32_ORACLE_STEP:.3e}), |HIP - f64| {dhip:.3e} "
          f"(bound {4 * F32_ORACLE_STEP:.3e})")
    assert dhip <= 4 * F32_ORACLE_STEP, (dhip, d32)
