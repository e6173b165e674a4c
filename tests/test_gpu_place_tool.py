"""PlaceSphere-v1 and PullCubeTool-v1 on the HIP backend: the two native epilogues (k_task_place, k_task_pulltool) against the
float64 reference (tests/place_tool_reference.py) on the case tables of tests/place_tool_cases.py, in their two launch forms
(the standalone kernel k_task_*<false> and the one that first copies the state out, k_task_*<true>; these tasks never run at
the control-step kernel's tail), at env counts 128 and the ragged 1, 17, 67; the refusals; the envs with the epilogue against
the same envs on the torch path (MS_FUSED=0) with a partial reset on the way; PullCubeTool on the two-row control step and
PlaceSphere on the one-row one; and both tasks against the oracle.

Flags equal the reference's with no env left out, observation entries (all copies, single subtractions or a flag as 0 / 1)
are bit-exact, rewards and PullCubeTool's three metric columns agree within 4 x the difference measured between the torch
path and the reference on the CPU (MEASURED in tests/place_tool_cases.py). Output tensors carry 8 guard rows that must stay
as they were.

Measured on an MI355X (max |kernel - float64 reference| over the tables, all N and both forms; each test prints its own):
PlaceSphere 8.1e-7 dense (tolerance 3.28e-6), 5.2e-8 normalised (2.76e-7); PullCubeTool 5.9e-7 dense (2.72e-6), 7.1e-8 normalised
(6.0e-7), its metrics 1.7e-7 (7.6e-7). No env is left out anywhere. Against the torch path on the same state over the env
rollouts: rewards within 1.2e-7 (both tasks), info floats within 3.0e-8. Against the oracle over 5 control steps: PlaceSphere
2.6e-5, PullCubeTool 2.2e-7."""
import numpy as np
import pytest
import torch

from tests import oracle_backend as ob
from tests import place_tool_cases as pc
from tests import place_tool_reference as ref

pytestmark = pytest.mark.gpu
BACKEND = "physx_cuda"
GUARD = 8


def _alloc(task, base, N):
    D = 2 * base.agent.robot.max_dof + pc.OBS_EXTRA[task]
    dev = base.device
    out = dict(obs=torch.full((N + GUARD, D), -77.0, device=dev), reward=torch.full((N + GUARD,), -77.0, device=dev),
               flags=torch.full((N + GUARD, pc.N_FLAGS[task]), 0xAB, dtype=torch.uint8, device=dev))
    if task == "tool":
        out["metrics"] = torch.full((N + GUARD, 3), -77.0, device=dev)
    return out


def _fn(task, px):
    return px.task_place_outputs if task == "place" else px.task_pulltool_outputs


def _call(task, base, P, out):
    extra = (out["metrics"],) if task == "tool" else ()
    _fn(task, base.scene.px)(pc.native_task(task, P), out["obs"], out["reward"], out["flags"], *extra)
    torch.cuda.synchronize()


def _read(task, out, N):
    """-> the `got` dict of pc.check; asserts that nothing behind row N was written and that flags are 0 or 1"""
    for k, t in out.items():
        assert bool((t[N:] == (0xAB if t.dtype == torch.uint8 else -77.0)).all()), (task, k, "guard rows written")
    fl = out["flags"][:N].cpu().numpy()
    assert ((fl == 0) | (fl == 1)).all()
    got = dict(obs=out["obs"][:N].cpu().numpy(), reward=out["reward"][:N].cpu().numpy(),
               flags={name: fl[:, i].astype(bool) for i, name in enumerate(pc.FLAG_NAMES[task])})
    if task == "tool":
        got["metrics"] = out["metrics"][:N].cpu().numpy()
    return got


def _report(what, task, P, diff, d_m, excluded):
    tol_r, tol_m = pc.tolerance(task, P)
    print(f"{what}: max |kernel - f64| reward {diff:.3e} (tolerance {tol_r:.3e})" + (f", metrics {d_m:.3e} (tolerance {tol_m:.3e})" if task == "tool" else "")
          + f", {excluded} envs left out")


def _standalone(task, base, S, P, labels, what):
    """k_task_*<false> on the case batch written into the user-visible buffers (nothing owed to the call)"""
    N = base.num_envs
    base.scene._gpu_fetch_all()
    pc.write_buffers(base, S)
    out = _alloc(task, base, N)
    _call(task, base, P, out)
    got = _read(task, out, N)
    R = ref.TASKS[task](S, P)
    diff, d_m, excluded = pc.check(task, got, R, labels, np.inf, np.inf, what=what)
    _report(what, task, P, diff, d_m, excluded)
    pc.check(task, got, R, labels, *pc.tolerance(task, P), what=what)
    assert excluded == 0
    return got, R


def _copy_out(task, base, S, P, labels, what):
    """the case states applied to the simulation, the copy-out owed to the task call: k_task_*<true>; then the standalone
    form on the buffers that launch filled: the same outputs, bit for bit"""
    N = base.num_envs
    px = base.scene.px
    base.scene._gpu_fetch_all()
    pc.write_buffers(base, S)
    base.scene._gpu_apply_all()
    px.gpu_update_articulation_kinematics()
    stale = {**S, "rigid": np.full_like(S["rigid"], 5.0)}
    pc.write_buffers(base, stale)  # (the launch has to refill the buffers)
    t0 = px.tail_step_count()
    px.defer_fetch_all()
    out = _alloc(task, base, N)
    _call(task, base, P, out)
    assert px.tail_step_count() == t0
    got = _read(task, out, N)
    S1 = pc.snapshot(base)
    assert not np.array_equal(S1["rigid"], stale["rigid"]), "the copy-out did not run"
    R = ref.TASKS[task](S1, P)
    diff, d_m, excluded = pc.check(task, got, R, labels, np.inf, np.inf, what=what)
    _report(what, task, P, diff, d_m, excluded)
    pc.check(task, got, R, labels, *pc.tolerance(task, P), what=what)
    assert excluded == 0
    out2 = _alloc(task, base, N)
    _call(task, base, P, out2)
    assert px.tail_step_count() == t0
    got2 = _read(task, out2, N)
    for k in ("obs", "reward") + (("metrics",) if task == "tool" else ()):
        assert np.array_equal(got[k].view(np.uint32), got2[k].view(np.uint32)), (what, k, "differs from the standalone form")
    for name in pc.FLAG_NAMES[task]:
        assert np.array_equal(got["flags"][name], got2["flags"][name]), (what, name)
    return R


@pytest.mark.parametrize("N", [128, 1, 17, 67])
@pytest.mark.parametrize("task", ["place", "tool"])
def test_epilogue_forms_match_reference(task, N, monkeypatch):
    monkeypatch.setenv("MS_FUSED", "1")
    env = pc.make_env(task, N, BACKEND)
    base = env.unwrapped
    start = pc.START_SINGLE[task] if N == 1 else 0  # (a single env: on the bin and grasped / positioned and grasping)
    pc.scripted_grasp(env, task, pc.released_mask(task, pc.params(task, base), N, start))
    tag = f"{task} N={N}"
    S0 = pc.snapshot(base)
    grasped = "is_obj_grasped" if task == "place" else "is_grasped"
    for normalized in (False, True):
        P = pc.params(task, base, normalized=normalized)
        S, labels = pc.build_batch(task, S0, P, start=start)
        got, R = _standalone(task, base, S, P, labels, f"{tag} standalone{' (normalised)' if normalized else ''}")
        F = R["flags"]
        g = F[grasped]
        if N == 1:
            assert g.all() and (F["is_obj_on_bin"] if task == "place" else F["positioned"]).all()
        elif N >= 67:  # the table is complete: every tier of the reward
            assert F["success"].any() and (~F["success"]).any() and g.any() and (~g).any() and (F["left"] != F["right"]).any()
            if task == "place":
                on, ok = F["is_obj_on_bin"], F["success"]
                for sel in (~g & ~on, g & ~on, g & on, ~g & on & ~ok, g & on & ~F["robot_static"], ~g & on & ~F["is_obj_static"] & ~F["robot_static"]):
                    assert sel.any()
            else:
                ok, pos, away = F["success"], F["positioned"], F["pushed_away"]
                for sel in (~g & ~ok, g & ~pos & ~ok, g & pos & ~ok, away & g, away & ~g, ok & g, ok & ~g, ok & g & pos):
                    assert sel.any()
    # the copy-out form: the link rows come from qpos (no finger is turned away, the base link stays; nothing is stepped
    # from here on)
    P = pc.params(task, base)
    S, labels = pc.build_batch(task, S0, P, start=start, link_rows=False)
    Rc = _copy_out(task, base, S, P, labels, f"{tag} copy-out")
    if N >= 17:
        assert Rc["flags"]["success"].any() and (~Rc["flags"]["success"]).any() and Rc["flags"][grasped].any() and (~Rc["flags"][grasped]).any()
    assert base.scene.px.overflow_count() == 0
    env.close()


def test_refusals_launch_nothing(monkeypatch):
    from maniskill_amd import native

    monkeypatch.setenv("MS_FUSED", "1")
    for task in ("place", "tool"):
        env = pc.make_env(task, 4, BACKEND)
        base = env.unwrapped
        px = base.scene.px
        out = _alloc(task, base, 4)
        P = pc.params(task, base)
        extra = (out["metrics"],) if task == "tool" else ()
        call = _fn(task, px)
        obj = "obj_row" if task == "place" else "tool_row"
        for row in (-1, base.scene.model.n_rows):
            with pytest.raises(native.NativeError, match=r"\(1\).*body row out of range"):
                call(pc.native_task(task, {**P, obj: row}), out["obs"], out["reward"], out["flags"], *extra)
        if task == "tool":
            with pytest.raises(native.NativeError, match=r"\(3\).*metrics"):
                call(pc.native_task(task, P), out["obs"], out["reward"], out["flags"], None)
        else:
            for width in (0.0, -0.08):
                with pytest.raises(native.NativeError, match=r"\(3\).*gripper width"):
                    call(pc.native_task(task, dict(P, gripper_width=width)), out["obs"], out["reward"], out["flags"])
        # a second handle of the same model whose buffers were never bound
        with torch.cuda.device(base.device):
            sim = native.NativeSim(px._lib, base.scene.model, 4, px._dev_ordinal)
        ptrs = [t.data_ptr() for t in (out["obs"], out["reward"], out["flags"]) + extra]
        with pytest.raises(native.NativeError, match=r"\(2\).*buffers not bound"):
            getattr(sim, "task_place_outputs" if task == "place" else "task_pulltool_outputs")(pc.native_task(task, P), *ptrs)
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


def _rollout(monkeypatch, env_id, fused, N=ENV_N, steps=ENV_STEPS, reset_at=RESET_AT, **kw):
    """a seeded run with uniform random actions and a partial reset after step `reset_at`. -> per step (obs, reward, terminated,
    info, truncated) as the env returned them; per step the torch path's (obs, reward, success, info) on the very same state;
    how many control steps took the kernel's tail; the overflow count; (n_dof, n_free) of the model"""
    import gymnasium as gym

    g = torch.Generator().manual_seed(3)
    acts = [2 * torch.rand(N, 8, generator=g) - 1 for _ in range(steps)]
    monkeypatch.setenv("MS_FUSED", fused)
    env = gym.make(env_id, num_envs=N, sim_backend=BACKEND, reward_mode="dense", **kw)
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


@pytest.mark.parametrize("task", ["place", "tool"])
def test_env_with_epilogue_matches_torch_path(task, monkeypatch):
    """32 envs, 25 random-action control steps, a partial reset after the 12th: env.step with the native epilogue (the plain
    control step + k_task_*<true>, two launches) against the torch path, step by step.

    As tests/test_gpu_poke_lift.py explains, an MS_FUSED=1 and an MS_FUSED=0 run start an ulp apart in the action map and
    separate once the arm strikes something, so the comparison is made where it can be exact: every step of the MS_FUSED=1 run
    against what the MS_FUSED=0 step computes (get_info, get_obs, get_reward) on that very state: observations bit for bit,
    integer and boolean info equal, rewards and info floats within the kernels' tolerance. The separate MS_FUSED=0 run is
    compared where it can be: the step counter and `truncated` at every step; `terminated`, observations and rewards over
    the first two control steps, within the 1e-5 tests/test_gpu_env.py allows that drift."""
    env_id = pc.ENV_IDS[task]
    fused, same, tail, overflow, (n_dof, n_free) = _rollout(monkeypatch, env_id, "1")
    plain, same_t, tail_t, _, _ = _rollout(monkeypatch, env_id, "0")
    assert tail == 0 and tail_t == 0, "the new tasks never take the control-step kernel's tail"
    assert overflow == 0
    if task == "tool":
        # 9 + 6 + 6 = 21 velocity components: two 16-lane rows per env (mssim_model_pack.h rows_per_env), the plain step
        # mssim_dispatch::plain_step answers for them is k_solve16<9, 0, false, 2>
        assert (n_dof, n_free) == (9, 2) and n_dof + 6 * n_free == 21
    else:
        # 9 + 6 = 15 components: one row, k_solve16<9, 0, false, 1> (the bin is kinematic: no velocity components)
        assert (n_dof, n_free) == (9, 1) and n_dof + 6 * n_free <= 16
    tol, tol_m = 4 * pc.MEASURED[task], 4 * pc.MEASURED["tool_metrics"]
    assert len(fused) == len(same) == len(plain) == ENV_STEPS + 2
    d_rew = max(float((a[1] - b[1]).abs().max()) for a, b in zip(fused, same))
    d_met = max([float((a[3][k] - b[3][k]).abs().max()) for a, b in zip(fused, same) for k in a[3] if a[3][k].dtype.is_floating_point] + [0.0])
    print(f"{env_id}: max |epilogue - torch path on the same state| reward {d_rew:.3e} (tolerance {tol:.3e}), info floats {d_met:.3e} ({tol_m:.3e}); "
          f"two runs: obs after the first step {float((fused[1][0] - plain[1][0]).abs().max()):.3e}, after the last {float((fused[-1][0] - plain[-1][0]).abs().max()):.3e}")
    want_es = torch.zeros(ENV_N, dtype=torch.int64)
    for step, ((o1, r1, t1, i1, tr1), (o2, r2, t2, i2)) in enumerate(zip(fused, same)):
        is_reset = step == 0 or step == RESET_AT + 1
        if step == RESET_AT + 1:
            want_es[list(RESET_IDX)] = 0
        elif step > 0:
            want_es += 1
        assert torch.equal(i1["elapsed_steps"].long(), want_es) and torch.equal(i2["elapsed_steps"].long(), want_es), step
        assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)), (step, float((o1 - o2).abs().max()))
        assert list(i1.keys()) == list(i2.keys()), step
        for k in i1:
            assert i1[k].shape == i2[k].shape and i1[k].dtype == i2[k].dtype, (step, k)
            if i1[k].dtype.is_floating_point:
                assert float((i1[k] - i2[k]).abs().max()) <= tol_m, (step, k)
            else:
                assert torch.equal(i1[k], i2[k]), (step, k)
        if task == "tool":
            assert i1["cube_progress"].dim() == 0 and i1["cube_distance"].dim() == 0 and i1["reward"].shape == (ENV_N,)
        if not is_reset:
            assert torch.equal(t1, t2) and tr1.dtype == torch.bool and not tr1.any(), step
            assert float((r1 - r2).abs().max()) <= tol, (step, float((r1 - r2).abs().max()))
    # the MS_FUSED=0 run itself: the same counters at every step, the same state-dependent outputs while the drift is small
    for step, ((o1, r1, t1, i1, tr1), (o2, r2, t2, i2, tr2)) in enumerate(zip(fused, plain)):
        assert torch.equal(tr1, tr2) and torch.equal(i1["elapsed_steps"], i2["elapsed_steps"]), step
        assert i1.keys() == i2.keys()
        if step <= 2:
            assert torch.equal(t1, t2), step
            assert torch.allclose(o1, o2, atol=1e-5) and torch.allclose(r1, r2, atol=1e-5), (step, float((o1 - o2).abs().max()))


@pytest.mark.parametrize("task", ["place", "tool"])
def test_truncation_at_the_time_limit(task, monkeypatch):
    """a 2-env run on the native path with a limit of 5 steps: `truncated` switches on at step 5, as with MS_FUSED=0"""
    traj, _, tail, _, _ = _rollout(monkeypatch, pc.ENV_IDS[task], "1", N=2, steps=6, reset_at=-1, max_episode_steps=5)
    plain, _, _, _, _ = _rollout(monkeypatch, pc.ENV_IDS[task], "0", N=2, steps=6, reset_at=-1, max_episode_steps=5)
    assert all(torch.equal(a[4], b[4]) and torch.equal(a[3]["elapsed_steps"], b[3]["elapsed_steps"]) for a, b in zip(traj, plain))
    assert not traj[4][4].any() and traj[5][4].all() and traj[6][4].all() and tail == 0
    assert torch.equal(traj[5][3]["elapsed_steps"], torch.full((2,), 5, dtype=traj[5][3]["elapsed_steps"].dtype))


@pytest.mark.parametrize("task", ["place", "tool"])
def test_rollout_matches_oracle_backend(task):
    """64 envs, identical start state, 5 zero-action control steps: obs / reward of the HIP env track the oracle-backed env
    within the bound of the PokeCube oracle test in tests/test_gpu_poke_lift.py (2e-3, that of StackCube's rollout).
    PlaceSphere starts with the sphere resting in the bin (let go just above its bottom plate: a released sphere on the open
    table rolls), PullCubeTool with the hook's inner face against the cube."""
    import gymnasium as gym

    from maniskill_amd.utils.structs.pose import Pose

    ob.register("f64", "oracle_f64_env")
    N = 64
    outs, ref_state = [], None
    for backend in ("oracle_f64_env", BACKEND):
        env = gym.make(pc.ENV_IDS[task], num_envs=N, sim_backend=backend)
        base = env.unwrapped
        env.reset(seed=11)
        if ref_state is None:
            ident = torch.tensor([[1.0, 0, 0, 0]]).expand(N, -1).clone()
            if task == "place":
                p = base.bin.pose.p.clone()
                p[:, 2] = 0.0025 + 0.0025 + 0.02 + 1e-4
                base.obj.set_pose(Pose.create_from_pq(p, ident))
            else:
                # the hook spans x in [0.15, 0.2], y in [0, 0.1] of the tool's frame: the cube in the L's inner corner, 1 mm
                # from the hook's face and clear of the handle
                p = base.l_shape_tool.pose.p.clone() + torch.tensor([[0.15 - 0.02 - 1e-3, 0.06, 0.0]])
                p[:, 2] = 0.02
                base.cube.set_pose(Pose.create_from_pq(p, ident))
            base.scene._gpu_apply_all()
            base.scene._gpu_fetch_all()
            ref_state = {k: {n: v.clone() for n, v in d.items()} for k, d in base.get_state_dict().items()}
        else:
            base.set_state_dict({k: {n: v.to(base.device) for n, v in d.items()} for k, d in ref_state.items()})
            base.agent.controller.reset()
        traj = [base.get_obs().cpu().clone()]
        for _ in range(5):
            obs, rew, *_ = env.step(torch.zeros(N, 8, device=base.device))
            traj.append(obs.cpu().clone())
            traj.append(rew.cpu().clone()[:, None])
        assert base.scene.px.overflow_count() == 0
        outs.append(traj)
        env.close()
    worst = max(float((a - b).abs().max()) for a, b in zip(*outs))
    print(f"{pc.ENV_IDS[task]} HIP against the oracle over 5 control steps: max difference {worst:.3e}")
    for a, b in zip(*outs):
        assert a.shape == b.shape and a.shape[0] == N
        assert torch.allclose(a, b, atol=2e-3), (a - b).abs().max()
