"""PushT-v1 on the HIP backend: the native epilogue (the tail of the one-row control-step kernel k_solve16<7, 5>, and the
standalone k_task_pusht) against the torch path on the same post-step state, the env against the oracle backend, a known
answer at the goal pose, and contact capacity at scale."""
import pytest
import torch

import maniskill_amd.envs  # noqa: F401  (registers the envs)
from tests import oracle_backend as ob

pytestmark = pytest.mark.gpu
BACKEND = "physx_cuda"


def _torch_outputs(base):
    """the torch path's evaluate / obs / reward and intersection count on the env's current state"""
    info = base.evaluate()
    obs = base.get_obs(info)
    rew = base.get_reward(obs=obs, action=None, info=info)
    return obs, rew, info["success"], base.pseudo_render_intersection_count()


def _compare(base, obs, rew, success, count, tag):
    t_obs, t_rew, t_succ, t_count = _torch_outputs(base)
    area = float(base.goal_area())
    d = (count - t_count).abs()
    assert d.max() <= 2, (tag, d.max())
    assert (d == 0).float().mean() >= 0.99, (tag, (d == 0).float().mean())
    # envs whose torch fraction lies within 2 pixels of the threshold may flip
    edge = ((t_count / area) - base.intersection_thresh).abs() <= 2 / area
    ok = ~edge
    assert torch.equal(success[ok], t_succ[ok]), tag
    assert torch.allclose(obs[ok], t_obs[ok], atol=1e-5), (tag, (obs[ok] - t_obs[ok]).abs().max())
    assert torch.allclose(rew[ok], t_rew[ok], atol=1e-5), (tag, (rew[ok] - t_rew[ok]).abs().max())
    return int(edge.sum())


def _fused_rollout_vs_torch(monkeypatch, N, n_steps, seed=5):
    import gymnasium as gym

    monkeypatch.setenv("MS_FUSED", "1")
    env = gym.make("PushT-v1", num_envs=N, sim_backend=BACKEND)
    base = env.unwrapped
    obs, info = env.reset(seed=seed)
    assert base._fused_ok(), "native epilogue not in use"
    # reset outputs: the standalone kernel (nothing owed, or the copy-out owed by the reset)
    o, r, i = base._fused_step_outputs(None, advance=False)
    assert torch.equal(o, obs)
    _compare(base, o, r, i["success"], base._fused_intersection, "reset")
    g = torch.Generator(device="cuda").manual_seed(seed)
    tail0 = base.scene.px.tail_step_count()
    for step in range(n_steps):
        a = 2 * torch.rand(N, 7, device="cuda", generator=g) - 1
        assert base._fused_action_ready(a)
        obs, rew, term, trunc, info = env.step(a)
        _compare(base, obs, rew, info["success"], base._fused_intersection, step)
        assert torch.equal(term, info["success"])
    tail = base.scene.px.tail_step_count() - tail0
    env.close()
    return tail


def test_fused_tail_matches_torch_path(monkeypatch):
    """N = 256: every control step is ONE launch of k_solve16<7, 5> (action map, substeps, copy-out, PushT epilogue with
    the pseudo-render over the env's 16 lanes)"""
    assert _fused_rollout_vs_torch(monkeypatch, 256, 12) == 12


def test_unfused_run_takes_no_tail(monkeypatch):
    import gymnasium as gym

    monkeypatch.setenv("MS_FUSED", "0")
    env = gym.make("PushT-v1", num_envs=256, sim_backend=BACKEND)
    env.reset(seed=5)
    t0 = env.unwrapped.scene.px.tail_step_count()
    for _ in range(4):
        env.step(2 * torch.rand(256, 7, device="cuda") - 1)
    assert env.unwrapped.scene.px.tail_step_count() == t0
    env.close()


def test_separate_epilogue_launch_matches_torch_path(monkeypatch):
    """N = 8192 is beyond 4 blocks of 16 envs per CU: the control step and k_task_pusht<true> are two launches"""
    assert _fused_rollout_vs_torch(monkeypatch, 8192, 4) == 0


def test_fused_and_unfused_runs_step_the_same_physics(monkeypatch):
    """k_solve16<7, 5> and k_solve16<7, 0> step the same physics: same seed and actions, the same states up to the action
    map, which MS_FUSED=0 computes in torch (the controllers) instead of at the kernel's head (measured: 1.8e-5 after
    6 steps)"""
    import gymnasium as gym

    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("MS_FUSED", fused)
        env = gym.make("PushT-v1", num_envs=64, sim_backend=BACKEND)
        env.reset(seed=3)
        g = torch.Generator(device="cuda").manual_seed(1)
        for _ in range(6):
            obs, *_ = env.step(2 * torch.rand(64, 7, device="cuda", generator=g) - 1)
        outs.append(obs.cpu())
        env.close()
    assert torch.allclose(outs[0], outs[1], atol=1e-4), (outs[0] - outs[1]).abs().max()


def test_env_rollout_matches_oracle_backend():
    """same start state, same actions: obs / reward of the HIP env track the oracle-backed env over the first control
    steps, in every env"""
    import gymnasium as gym

    ob.register("f64", "oracle_f64_env")
    N = 32
    g = torch.Generator().manual_seed(0)
    acts = [2 * torch.rand(N, 7, generator=g) - 1 for _ in range(5)]
    outs, ref_state = [], None
    for backend in ("oracle_f64_env", BACKEND):
        env = gym.make("PushT-v1", num_envs=N, sim_backend=backend)
        env.reset(seed=11)
        if ref_state is None:
            ref_state = {k: {n: v.clone() for n, v in d.items()} for k, d in env.unwrapped.get_state_dict().items()}
        else:
            dev = env.unwrapped.device
            env.unwrapped.set_state_dict({k: {n: v.to(dev) for n, v in d.items()} for k, d in ref_state.items()})
            env.unwrapped.agent.controller.reset()
        traj = [env.unwrapped.get_obs().cpu().clone()]
        for a in acts:
            obs, rew, *_ = env.step(a.to(env.unwrapped.device))
            traj.append(obs.cpu().clone())
            traj.append(rew.cpu().clone()[:, None])
        outs.append(traj)
        env.close()
    for a, b in zip(*outs):
        assert a.shape == b.shape and a.shape[0] == N
        assert torch.allclose(a, b, atol=2e-3), (a - b).abs().max()


def test_tee_at_goal_succeeds_after_zero_action_steps():
    import gymnasium as gym

    from maniskill_amd.utils.structs.pose import Pose

    N = 1024
    env = gym.make("PushT-v1", num_envs=N, sim_backend=BACKEND)
    env.reset(seed=0)
    base = env.unwrapped
    gp = base.goal_tee.pose.raw_pose
    p = gp[:, :3].clone()
    p[:, 2] = 0.021
    base.tee.set_pose(Pose.create_from_pq(p, gp[:, 3:].clone()))
    base.tee.set_linear_velocity(torch.zeros(N, 3, device="cuda"))
    base.tee.set_angular_velocity(torch.zeros(N, 3, device="cuda"))
    base.scene._gpu_apply_all()
    base.scene._gpu_fetch_all()
    a = torch.zeros(N, 7, device="cuda")
    for _ in range(10):
        obs, rew, term, trunc, info = env.step(a)
    rate = info["success"].float().mean().item()
    print(f"tee at goal: success in {int(info['success'].sum())} / {N} envs")
    assert rate >= 0.95, rate
    env.close()


def test_contact_overflow_is_rare_at_scale():
    """200 uniform random control steps in 1024 envs: at most 1 env in 1000 exceeds a contact capacity"""
    import gymnasium as gym

    N = 1024
    env = gym.make("PushT-v1", num_envs=N, sim_backend=BACKEND)
    env.reset(seed=0)
    px = env.unwrapped.scene.px
    g = torch.Generator(device="cuda").manual_seed(0)
    for _ in range(200):
        obs, *_ = env.step(2 * torch.rand(N, 7, device="cuda", generator=g) - 1)
    assert torch.isfinite(obs).all()
    reasons = px.read_internal("overflow", 1)[0].int()
    n_over = px.overflow_count()
    print(f"contact capacity: {n_over} of {N} envs overflowed")
    assert n_over <= N // 1000, (n_over, torch.unique(reasons[reasons != 0], return_counts=True))
    env.close()
