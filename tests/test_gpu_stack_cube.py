"""StackCube-v1 on the HIP backend: the native epilogue (k_task_stack, and the tail of the two-row control-step kernel
k_solve16<9, 4, false, 2>) against the torch path, the env against the oracle backend, known answers, a scripted stack
and contact capacity at scale."""
import pytest
import torch

from tests import oracle_backend as ob
from tests.stack_script import run_scripted_stack
from tests.test_stack_cube import check_known_answers

pytestmark = pytest.mark.gpu
BACKEND = "physx_cuda"


def _rollout(monkeypatch, fused, N, n_steps, seed=5):
    """(per step: obs, reward, terminated, info, truncated) of a seeded run with the same uniform random actions,
    and how many control steps ran with the epilogue at the kernel's tail"""
    import gymnasium as gym

    g = torch.Generator().manual_seed(3)
    acts = [2 * torch.rand(N, 8, generator=g) - 1 for _ in range(n_steps)]
    monkeypatch.setenv("MS_FUSED", fused)
    env = gym.make("StackCube-v1", num_envs=N, sim_backend=BACKEND, max_episode_steps=8)  # truncation switches on at step 8
    base = env.unwrapped
    assert base._use_fused_callers == (fused == "1")
    obs, rinfo = env.reset(seed=5)
    if fused == "1":
        assert base._fused_ok() and base._fused_action_ready(acts[0].cuda()), "native action map / epilogue not in use"
        assert base.scene.model.n_dof + 6 * base.scene.model.n_free > 16  # (two 16-lane rows per env)
    tail0 = base.scene.px.tail_step_count()
    z = torch.zeros(N)
    traj = [(obs.cpu().clone(), z, z.bool(), {k: v.cpu().clone() for k, v in rinfo.items() if isinstance(v, torch.Tensor)}, z.bool())]
    for a in acts:
        obs, rew, term, trunc, info = env.step(a.cuda())
        traj.append((obs.cpu().clone(), rew.cpu().clone(), term.cpu().clone(), {k: v.cpu().clone() for k, v in info.items()}, trunc.cpu().clone()))
    tail = base.scene.px.tail_step_count() - tail0
    env.close()
    return traj, tail


def _assert_same(fused, torch_path, tol=1e-5):
    for step, ((o1, r1, t1, i1, tr1), (o2, r2, t2, i2, tr2)) in enumerate(zip(fused, torch_path)):
        assert tr1.dtype == torch.bool and torch.equal(tr1, tr2), step
        assert torch.allclose(o1, o2, atol=tol), (step, (o1 - o2).abs().max())
        assert torch.allclose(r1, r2, atol=tol), (step, (r1 - r2).abs().max())
        assert torch.equal(t1, t2), step
        assert i1.keys() == i2.keys()
        for k in i1:
            if i1[k].dtype.is_floating_point:
                assert torch.allclose(i1[k], i2[k], atol=tol), (step, k)
            else:
                assert torch.equal(i1[k], i2[k]), (step, k)


def test_fused_tail_matches_torch_path(monkeypatch):
    """N = 256: every control step is ONE launch of k_solve16<9, 4, false, 2> (action map, substeps, copy-out over the
    env's 32 lanes, StackCube epilogue on one of them); step outputs equal the torch path's"""
    fused, tail = _rollout(monkeypatch, "1", 256, 12)
    ref, tail_ref = _rollout(monkeypatch, "0", 256, 12)
    assert tail == 12 and tail_ref == 0, (tail, tail_ref)
    _assert_same(fused, ref)


def test_separate_epilogue_launch_matches_torch_path(monkeypatch):
    """N = 16384 is beyond 4 blocks of 8 envs per CU: the control step and k_task_stack<true> (copy-out + epilogue) are
    two launches; the reset's outputs come from k_task_stack<false> (nothing owed)"""
    fused, tail = _rollout(monkeypatch, "1", 16384, 4)
    ref, _ = _rollout(monkeypatch, "0", 16384, 4)
    assert tail == 0
    _assert_same(fused, ref)


def test_env_rollout_matches_oracle_backend():
    """same start state, same actions: obs / reward of the HIP env track the oracle-backed env over the first control
    steps, in every env"""
    import gymnasium as gym

    ob.register("f64", "oracle_f64_env")
    N = 32
    g = torch.Generator().manual_seed(0)
    acts = [2 * torch.rand(N, 8, generator=g) - 1 for _ in range(5)]
    outs, ref_state = [], None
    for backend in ("oracle_f64_env", BACKEND):
        env = gym.make("StackCube-v1", num_envs=N, sim_backend=backend)
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


def test_known_answers():
    """the hand-set stacks of tests/test_stack_cube.py, through the fused epilogue"""
    check_known_answers(BACKEND)


def test_scripted_stack():
    """reach, grasp, lift, carry over B, lower, release, retreat (tests/stack_script.py) in 256 envs with random
    placements. Measured: 254 / 256 envs succeed (oracle backend, 64 envs: 63 / 64); asserted: 85 %."""
    import gymnasium as gym

    N = 256
    env = gym.make("StackCube-v1", num_envs=N, sim_backend=BACKEND, control_mode="pd_ee_delta_pose", max_episode_steps=1000)
    env.reset(seed=0)
    info = run_scripted_stack(env)
    rate = info["success"].float().mean().item()
    print(f"scripted stack: success in {int(info['success'].sum())} / {N} envs")
    assert not info["is_cubeA_grasped"].any()
    assert rate >= 0.85, rate
    env.close()


def test_contact_overflow_is_rare_at_scale():
    """200 uniform random control steps in 4096 envs: at most 1 env in 1000 exceeds a contact capacity (the capacities
    are per env and shared by every instance of the control-step kernel). Measured: 1 env of 4096 (seed 0)."""
    import gymnasium as gym

    N = 4096
    env = gym.make("StackCube-v1", num_envs=N, sim_backend=BACKEND)
    env.reset(seed=0)
    px = env.unwrapped.scene.px
    g = torch.Generator(device="cuda").manual_seed(0)
    for _ in range(200):
        obs, *_ = env.step(2 * torch.rand(N, 8, device="cuda", generator=g) - 1)
    assert torch.isfinite(obs).all()
    reasons = px.read_internal("overflow", 1)[0].int()  # MSSIM_OVERFLOW_* bits per env (include/mssim.h)
    n_over = px.overflow_count()
    assert n_over <= N // 1000, (n_over, torch.unique(reasons[reasons != 0], return_counts=True))
    env.close()
