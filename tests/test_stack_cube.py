"""StackCube-v1 on CPU: the env layer driven by the oracle registered as a test backend (as tests/test_env_surface.py
does). The same known answers run on the HIP backend in tests/test_gpu_stack_cube.py."""
import math

import pytest
import torch

from tests import env_checks as ec
from tests import oracle_backend as ob

BACKEND = "oracle_f64_env"
# the placement sampler's radius per cube (stack_cube.py: |(0.02, 0.02)| + 1 mm); two centres are kept 2 radii apart
SAMPLER_RADIUS = math.sqrt(2) * 0.02 + 0.001


@pytest.fixture(scope="module", autouse=True)
def _register():
    ob.register("f64", BACKEND)


def set_stack_state(env, offset_a):
    """cube B at a fixed spot of every env, cube A at B + offset_a (both axis-aligned, at rest), the arm in its rest pose
    with the gripper open -- the TCP ~15 cm above the cubes and 25 cm away"""
    from maniskill_amd.utils.structs.pose import Pose

    base = env.unwrapped
    dev = base.device
    N = base.num_envs
    pb = torch.tensor([0.1, 0.2, 0.02], device=dev).repeat(N, 1)
    pa = pb + torch.as_tensor(offset_a, dtype=torch.float32, device=dev)
    q = torch.tensor([[1.0, 0, 0, 0]], device=dev).repeat(N, 1)
    base.cubeB.set_pose(Pose.create_from_pq(pb, q))
    base.cubeA.set_pose(Pose.create_from_pq(pa, q))
    for cube in (base.cubeA, base.cubeB):
        cube.set_linear_velocity(torch.zeros(N, 3, device=dev))
        cube.set_angular_velocity(torch.zeros(N, 3, device=dev))
    robot = base.agent.robot
    rest = torch.tensor([0.0, math.pi / 8, 0, -math.pi * 5 / 8, 0, math.pi * 3 / 4, math.pi / 4, 0.04, 0.04], device=dev)
    robot.set_qpos(rest.repeat(N, 1))
    robot.set_qvel(torch.zeros(N, 9, device=dev))
    base.scene._gpu_apply_all()
    base.scene.px.gpu_update_articulation_kinematics()
    base.scene._gpu_fetch_all()
    base.agent.controller.reset()


def known_answer(sim_backend, offset_a, reward_mode="dense", steps=5, N=4):
    """a few zero-action steps (pd_joint_delta_pos: hold the arm; gripper action +1: open) from a hand-set state"""
    env = ec.make("StackCube-v1", N, sim_backend, robot_uids="panda", reward_mode=reward_mode)
    env.reset(seed=0)
    set_stack_state(env, offset_a)
    dev = env.unwrapped.device
    a = torch.zeros(N, 8, device=dev)
    a[:, 7] = 1.0
    for _ in range(steps):
        obs, rew, term, trunc, info = env.step(a)
    out = dict(rew=rew.cpu(), term=term.cpu(), info={k: v.cpu() for k, v in info.items()}, cubeA=env.unwrapped.cubeA.pose.p.cpu(),
               cubeB=env.unwrapped.cubeB.pose.p.cpu())
    env.close()
    return out


def check_known_answers(sim_backend):
    # A resting centred on B: on, static, not grasped -> success, the top tier of the reward
    r = known_answer(sim_backend, [0.0, 0.0, 0.04])
    i = r["info"]
    assert i["is_cubeA_on_cubeB"].all() and i["is_cubeA_static"].all() and not i["is_cubeA_grasped"].any(), i
    assert i["success"].all() and r["term"].all()
    assert torch.allclose(r["rew"], torch.full_like(r["rew"], 8.0))
    r = known_answer(sim_backend, [0.0, 0.0, 0.04], reward_mode="normalized_dense")
    assert torch.allclose(r["rew"], torch.ones_like(r["rew"]))
    # A stacked 1 cm off centre: still on B -- the reference's tolerance is |dxy| <= |half_xy| + 5 mm = 3.3 cm
    r = known_answer(sim_backend, [0.01, 0.0, 0.04])
    assert r["info"]["is_cubeA_on_cubeB"].all() and r["info"]["success"].all()
    # A on the table, against B's side (dxy = 4 cm) or apart from it: not on B, no success; the reward is the reach tier
    for off in ([0.04, 0.0, 0.0], [0.0, -0.1, 0.0]):
        r = known_answer(sim_backend, off)
        i = r["info"]
        assert not i["is_cubeA_on_cubeB"].any() and not i["success"].any() and not r["term"].any(), (off, i)
        assert torch.all(r["rew"] < 2.0) and torch.all(r["rew"] > 0.0)
        assert torch.all((r["cubeA"][:, 2] - 0.02).abs() < 2e-3)  # (still lying on the table)


def test_registered_and_shapes():
    N = 8
    env = ec.make("StackCube-v1", N, BACKEND)
    base = env.unwrapped
    assert base.robot_uids == "panda_wristcam"  # the reference's default robot
    assert env.spec.max_episode_steps == 50
    obs, info = env.reset(seed=0)
    assert obs.shape == (N, 48) and obs.dtype == torch.float32  # 9 + 9 + 3 x 7 + 3 x 3
    assert base.single_action_space.shape == (8,)
    for _ in range(3):
        obs, rew, term, trunc, info = env.step(torch.from_numpy(base.action_space.sample()))
    assert obs.shape == (N, 48) and rew.shape == (N,) and torch.isfinite(obs).all() and torch.isfinite(rew).all()
    for k in ("is_cubeA_grasped", "is_cubeA_on_cubeB", "is_cubeA_static", "success", "elapsed_steps"):
        assert k in info and info[k].shape == (N,), k
    assert info["success"].dtype == torch.bool and torch.all(info["elapsed_steps"] == 3)
    # obs layout: the extras follow qpos / qvel in the order of _get_obs_extra
    tcp, a, b = base.agent.tcp.pose, base.cubeA.pose, base.cubeB.pose
    o = obs.cpu()
    assert torch.allclose(o[:, 18:25], tcp.raw_pose.cpu(), atol=1e-6)
    assert torch.allclose(o[:, 25:32], a.raw_pose.cpu(), atol=1e-6)
    assert torch.allclose(o[:, 32:39], b.raw_pose.cpu(), atol=1e-6)
    assert torch.allclose(o[:, 45:48], (b.p - a.p).cpu(), atol=1e-6)
    env.close()


def test_mani_skill_alias_exports_the_class():
    from mani_skill.envs.tasks.tabletop import StackCubeEnv
    from maniskill_amd.envs.tasks.tabletop.stack_cube import StackCubeEnv as Local

    assert StackCubeEnv is Local


def test_plain_panda():
    """(the Fetch is listed as in the reference, but the table scene of this build initialises Pandas only)"""
    env = ec.make("StackCube-v1", 2, BACKEND, robot_uids="panda")
    obs, _ = env.reset(seed=1)
    n = env.unwrapped.agent.robot.max_dof
    assert obs.shape == (2, 2 * n + 30)
    obs, rew, *_ = env.step(torch.from_numpy(env.unwrapped.action_space.sample()))
    assert torch.isfinite(obs).all() and torch.isfinite(rew).all()
    env.close()


def test_seeded_reset_determinism():
    N = 4
    env = ec.make("StackCube-v1", N, BACKEND)
    base = env.unwrapped
    o1, _ = env.reset(seed=7)
    acts = [torch.from_numpy(base.action_space.sample()) for _ in range(4)]
    r1 = [env.step(a)[0].clone() for a in acts]
    o2, _ = env.reset(seed=7)
    r2 = [env.step(a)[0].clone() for a in acts]
    ec.assert_obs_equal(o1, o2, atol=0.0)
    for a, b in zip(r1, r2):
        ec.assert_obs_equal(a, b, atol=0.0)
    o3, _ = env.reset(seed=8)
    assert (o3 - o1).abs().max() > 1e-3
    env.close()


def test_partial_reset_touches_only_its_envs():
    N = 8
    env = ec.make("StackCube-v1", N, BACKEND)
    base = env.unwrapped
    env.reset(seed=0)
    for _ in range(4):
        obs, *_ = env.step(torch.from_numpy(base.action_space.sample()))
    idx = torch.tensor([1, 4, 6])
    keep = torch.ones(N, dtype=torch.bool)
    keep[idx] = False
    new_obs, _ = env.reset(options=dict(env_idx=idx))
    ec.assert_obs_equal(new_obs[keep], obs[keep])
    assert (new_obs[idx] - obs[idx]).abs().max() > 1e-3
    assert torch.all(base.elapsed_steps[idx] == 0) and torch.all(base.elapsed_steps[keep] == 4)
    env.close()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_initial_placements_never_overlap(seed):
    N = 256
    env = ec.make("StackCube-v1", N, BACKEND)
    env.reset(seed=seed)
    base = env.unwrapped
    pa, pb = base.cubeA.pose.p, base.cubeB.pose.p
    d = torch.linalg.norm(pa[:, :2] - pb[:, :2], dim=1)
    # (float32 positions: the shared jitter added after the test may round the distance by an ulp)
    assert torch.all(d > 2 * SAMPLER_RADIUS - 1e-6), d.min()
    assert torch.all(pa[:, 2] == 0.02) and torch.all(pb[:, 2] == 0.02)
    # every cube is yawed (random about z only): unit quaternions with x = y = 0
    for q in (base.cubeA.pose.q, base.cubeB.pose.q):
        assert torch.allclose(q[:, 1:3], torch.zeros_like(q[:, 1:3])) and torch.allclose(q.norm(dim=1), torch.ones(N), atol=1e-6)
    env.close()


def test_known_answers():
    check_known_answers(BACKEND)
