"""RollBall-v1 and PullCube-v1 on the CPU: the env layer driven by the oracle registered as a test backend (as
tests/test_stack_cube.py does), and the torch path of both tasks against the float64 reference
(tests/roll_pull_reference.py) over the case tables of tests/roll_pull_cases.py. No kernel involved; the same tables run
through the native epilogues in tests/test_gpu_roll_pull.py."""
import numpy as np
import pytest
import torch

from tests import env_checks as ec
from tests import oracle_backend as ob
from tests import roll_pull_cases as rc
from tests import roll_pull_reference as ref

BACKEND = "oracle_f64_env"


@pytest.fixture(scope="module", autouse=True)
def _register():
    ob.register("f64", BACKEND)


def test_registered_shapes_and_key_order():
    N = 4
    for env_id, steps, robots, D, keys in (
        ("RollBall-v1", 80, ["panda"], 18 + 26, ["tcp_pose", "goal_pos", "ball_pose", "ball_vel", "tcp_to_ball_pos", "ball_to_goal_pos"]),
        ("PullCube-v1", 50, ["panda", "fetch"], 18 + 17, ["tcp_pose", "goal_pos", "obj_pose"]),
    ):
        env = ec.make(env_id, N, BACKEND)
        base = env.unwrapped
        assert env.spec.max_episode_steps == steps and base.SUPPORTED_ROBOTS == robots and base.robot_uids == "panda"
        obs, info = env.reset(seed=0)
        assert obs.shape == (N, D) and obs.dtype == torch.float32 and base.single_action_space.shape == (8,)
        extra = base._get_obs_extra(info)
        assert list(extra.keys()) == keys
        # the flat observation: qpos, qvel, then the extras in that order
        flat = torch.cat([base.agent.robot.get_qpos(), base.agent.robot.get_qvel()] + [extra[k] for k in keys], 1)
        assert torch.equal(obs, flat)
        obs, rew, term, trunc, info = env.step(torch.from_numpy(base.action_space.sample()))
        assert obs.shape == (N, D) and rew.shape == (N,) and torch.isfinite(obs).all() and torch.isfinite(rew).all()
        assert info["success"].dtype == torch.bool and torch.all(info["elapsed_steps"] == 1) and torch.equal(term, info["success"])
        env.close()


def test_mani_skill_alias_exports_the_classes():
    from mani_skill.envs.tasks.tabletop import PullCubeEnv, RollBallEnv
    from maniskill_amd.envs.tasks.tabletop.pull_cube import PullCubeEnv as P
    from maniskill_amd.envs.tasks.tabletop.roll_ball import RollBallEnv as R

    assert RollBallEnv is R and PullCubeEnv is P


@pytest.mark.parametrize("seed", [0, 1])
def test_reset_ranges(seed):
    N = 256
    env = ec.make("RollBall-v1", N, BACKEND)
    env.reset(seed=seed)
    base = env.unwrapped
    b, g = base.ball.pose.raw_pose, base.goal_region.pose.raw_pose
    eps = 1e-6
    assert torch.all(b[:, 0] >= -0.4 - eps) and torch.all(b[:, 0] <= 0.2 + eps) and torch.all(b[:, 1] >= 0.5 - eps) and torch.all(b[:, 1] <= 0.7 + eps)
    assert torch.all(b[:, 2] == np.float32(0.035)) and torch.all(b[:, 3] == 1) and torch.all(b[:, 4:] == 0)
    assert torch.all(g[:, 0] >= -0.4 - eps) and torch.all(g[:, 0] <= 0.2 + eps) and torch.all(g[:, 1] >= -0.9 - eps) and torch.all(g[:, 1] <= -0.7 + eps)
    assert torch.all(g[:, 2] == np.float32(1e-3))
    assert b[:, 0].max() - b[:, 0].min() > 0.4 and g[:, 1].max() - g[:, 1].min() > 0.15  # (the ranges are used)
    # the root pose the task writes over the table scene's (read back from the simulation, which reports the link's pose
    # with a unit quaternion: the stated one is 6e-5 off unit length)
    root = base.agent.robot.pose.raw_pose
    assert torch.allclose(root, torch.tensor([[-0.1, 1.0, 0.0, 0.7071, 0.0, 0.0, -0.7072]]).expand(N, -1), atol=1e-4, rtol=0)
    assert torch.all(root[:, 6] < -root[:, 3])  # (the larger z component survives the normalisation)
    assert base.reached_status.dtype == torch.float32 and base.reached_status.shape == (N,) and torch.all(base.reached_status == 0)
    env.close()

    env = ec.make("PullCube-v1", N, BACKEND)
    env.reset(seed=seed)
    base = env.unwrapped
    o, g = base.obj.pose.raw_pose, base.goal_region.pose.raw_pose
    assert torch.all(o[:, :2].abs() <= 0.1 + eps) and torch.all(o[:, 2] == np.float32(0.02)) and torch.all(o[:, 3] == 1)
    assert o[:, 0].max() - o[:, 0].min() > 0.15 and o[:, 1].max() - o[:, 1].min() > 0.15
    # the goal lies 0.1 + radius behind the cube (-x), on the table
    assert torch.allclose(g[:, 0], o[:, 0] - 0.2, atol=1e-6) and torch.equal(g[:, 1], o[:, 1]) and torch.all(g[:, 2] == np.float32(1e-3))
    env.close()


def _measure(task, normalized):
    """the torch path on the case table against the reference: -> (max reward difference, reference result, labels)"""
    env = rc.make_env(task, 48, BACKEND)
    base = env.unwrapped
    base._reward_mode = "normalized_dense" if normalized else "dense"
    P = rc.params(task, base, normalized=normalized)
    S, labels = rc.build_batch(task, rc.snapshot(base, task), P)
    rc.write_buffers(base, S)
    R = ref.TASKS[task](S, P)
    got = rc.torch_outputs(task, base, S)
    diff, excluded = rc.check(task, got, R, labels, np.inf, what="torch path")
    assert excluded == 0
    env.close()
    return diff, R, labels


@pytest.mark.parametrize("task", ["roll", "pull"])
def test_torch_path_matches_reference(task):
    diff, R, labels = _measure(task, normalized=False)
    diff_n, Rn, _ = _measure(task, normalized=True)
    print(f"\n{task}: {len(labels)} cases, max |torch f32 - f64| dense {diff:.3e}, normalised {diff_n:.3e}")
    # the recorded values (the GPU tolerances derive from them) still bound what is measured
    assert diff <= rc.MEASURED[task] and diff_n <= rc.MEASURED_NORMALIZED[task], (diff, diff_n)
    # normalised = dense over the top reward
    assert np.allclose(Rn["reward"] * rc.TOP_REWARD[task], R["reward"], rtol=1e-6)
    # the table reaches every tier
    F, lab = R["flags"], np.array(labels)
    top = rc.TOP_REWARD[task]
    assert np.all(R["reward"][F["success"]] == top) and np.all(R["reward"][~F["success"]] < top)
    if task == "roll":
        new = R["reached_new"]
        for case, before, after in (("far, latch 0", 0, 0), ("hit distance inside", 0, 1), ("hit distance outside", 0, 0), ("latch 1, tcp far", 1, 1),
                                    ("success, latch 0", 0, 0), ("success, latch 1", 1, 1), ("above the goal centre, tcp at the hit point", 0, 1)):
            assert np.all(new[lab == case] == after), case
        sel = lab == "latch 1, tcp far"
        assert np.allclose(R["reward"][sel], 20 * (1 - np.tanh(R["d_xy"][sel])) + 1, atol=1e-12) and np.all(R["reward"][sel] > 1)
        for case in ("success, latch 0", "success, latch 1", "above the goal centre"):
            assert F["success"][lab == case].all(), case
        assert np.isfinite(R["reward"]).all() and np.isfinite(R["obs"]).all()
        for case in rc.FLIPS:
            assert np.all(new[lab == case] == 1)
    else:
        for reached in (False, True):
            for inside in (False, True):
                assert ((F["reached"] == reached) & (F["success"] == inside)).any()
        assert F["success"][lab == "inside, lifted (no height condition)"].all()


def test_normalized_reward_is_dense_over_top_reward():
    for env_id, top in (("RollBall-v1", 30.0), ("PullCube-v1", 3.0)):
        rews = []
        for mode in ("dense", "normalized_dense"):
            env = ec.make(env_id, 4, BACKEND, reward_mode=mode)
            env.reset(seed=2)
            a = torch.zeros(4, 8)
            rews.append(torch.stack([env.step(a)[1] for _ in range(3)]))
            env.close()
        assert torch.equal(rews[1], rews[0] / top), env_id


def test_latch_survives_steps_and_partial_reset_clears_only_its_envs():
    N = 8
    env = ec.make("RollBall-v1", N, BACKEND, reward_mode="dense")
    base = env.unwrapped
    env.reset(seed=0)
    a = torch.zeros(N, 8)
    env.step(a)
    assert torch.all(base.reached_status == 0)  # (the tcp starts half a metre from the hit point)
    base.reached_status[:] = torch.tensor([1, 0, 1, 1, 0, 1, 1, 0], dtype=torch.float32)
    before = base.reached_status.clone()
    storage = base.reached_status.data_ptr()
    for _ in range(3):
        obs, rew, *_ = env.step(a)
    assert torch.equal(base.reached_status, before), "the latch does not survive steps"
    assert torch.all(rew[before == 1] > 1.0) and torch.all(rew[before == 0] < 1.0)  # the 20 (...) + 1 branch / the reaching branch
    idx = torch.tensor([0, 3, 4])
    env.reset(options=dict(env_idx=idx))
    want = before.clone()
    want[idx] = 0
    assert torch.equal(base.reached_status, want)
    assert base.reached_status.data_ptr() == storage  # (cleared in place: a native epilogue keeps pointing at it)
    # the observation of a state does not move the latch: only the reward does
    base.get_obs(base.get_info())
    assert torch.equal(base.reached_status, want)
    env.close()
