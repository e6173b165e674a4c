"""PokeCube-v1 and LiftPegUpright-v1 on the CPU: the env layer driven by the oracle registered as a test backend (as
tests/test_roll_pull.py does), `matrix_to_euler_angles`, the torch path of both tasks against the float64 reference
(tests/poke_lift_reference.py) over the case tables of tests/poke_lift_cases.py, and physics known answers. No kernel
involved; the same tables run through the native epilogues in tests/test_gpu_poke_lift.py."""
import itertools
import math

import numpy as np
import pytest
import torch

from maniskill_amd.utils.geometry import rotation_conversions as rc
from tests import env_checks as ec
from tests import oracle_backend as ob
from tests import poke_lift_cases as pc
from tests import poke_lift_reference as ref

BACKEND = "oracle_f64_env"
POKE_KEYS = ["tcp_pose", "cube_pose", "peg_pose", "goal_pos", "tcp_to_peg_pos", "peg_to_cube_pos", "cube_to_goal_pos", "peghead_to_cube_pos"]
POKE_INFO = ["success", "is_cube_placed", "is_peg_cube_fit", "is_peg_grasped", "angle_diff", "head_to_cube_dist"]


@pytest.fixture(scope="module", autouse=True)
def _register():
    ob.register("f64", BACKEND)


def test_registered_shapes_and_key_order():
    N = 4
    for env_id, D, keys, info_keys in (("PokeCube-v1", 18 + 36, POKE_KEYS, POKE_INFO), ("LiftPegUpright-v1", 18 + 14, ["tcp_pose", "obj_pose"], ["success"])):
        env = ec.make(env_id, N, BACKEND)
        base = env.unwrapped
        assert env.spec.max_episode_steps == 50 and base.SUPPORTED_ROBOTS == ["panda", "fetch"] and base.robot_uids == "panda"
        obs, info = env.reset(seed=0)
        assert obs.shape == (N, D) and obs.dtype == torch.float32 and base.single_action_space.shape == (8,)
        assert torch.allclose(base.agent.robot.pose.p, torch.tensor([[-0.615, 0.0, 0.0]]).expand(N, -1))
        ev = base.evaluate()
        assert list(ev.keys()) == info_keys
        extra = base._get_obs_extra(ev)
        assert list(extra.keys()) == keys
        # the flat observation: qpos, qvel, then the extras in that order
        flat = torch.cat([base.agent.robot.get_qpos(), base.agent.robot.get_qvel()] + [extra[k] for k in keys], 1)
        assert torch.equal(obs, flat)
        if env_id == "PokeCube-v1":  # the reference's quirks: goal_pos is the peg's position, the head offset is not rotated
            assert torch.equal(extra["goal_pos"], base.peg.pose.p)
            assert torch.equal(extra["peghead_to_cube_pos"], base.peg.pose.p + torch.tensor([base.peg_half_length, 0, 0]) - base.cube.pose.p)
        obs, rew, term, trunc, info = env.step(torch.from_numpy(base.action_space.sample()))
        assert obs.shape == (N, D) and rew.shape == (N,) and torch.isfinite(obs).all() and torch.isfinite(rew).all()
        assert [k for k in info if k in info_keys] == info_keys
        assert info["success"].dtype == torch.bool and torch.all(info["elapsed_steps"] == 1) and torch.equal(term, info["success"])
        env.close()


def test_mani_skill_alias_exports_the_classes():
    from mani_skill.envs.tasks.tabletop import LiftPegUprightEnv, PokeCubeEnv
    from maniskill_amd.envs.tasks.tabletop.lift_peg_upright import LiftPegUprightEnv as L
    from maniskill_amd.envs.tasks.tabletop.poke_cube import PokeCubeEnv as P

    assert PokeCubeEnv is P and LiftPegUprightEnv is L


def test_reset_ranges():
    N = 256
    env = ec.make("PokeCube-v1", N, BACKEND)
    env.reset(seed=1)
    base = env.unwrapped
    p, c, g = base.peg.pose.raw_pose, base.cube.pose.raw_pose, base.goal_region.pose.raw_pose
    eps = 1e-6
    assert torch.all(p[:, :2].abs() <= 0.1 + eps) and torch.all(p[:, 2] == np.float32(0.025)) and torch.all(p[:, 3] == 1)
    assert torch.allclose(c[:, 0], p[:, 0] + 0.22, atol=1e-6) and torch.all(c[:, 1].abs() <= 0.1 + eps) and torch.all(c[:, 2] == np.float32(0.02))
    yaw = 2 * torch.atan2(c[:, 6], c[:, 3])
    assert torch.all(c[:, 4:6] == 0) and torch.all(yaw.abs() <= math.pi / 6 + 1e-5) and yaw.max() - yaw.min() > 0.8
    assert torch.allclose(g[:, 0], c[:, 0] + 0.1, atol=1e-6) and torch.equal(g[:, 1], c[:, 1]) and torch.all(g[:, 2] == np.float32(1e-3))
    env.close()
    env = ec.make("LiftPegUpright-v1", N, BACKEND)
    env.reset(seed=1)
    p = env.unwrapped.peg.pose.raw_pose
    s = np.float32(math.sqrt(0.5))
    assert torch.all(p[:, :2].abs() <= 0.1 + eps) and torch.all(p[:, 2] == np.float32(0.025))
    assert torch.allclose(p[:, 3:], torch.tensor([[s, s, 0, 0]]).expand(N, -1), atol=1e-6)
    env.close()


# ---------------------------------------------------------------------------------------------------------------------
def test_matrix_to_euler_angles_round_trip():
    """all six Tait-Bryan conventions on seeded angles with |b| <= 1.4, in float64 and float32"""
    g = torch.Generator().manual_seed(11)
    ang = (2 * torch.rand(512, 3, generator=g, dtype=torch.float64) - 1) * torch.tensor([3.1, 1.4, 3.1], dtype=torch.float64)
    for conv in ("".join(p) for p in itertools.permutations("XYZ")):
        back = rc.matrix_to_euler_angles(rc.euler_angles_to_matrix(ang, conv), conv)
        assert back.shape == ang.shape and float((back - ang).abs().max()) < 1e-12, conv
        # float32 against the float64 angles: the entries carry 2^-24 each, the middle angle's asin amplifies its own by
        # 1 / cos 1.4 = 5.9, the outer angles' atan2 theirs by the same factor: 5e-6 bounds all three
        back32 = rc.matrix_to_euler_angles(rc.euler_angles_to_matrix(ang.float(), conv), conv)
        assert back32.dtype == torch.float32 and float((back32.double() - ang).abs().max()) < 5e-6, conv


def test_matrix_to_euler_angles_xyz_closed_form():
    g = torch.Generator().manual_seed(12)
    R = rc.quaternion_to_matrix(torch.nn.functional.normalize(torch.randn(64, 4, generator=g, dtype=torch.float64), dim=1))
    e = rc.matrix_to_euler_angles(R, "XYZ")
    want = torch.stack([torch.atan2(-R[:, 1, 2], R[:, 2, 2]), torch.asin(R[:, 0, 2]), torch.atan2(-R[:, 0, 1], R[:, 0, 0])], 1)
    assert torch.equal(e, want)
    # a batch shape in front, and a hand-made matrix: Rx(0.3) Ry(-0.5) Rz(2.0)
    one = rc.euler_angles_to_matrix(torch.tensor([[[0.3, -0.5, 2.0]]], dtype=torch.float64), "XYZ")
    assert rc.matrix_to_euler_angles(one, "XYZ").shape == (1, 1, 3)
    assert torch.allclose(rc.matrix_to_euler_angles(one, "XYZ")[0, 0], torch.tensor([0.3, -0.5, 2.0], dtype=torch.float64), atol=1e-14)
    for bad in ("XY", "XXY", "XYA"):
        with pytest.raises(ValueError):
            rc.matrix_to_euler_angles(one, bad)
    with pytest.raises(ValueError):
        rc.matrix_to_euler_angles(torch.zeros(2, 3), "XYZ")


# ---------------------------------------------------------------------------------------------------------------------
_GRASPED = {}


def _grasped_env(task):
    """one env per task with the scripted grasp done, shared by the measurements (nothing steps it afterwards)"""
    if task not in _GRASPED:
        env = pc.make_env(task, 32, BACKEND)
        pc.scripted_grasp(env, task)
        _GRASPED[task] = (env, pc.snapshot(env.unwrapped))
    return _GRASPED[task]


def _measure(task, normalized):
    """the torch path on the case table against the reference: -> (reward difference, metric difference, reference, labels)"""
    env, S0 = _grasped_env(task)
    base = env.unwrapped
    base._reward_mode = "normalized_dense" if normalized else "dense"
    P = pc.params(task, base, normalized=normalized)
    S, labels = pc.build_batch(task, S0, P)
    pc.write_buffers(base, S)
    R = ref.TASKS[task](S, P)
    got = pc.torch_outputs(task, base)
    diff, d_m, excluded = pc.check(task, got, R, labels, np.inf, np.inf, what="torch path")
    assert excluded == 0
    return diff, d_m, R, labels


@pytest.mark.parametrize("task", ["poke", "lift"])
def test_torch_path_matches_reference(task):
    diff, d_m, R, labels = _measure(task, normalized=False)
    diff_n, d_mn, Rn, _ = _measure(task, normalized=True)
    print(f"\n{task}: {len(labels)} cases, max |torch f32 - f64| dense {diff:.3e}, normalised {diff_n:.3e}, metrics {max(d_m, d_mn):.3e}, "
          f"finger forces of env 0: {float(R['forces'][0][0]):.2f} / {float(R['forces'][1][0]):.2f} N")
    # the recorded values (the GPU tolerances derive from them) still bound what is measured
    assert diff <= pc.MEASURED[task] and diff_n <= pc.MEASURED_NORMALIZED[task], (diff, diff_n)
    assert max(d_m, d_mn) <= pc.MEASURED["poke_metrics"]
    # normalised = dense over the top reward
    top = pc.TOP_REWARD[task]
    assert np.allclose(Rn["reward"] * top, R["reward"], rtol=1e-6)
    F, lab, r = R["flags"], np.array(labels), R["reward"]
    assert np.all(r[F["success"]] == top) and np.all(r[~F["success"]] < top) and F["success"].any()
    g = F["is_peg_grasped"] if task == "poke" else F["is_grasped"]
    assert g.any() and (~g).any() and (F["left"] != F["right"]).any()
    if task == "poke":
        held, fit, placed = F["held"], F["is_peg_cube_fit"], F["is_cube_placed"]
        # every tier: reaching only (below 2), held (4 .. 6), fit and held (7 .. 8), each with and without the static term
        t1, t2, t3 = ~held & ~placed, held & ~fit & ~placed, held & fit & ~placed
        assert t1.any() and np.all(r[t1] < 2) and t2.any() and np.all((r[t2] >= 4) & (r[t2] <= 6)) and t3.any() and np.all((r[t3] >= 7) & (r[t3] <= 8))
        assert (fit & ~held).any() and np.all(r[fit & ~held & ~placed] < 2), "fit without the grasp stays on the reaching tier"
        moving = placed & ~F["success"]
        assert (moving & held & fit).any() and (moving & ~held).any() and np.all(r[moving & held & fit] > 7)
        assert F["success"][lab == "placed and static"].all() and F["success"][lab == "placed, finger joint velocity is not read"].all()
        for name in ("aligned", "close", "reached", "static", "is_cube_placed"):
            assert F[name].any() and (~F[name]).any(), name
        assert np.allclose(R["metrics"][lab == "angle difference is not wrapped", 0], 3.4, atol=1e-6)  # (wrapped: 2.88)
    else:
        for case, ok in (("lying flat, grasped", False), ("upright, angle +", True), ("upright, angle -", True), ("upright, upside down", True),
                         ("upright, not grasped", True), ("upright, too high", False), ("upright, too low", False), ("height inside, above", True),
                         ("height outside, below", False), ("tilt inside", True), ("tilt outside", False), ("tilt inside, beyond, angle -", True),
                         ("tilt outside, beyond, angle -, not grasped", False)):
            assert np.all(F["success"][lab == case] == ok), case
        flat_g, flat_n = r[lab == "lying flat, grasped"], r[lab == "lying flat, not grasped"]
        # lying flat: no rotation term; grasped: the full reaching term 1 / 5
        assert np.allclose(flat_g, 1 - np.tanh(5 * (0.12 - 0.025)) + 0.2, atol=1e-6) and np.all(flat_n < flat_g)


def test_normalized_reward_is_dense_over_top_reward():
    for env_id, top in (("PokeCube-v1", 10.0), ("LiftPegUpright-v1", 3.0)):
        rews = []
        for mode in ("dense", "normalized_dense"):
            env = ec.make(env_id, 4, BACKEND, reward_mode=mode)
            env.reset(seed=2)
            a = torch.zeros(4, 8)
            rews.append(torch.stack([env.step(a)[1] for _ in range(3)]))
            env.close()
        assert torch.equal(rews[1], rews[0] / top), env_id


# ---------------------------------------------------------------------------------------------------------------------
def test_peg_flat_and_upright_known_answers():
    """zero action, a few control steps: a peg laid flat stays at z = half_width and is not successful; a peg stood on its
    end at z = half_length stays there, and `success` is true"""
    from maniskill_amd.utils.structs.pose import Pose

    N = 4
    env = ec.make("LiftPegUpright-v1", N, BACKEND, reward_mode="dense")
    base = env.unwrapped
    env.reset(seed=3)
    a = torch.zeros(N, 8)
    for _ in range(5):
        _, _, _, _, info = env.step(a)
    assert torch.allclose(base.peg.pose.p[:, 2], torch.full((N,), 0.025), atol=5e-4) and not info["success"].any()
    q = rc.euler_angles_to_quaternion(torch.tensor([[math.pi / 2, 0.0, math.pi / 2]]), "XYZ").expand(N, -1)
    p = torch.tensor([[0.1, 0.2, 0.12]]).expand(N, -1)  # (beside the arm's rest pose)
    base.peg.set_pose(Pose.create_from_pq(p.clone(), q.clone()))
    base.peg.set_linear_velocity(torch.zeros(N, 3))
    base.peg.set_angular_velocity(torch.zeros(N, 3))
    base.scene._gpu_apply_all()
    base.scene._gpu_fetch_all()
    assert base.evaluate()["success"].all()
    for _ in range(5):
        _, rew, _, _, info = env.step(a)
    assert torch.allclose(base.peg.pose.p[:, 2], torch.full((N,), 0.12), atol=5e-4) and torch.allclose(base.peg.pose.p[:, :2], p[:, :2], atol=1e-3)
    assert info["success"].all() and torch.all(rew == 3.0)
    env.close()


def test_poke_reset_state_rests_and_is_not_successful():
    N = 4
    env = ec.make("PokeCube-v1", N, BACKEND)
    base = env.unwrapped
    env.reset(seed=3)
    p0, c0 = base.peg.pose.raw_pose.clone(), base.cube.pose.raw_pose.clone()
    a = torch.zeros(N, 8)
    for _ in range(5):
        _, _, _, _, info = env.step(a)
    assert not info["success"].any() and not info["is_cube_placed"].any() and not info["is_peg_grasped"].any()
    assert torch.allclose(base.peg.pose.raw_pose, p0, atol=5e-4) and torch.allclose(base.cube.pose.raw_pose, c0, atol=5e-4)
    assert float(base.peg.linear_velocity.abs().max()) < 1e-2 and float(base.cube.linear_velocity.abs().max()) < 1e-2
    # the cube starts 0.1 ahead of the peg's head, turned by up to 30 degrees: both metrics say so
    assert torch.all((info["head_to_cube_dist"] >= 0.1 - 1e-3) & (info["head_to_cube_dist"] <= math.hypot(0.1, 0.2) + 1e-3))
    assert torch.all(info["angle_diff"] <= math.pi / 6 + 1e-3)
    assert base.scene.px.overflow_count() == 0
    env.close()
