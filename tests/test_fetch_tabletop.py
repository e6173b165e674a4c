"""The eight table-top tasks that list the Fetch, with the Fetch, on the oracle back end: the table scene's Fetch branch
(utils/scene_builder/table/scene_builder.py: fixed qpos, root pose behind the table on the ground, the wheels' collision bit
on the ground at build time), and the float64 statement of the Fetch's rules in the task epilogues
(tests/fetch_task_reference.py) pinned by hand-made cases and held against the torch path. The HIP side is
tests/test_gpu_fetch_tabletop.py."""
import numpy as np
import pytest
import torch

import maniskill_amd.envs  # noqa: F401
import gymnasium as gym
from tests import fetch_task_cases as fc
from tests import fetch_task_reference as fr
from tests import oracle_backend as ob

BACKEND = "oracle_f64_fetch_tabletop"
TASKS = list(fc.ALL_ENV_IDS)
HOLD_STEPS = 20


@pytest.fixture(scope="module", autouse=True)
def _backend():
    ob.register("f64", BACKEND)


def _base_drift(env, steps=HOLD_STEPS):
    """(|dz|, |dxy|) of base_link over `steps` zero-action control steps, the largest over the envs"""
    base = env.unwrapped
    p0 = base.agent.base_link.pose.p.clone()
    zero = torch.zeros(base.num_envs, base.single_action_space.shape[0])
    for _ in range(steps):
        out = env.step(zero)
    d = base.agent.base_link.pose.p - p0
    return float(d[:, 2].abs().max()), float(d[:, :2].norm(dim=1).max()), out


@pytest.fixture(scope="module")
def empty_drift():
    """what the Fetch's base does in Empty-v1 over the same steps: the bound of the table-top tasks"""
    env = gym.make("Empty-v1", robot_uids="fetch", num_envs=2, obs_mode="state", sim_backend=BACKEND)
    env.reset(seed=0)
    dz, dxy, _ = _base_drift(env)
    env.close()
    return dz, dxy


def _pairs(base):
    """the compiled collision pairs as (body row, body row); a static actor's shapes have row -1"""
    m = base.scene.model
    ps, sr = np.asarray(m.arrays["pair_shape"]).reshape(-1, 2), np.asarray(m.arrays["shape_row"])
    return [(int(sr[a]), int(sr[b])) for a, b in ps]


@pytest.mark.parametrize("task", TASKS)
def test_task_runs_with_the_fetch(task, empty_drift):
    env = gym.make(fc.ALL_ENV_IDS[task], robot_uids="fetch", num_envs=2, obs_mode="state", sim_backend=BACKEND)
    base = env.unwrapped
    obs, _ = env.reset(seed=3)
    agent = base.agent
    assert agent.uid == "fetch" and agent.robot.max_dof == fc.FETCH_DOF and agent.tcp.name == "gripper_link"
    assert obs.shape == (2, 2 * fc.FETCH_DOF + fc.OBS_EXTRA[task]) and base.single_observation_space.shape == obs.shape[1:]
    assert torch.isfinite(obs).all()
    # the reset state: the scene builder's qpos, without noise, and the root on the ground behind the table
    assert torch.allclose(agent.robot.get_qpos(), torch.tensor(fc.FETCH_QPOS, dtype=torch.float32).expand(2, -1), atol=1e-6)
    root = agent.robot.pose.raw_pose
    assert torch.allclose(root[:, :3], torch.tensor(fc.FETCH_ROOT).expand(2, -1), atol=1e-6) and torch.allclose(root[:, 3:], torch.tensor([1.0, 0, 0, 0]).expand(2, -1), atol=1e-6)
    model = base.scene.model
    assert (int(model.n_dof), int(model.n_free)) == (fc.FETCH_DOF, fc.N_FREE[task]) and fc.plain_instance(model) == (15, 2)
    # the pair table: no wheel <-> ground pair (the ground is the scene's one static actor), and the table against the arm
    rows = {name: i for i, name in enumerate(model.link_names)}
    pairs = _pairs(base)
    wheels = {rows["l_wheel_link"], rows["r_wheel_link"]}
    assert not any((a in wheels and b == -1) or (b in wheels and a == -1) for a, b in pairs)
    assert any({a, b} == {rows["base_link"], -1} for a, b in pairs), "the base's hull still faces the ground, as in Empty-v1"
    table = int(base.scene.actors["table-workspace"]._body_row)
    for link in ("gripper_link", "l_gripper_finger_link", "r_gripper_finger_link", "wrist_roll_link", "forearm_roll_link"):
        assert any({a, b} == {table, rows[link]} for a, b in pairs), link
    # the same seed gives the same reset
    obs2, _ = env.reset(seed=3)
    assert torch.equal(obs, obs2)
    obs3, _ = env.reset(seed=4)
    assert not torch.equal(obs, obs3)
    # 20 zero-action steps: finite outputs, and the base neither sinks nor drifts more than on the open ground
    dz, dxy, (obs, rew, term, trunc, info) = _base_drift(env)
    print(f"{task}: base_link over {HOLD_STEPS} steps |dz| {dz:.2e} |dxy| {dxy:.2e} (Empty-v1: {empty_drift[0]:.2e}, {empty_drift[1]:.2e})")
    # (both figures are of the order of 1e-22 m on this float64 back end, the velocity drives of the base answering arms in
    # two different poses: noise of the solver, not motion. The bound is Empty-v1's figure plus 1e-12 m, ten orders of
    # magnitude above that noise and nine below a millimetre of sinking or drift.)
    assert dz <= empty_drift[0] + 1e-12 and dxy <= empty_drift[1] + 1e-12
    assert torch.isfinite(obs).all() and torch.isfinite(rew).all() and rew.shape == (2,) and "success" in info
    assert base.scene.px.overflow_count() == 0
    env.close()


def test_other_robots_are_still_refused():
    from maniskill_amd.utils.scene_builder.table import TableSceneBuilder

    class _Env:
        robot_uids = "xarm6_robotiq"
        device = torch.device("cpu")

    sb = TableSceneBuilder.__new__(TableSceneBuilder)
    sb.env, sb.table = _Env(), type("T", (), dict(set_pose=lambda self, p: None))()
    with pytest.raises(NotImplementedError, match="xarm6_robotiq"):
        sb.initialize(torch.arange(1))


def test_a_panda_scene_after_a_fetch_scene_is_unaffected():
    """the ground's wheel bit belongs to the scene it was set in"""
    def panda_pairs():
        env = gym.make("PickCube-v1", num_envs=2, obs_mode="state", sim_backend=BACKEND)
        base = env.unwrapped
        obs, _ = env.reset(seed=1)
        out = (_pairs(base), np.asarray(base.scene.model.arrays["pair_shape"]).copy(), obs.clone())
        env.close()
        return out

    before = panda_pairs()
    env = gym.make("PickCube-v1", robot_uids="fetch", num_envs=2, obs_mode="state", sim_backend=BACKEND)
    env.reset(seed=1)
    env.close()
    after = panda_pairs()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and torch.equal(before[2], after[2])
    assert any(-1 in p for p in after[0]), "the Panda's links still face the ground"


# ---------------------------------------------------------------------------------------------------------------------
# the reference, pinned by hand
TCP, OBJ, GOAL, LEFT, RIGHT, CUBE = range(6)


def _state(N, n_dof=15):
    """a synthetic snapshot: six body rows at rest with identity rotations, one shape each, the pairs (left finger, object)
    and (object, right finger)"""
    rigid = np.zeros((6, N, 13), np.float32)
    rigid[:, :, 3] = 1.0
    return dict(rigid=rigid, qpos=np.zeros((N, n_dof), np.float32), qvel=np.zeros((N, n_dof), np.float32), imp=np.zeros((2, N, 3), np.float32),
                cnt=np.ones((2, N), np.int32), pair_shape=np.array([[LEFT, OBJ], [OBJ, RIGHT]]), shape_row=np.arange(6), dt=0.01)


def _dir(deg_from, axis_sign):
    """a unit vector at `deg_from` degrees from axis_sign * y, tilted towards x"""
    a = np.radians(deg_from)
    return np.array([np.sin(a), axis_sign * np.cos(a), 0.0])


def test_grasp_direction_by_hand():
    """the left finger closes along -y of its frame, the right along +y; 85 degrees is the limit"""
    cases = [  # (direction of the force on the left finger, on the right finger, left flag, right flag)
        (_dir(0, -1), _dir(0, +1), True, True),
        (_dir(84, -1), _dir(84, +1), True, True),
        (_dir(86, -1), _dir(84, +1), False, True),
        (_dir(84, -1), _dir(86, +1), True, False),
        (_dir(0, +1), _dir(0, +1), False, True),    # against the left finger's closing axis
        (_dir(0, -1), _dir(0, -1), True, False),    # against the right finger's
        (_dir(0, +1), _dir(0, -1), False, False),   # the Panda's directions: no grasp for a Fetch
    ]
    S = _state(len(cases))
    for e, (fl, fr_, _, _) in enumerate(cases):
        S["imp"][0, e] = 10.0 * fl * S["dt"]    # pair 0: the finger is shape A: the impulse on A
        S["imp"][1, e] = -10.0 * fr_ * S["dt"]  # pair 1: the finger is shape B: minus the impulse on A
    m = {}
    grasped, lflag, rflag = fr.fetch_grasp(S, m, OBJ, LEFT, RIGHT)
    assert fr._val(lflag).tolist() == [c[2] for c in cases] and fr._val(rflag).tolist() == [c[3] for c in cases]
    assert fr._val(grasped).tolist() == [c[2] and c[3] for c in cases]
    # a force below 0.5 N does not count, whatever its direction
    S["imp"][0] *= 0.04
    assert not fr._val(fr.fetch_grasp(S, {}, OBJ, LEFT, RIGHT)[1]).any()
    # a finger turned half round about z closes the other way
    S = _state(1)
    S["imp"][0, 0], S["imp"][1, 0] = 10.0 * _dir(0, -1) * S["dt"], -10.0 * _dir(0, +1) * S["dt"]
    S["rigid"][LEFT, 0, 3:7] = [0, 0, 0, 1]
    assert not fr._val(fr.fetch_grasp(S, {}, OBJ, LEFT, RIGHT)[0]).any()


def test_static_rule_by_hand():
    q, labels, static = fc.qvel_batch(len(fc.QVEL_CASES))
    got = fr.fetch_static(q, {})
    assert got.decided.all() and fr._val(got).tolist() == static.tolist(), labels
    # the cases the issue names, spelled out
    def one(**joints):
        v = np.zeros((1, 15), np.float32)
        for j, x in joints.items():
            v[0, int(j[1:])] = x
        return bool(fr._val(fr.fetch_static(v, {}))[0])

    assert one(j0=0.04) and not one(j0=0.06) and one(j1=0.04) and not one(j2=0.06)
    assert one(j3=0.19) and not one(j3=0.21) and one(j12=0.19) and not one(j12=0.21)
    assert one(j7=-1.0) and one(j0=-1.0), "signed: fast in the negative direction is static"
    assert one(j13=9.0, j14=9.0), "the gripper joints are not read"
    assert not one(j3=0.06 + 0.2) and one(j3=0.06), "the base's threshold holds for the base alone"
    assert not one(j5=0.1, j0=0.06)
    # another threshold, as a task may pass it
    assert not bool(fr._val(fr.fetch_static(np.full((1, 15), 0.03, np.float32), {}, threshold=0.02))[0])


def test_reward_norm_by_hand():
    """PickCube's static reward covers all 15 joints of a Fetch, PokeCube's 13; both read the Fetch's static rule"""
    assert fr.reward_norm_dofs("pick", "fetch", 15) == 15 and fr.reward_norm_dofs("pick", "panda", 9) == 7
    assert fr.reward_norm_dofs("poke", "fetch", 15) == 13 and fr.reward_norm_dofs("poke", "panda", 9) == 7
    S = _state(3)
    S["rigid"][TCP, :, :3] = [0.1, 0.0, 0.3]
    S["rigid"][OBJ, :, :3] = [0.1, 0.0, 0.2]
    S["rigid"][GOAL, :, :3] = [0.1, 0.0, 0.21]   # placed: 1 cm from the goal
    S["rigid"][CUBE, :, :3] = [0.1, 0.0, 0.02]
    S["qvel"][:, 5], S["qvel"][:, 13], S["qvel"][:, 14] = 0.3, 0.4, 1.2   # env 0: a body joint above 0.2: not static
    S["qvel"][1, 5] = -0.3                                                # env 1: static by the signed rule, same norm
    S["qvel"][2, 5] = 0.0                                                 # env 2: static, the gripper still moving
    common = dict(tcp_row=TCP, left_row=LEFT, right_row=RIGHT, min_force=0.5, max_angle_deg=85.0, reward_scale=1.0, static_thresh=0.2)
    R = fr.evaluate("pick", S, dict(common, obj_row=OBJ, goal_row=GOAL, goal_thresh=0.025))
    assert R["flags"]["is_obj_placed"].all() and R["flags"]["is_robot_static"].tolist() == [False, True, True] and R["flags"]["success"].tolist() == [False, True, True]
    reach = 1 - np.tanh(5 * 0.1)
    norm15 = np.sqrt(0.3 ** 2 + 0.4 ** 2 + 1.2 ** 2)
    assert abs(R["reward"][0] - (reach + 1 - np.tanh(5 * norm15))) < 1e-6 and R["reward"][1] == 5.0 and R["reward"][2] == 5.0
    # PokeCube: the cube on its goal; the peg (row OBJ) in the air
    P = dict(common, peg_row=OBJ, cube_row=CUBE, goal_row=GOAL, peg_half_length=0.12, cube_half_size=0.02, goal_radius=0.05, align_thresh=0.05, reach_thresh=0.01)
    R = fr.evaluate("poke", S, P)
    assert R["flags"]["is_cube_placed"].all() and R["flags"]["success"].tolist() == [False, True, True]
    assert abs(R["reward"][0] - (2 * reach + 1 - np.tanh(5 * 0.3))) < 1e-6 and R["reward"][1] == 10.0, "13 joints: the gripper's velocity is no part of the norm"


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task", fc.GATED)
def test_torch_path_matches_reference(task):
    """the scripted squeeze on the oracle, then the velocity table: the torch path (Fetch.is_grasping / is_static, the task's
    evaluate / observation / reward) against the float64 reference. Both values of the grasp flag occur, a quarter of the
    envs at least on each side."""
    N = 30
    env = fc.make_env(task, N, BACKEND)
    base = env.unwrapped
    closed = np.arange(N) % 2 == 0
    fc.squeeze(env, task, closed)
    fc.arrange(task, base, np.arange(N) % 3 != 2)
    S = fc.snapshot(base)
    P = fc.params(task, base)
    S["qvel"], labels, static = fc.qvel_batch(N)
    fc.write_buffers(base, S)
    R = fr.evaluate(task, S, P)
    g = R["flags"][fr.GRASP_FLAG[task]]
    assert min(int(g.sum()), int((~g).sum())) >= N // 4 and np.array_equal(g, closed), (task, g.tolist())
    if "fetch_static" in R["flags"]:
        assert np.array_equal(R["flags"]["fetch_static"], static)
    if task in ("pick", "poke"):
        assert R["flags"]["success"].any() and (~R["flags"]["success"] & static).any() and (~static & R["flags"]["is_obj_placed" if task == "pick" else "is_cube_placed"]).any()
    if task == "place":
        assert (R["flags"]["is_obj_on_bin"] & g & static).any() and (R["flags"]["is_obj_on_bin"] & g & ~static).any()
    d = fc.compare(task, fc.torch_outputs(task, base), R, labels, 2e-5 * fc.TOP_REWARD[task] * P["reward_scale"], "torch path (oracle)")
    print(f"{task}: max |torch path - f64 reference| reward {d:.3e}")
    env.close()
