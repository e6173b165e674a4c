"""Constructed states for the PlugCharger epilogue, one case per env index (the table repeats over the batch): the
charger's pose is given in the frame of the env's stored goal and installed by teleport (written into the user-visible
buffers; nothing is stepped). Shared by tests/test_plug_charger.py (the torch path on the oracle backend) and
tests/test_gpu_plug_charger.py (k_task_plug), both against tests/plug_reference.py.

Margins. A case meant to lie on one side of a threshold must lie there for the float64 reference AND for any float32
evaluation of the same inputs, so it sits at least 8 x the float32 path's own error away from the threshold. That error
is measured, not assumed: the torch path (float32, CPU, oracle backend) against the float64 reference over this table, the
larger of the two info floats, over batches of 128, 67, 17 and 1 envs at seed 7 and of 128 envs at seeds 1 and 2
(tests/test_plug_charger.py::test_torch_path_matches_reference prints its own figures and asserts that the band still
bounds them):

    obj_to_goal_angle  max |torch f32 - f64| = 5.83e-7 rad (the cases near pi; 3.9e-8 at the 0.2 rad threshold)
    obj_to_goal_dist   max |torch f32 - f64| = 1.49e-8 m   (the far-away case; 3.5e-10 at the 5 mm threshold)

MEASURED is that band, 5.9e-7, one figure for both columns as for the other epilogues' metrics. The threshold cases sit
EDGE_D = 6e-6 m and EDGE_A = 2e-5 rad from the thresholds: 10 x and 34 x the band, and no less than 8 x it after the poses
are rounded to float32 (`check_margins`). The native epilogue's metrics are held to 4 x MEASURED = 2.36e-6, the project's
rule for every epilogue."""
import numpy as np
import torch

from tests import plug_reference as ref

f32 = np.float32
ENV_ID = "PlugCharger-v1"
OBS_EXTRA = 28
DIST_THRESH, ANGLE_THRESH = 5e-3, 0.2
EDGE_D, EDGE_A = 6e-6, 2e-5
MEASURED = 5.9e-7
NAN_CASE = 5  # the table's index of the NaN pose; installed in env NAN_CASE alone, its repeats take the identity


def make_env(N, backend, seed=7, **kw):
    import maniskill_amd.envs  # noqa: F401  (registers the task; installs the gymnasium stand-in when gymnasium is absent)
    import gymnasium as gym

    env = gym.make(ENV_ID, num_envs=N, sim_backend=backend, **kw)
    env.reset(seed=seed)
    return env


def params(base):
    """task parameters as the env's own fused path states them; every float rounded to float32, the value the native
    struct carries"""
    r = lambda o: int(o._body_row)
    F = lambda x: float(f32(x))
    return dict(tcp_row=r(base.agent.tcp), charger_row=r(base.charger), receptacle_row=r(base.receptacle), dist_thresh=F(base.dist_thresh),
                angle_thresh=F(base.angle_thresh), reward_scale=F(1))


def native_task(P, goal: torch.Tensor):
    from maniskill_amd import native

    return native.PlugTask(goal_pose=goal.data_ptr(), **P)


def snapshot(base):
    """what the epilogue reads, as numpy float32 (tests/plug_reference.py `S`)"""
    px, N = base.scene.px, base.num_envs
    return dict(rigid=px.cuda_rigid_body_data.torch().cpu().numpy().reshape(-1, N, 13).copy(), qpos=px.cuda_articulation_qpos.torch().cpu().numpy().copy(),
                qvel=px.cuda_articulation_qvel.torch().cpu().numpy().copy(), goal=base._goal_pose_raw.cpu().numpy().copy())


def write_buffers(base, S):
    """the case batch into the user-visible buffers and the stored goal (nothing is applied to the simulation state)"""
    px, dev = base.scene.px, base.device
    px.cuda_rigid_body_data.torch()[:] = torch.from_numpy(S["rigid"].reshape(-1, 13)).to(dev)
    px.cuda_articulation_qpos.torch()[:] = torch.from_numpy(S["qpos"]).to(dev)
    px.cuda_articulation_qvel.torch()[:] = torch.from_numpy(S["qvel"]).to(dev)
    base._goal_pose_raw[:] = torch.from_numpy(S["goal"]).to(dev)


def torch_outputs(base):
    info = base.evaluate()
    obs = base.get_obs(info)
    rew = base.get_reward(obs=obs, action=None, info=info)
    return dict(obs=obs.cpu().numpy(), reward=rew.cpu().numpy(), success=info["success"].cpu().numpy().astype(bool),
                metrics=np.stack([info["obj_to_goal_dist"].cpu().numpy(), info["obj_to_goal_angle"].cpu().numpy()], 1))


# ---------------------------------------------------------------------------------------------------------------------
# the table: (label, offset in the goal frame [m], rotation vector in the goal frame [rad], flags)
#   "neg": the charger's quaternion is negated; "nan": a NaN pose; "rest": the charger stays where the reset put it
X, Y, Z = np.eye(3)
SKEW = np.array([2.0, -1.0, 2.0]) / 3.0
D_IN, D_OUT = DIST_THRESH - EDGE_D, DIST_THRESH + EDGE_D
A_IN, A_OUT = ANGLE_THRESH - EDGE_A, ANGLE_THRESH + EDGE_A
TABLE = [
    ("identity", 0 * X, 0 * Z, ""),
    ("dist inside, along x", D_IN * X, 0 * Z, ""),
    ("dist outside, along x", D_OUT * X, 0 * Z, ""),
    ("angle inside, yaw", 0 * X, A_IN * Z, ""),
    ("angle outside, yaw", 0 * X, A_OUT * Z, ""),
    ("nan pose", 0 * X, 0 * Z, "nan"),
    ("dist inside, skew", D_IN * SKEW, 0 * Z, ""),
    ("dist outside, skew", D_OUT * SKEW, 0 * Z, ""),
    ("angle inside, about x", 0 * X, -A_IN * X, ""),
    ("angle outside, about x", 0 * X, -A_OUT * X, ""),
    ("both inside", -D_IN * Y, A_IN * SKEW, ""),
    ("dist inside, angle outside", D_IN * Z, A_OUT * SKEW, ""),
    ("dist outside, angle inside", -D_OUT * Z, -A_IN * SKEW, ""),
    ("both outside", D_OUT * Y, -A_OUT * Y, ""),
    ("both inside, negated quaternion", 1e-3 * SKEW, 0.1 * Z, "neg"),
    ("angle inside, negated quaternion", 0 * X, A_IN * Y, "neg"),
    ("angle outside, negated quaternion", 0 * X, A_OUT * Y, "neg"),
    ("far away, at rest", 0 * X, 0 * Z, "rest"),
    ("half turn, yaw", 0 * X, np.pi * Z, ""),
    ("half turn, skew, negated quaternion", 1e-3 * X, np.pi * SKEW, "neg"),
    ("near pi, below", 0 * X, (np.pi - 1e-2) * Z, ""),
    ("near pi, beyond (the short way round is 1e-2 less)", 0 * X, (np.pi + 1e-2) * X, ""),
    ("near pi, 1e-4 below", 2e-3 * Y, (np.pi - 1e-4) * SKEW, ""),
    ("inserted 2 mm short", -2e-3 * X, 0.078 * Y, ""),
    ("tipped out", np.array([-0.03, 0.0, -0.05]), 0.5 * np.pi * Y, ""),
]
LABELS = [c[0] for c in TABLE]
# what each threshold case must give: label -> (dist <= thresh, angle <= thresh); None: not stated (the resting charger's
# yaw is the reset's draw, its distance alone decides)
WANT = {
    "identity": (True, True), "dist inside, along x": (True, True), "dist outside, along x": (False, True), "angle inside, yaw": (True, True),
    "angle outside, yaw": (True, False), "dist inside, skew": (True, True), "dist outside, skew": (False, True), "angle inside, about x": (True, True),
    "angle outside, about x": (True, False), "both inside": (True, True), "dist inside, angle outside": (True, False),
    "dist outside, angle inside": (False, True), "both outside": (False, False), "both inside, negated quaternion": (True, True),
    "angle inside, negated quaternion": (True, True), "angle outside, negated quaternion": (True, False), "far away, at rest": (False, None),
    "half turn, yaw": (True, False), "inserted 2 mm short": (True, True), "tipped out": (False, False),
}


def _rotvec_quat(v):
    a = np.linalg.norm(v)
    if a == 0:
        return np.array([1.0, 0, 0, 0])
    return np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * v / a])


def _rotate(q, v):
    return ref.quat_mul(ref.quat_mul(q, np.concatenate([[0.0], v])), ref.quat_conj(q))[1:]


def build_batch(S0, P, nan="charger"):
    """the table over the batch of snapshot S0: env e takes case e mod len(TABLE), composed with ITS goal in float64 and
    rounded to float32. The NaN pose goes to env NAN_CASE alone: into the charger's pose (nan="charger"), or, where the
    charger's pose is going to enter the simulation state, into the stored goal (nan="goal"). -> (S, labels)"""
    S = {k: v.copy() for k, v in S0.items()}
    N = S["goal"].shape[0]
    row, labels = P["charger_row"], []
    for e in range(N):
        label, off, rotvec, flag = TABLE[e % len(TABLE)]
        if flag == "nan" and e != NAN_CASE:
            label, off, rotvec, flag = TABLE[0]
        labels.append(label)
        if flag == "rest":
            continue
        g = S["goal"][e].astype(np.float64)
        q = ref.quat_mul(g[3:], _rotvec_quat(np.asarray(rotvec, np.float64)))
        pose = np.concatenate([g[:3] + _rotate(g[3:], np.asarray(off, np.float64)), -q if flag == "neg" else q])
        if flag == "nan" and nan == "charger":
            pose[:] = np.nan
        S["rigid"][row, e, :7] = pose.astype(f32)
        S["rigid"][row, e, 7:] = 0
        if flag == "nan" and nan == "goal":
            S["goal"][e] = np.nan
    return S, labels


def check_margins(R, labels):
    """every case with a stated side lies on it, no closer to a threshold than 8 x the measured float32 band"""
    for e, label in enumerate(labels):
        if label in WANT:
            for k, (want, ok) in enumerate(zip(WANT[label], (R["dist_ok"][e], R["angle_ok"][e]))):
                assert want is None or (bool(ok) == want and abs(R["margins"][e, k]) >= 8 * MEASURED), (e, label, k, R["margins"][e])


def tolerance():
    return 4 * MEASURED


def check(got, R, labels, tol, what):
    """`got` (obs [N, D] f32, reward [N], success [N] bool, metrics [N, 2]) against the reference R: success equal on EVERY
    env, observations bit for bit (a NaN matches a NaN), the reward zero, metrics within the tolerance and NaN exactly where
    the reference's are. -> (max dist difference, max angle difference)"""
    assert np.array_equal(got["success"], R["success"]), (what, [labels[e] for e in np.nonzero(got["success"] != R["success"])[0]])
    want_obs = R["obs"].astype(f32)
    assert got["obs"].dtype == f32 and got["obs"].shape == want_obs.shape, (what, got["obs"].shape)
    same = (got["obs"].view(np.uint32) == want_obs.view(np.uint32)) | (np.isnan(got["obs"]) & np.isnan(want_obs))
    assert same.all(), (what, "obs", np.argwhere(~same)[:4])
    assert np.all(got["reward"] == 0), (what, "reward")
    nan = np.isnan(R["metrics"])
    assert np.array_equal(np.isnan(got["metrics"]), nan), (what, "NaN metrics")
    d = np.where(nan, 0.0, np.abs(got["metrics"].astype(np.float64) - np.where(nan, 0.0, R["metrics"])))
    worst = d.max(0)
    assert worst.max() <= tol, (what, worst, labels[int(d[:, 0].argmax())], labels[int(d[:, 1].argmax())])
    return float(worst[0]), float(worst[1])


# ---- physics known answers, shared by the CPU and the GPU test -------------------------------------------------------------
SHORT = (0.0, 2e-3, 8e-3, 12e-3)  # how far short of the goal each env's charger is teleported (4 and 6 mm are marginal)


def teleport_short_of_goal(base, short=SHORT):
    """env e: the charger at its goal pose, backed out of the slots by short[e] along the goal's x axis, at rest"""
    from maniskill_amd.utils.structs.pose import Pose

    N = base.num_envs
    assert N == len(short)
    off = torch.zeros(N, 3, device=base.device)
    off[:, 0] = -torch.tensor(short, device=base.device)
    ident = torch.zeros(N, 4, device=base.device)
    ident[:, 0] = 1
    base.charger.set_pose(base.goal_pose * Pose.create_from_pq(off, ident))
    base.charger.set_linear_velocity(torch.zeros(N, 3, device=base.device))
    base.charger.set_angular_velocity(torch.zeros(N, 3, device=base.device))
    base.scene._gpu_apply_all()
    base.scene._gpu_fetch_all()


def check_plugged_rollout(env, steps=20):
    """zero actions from `teleport_short_of_goal`: the chargers at the goal and 2 mm short of it stay plugged (success at
    every step, at rest at the end), those 8 and 12 mm short tip out (no success from step 5 on, angle > 1 rad at the end)"""
    base = env.unwrapped
    a = torch.zeros(base.num_envs, 8, device=base.device)
    px = base.scene.px
    px.overflow_count()
    for step in range(1, steps + 1):
        _, _, _, _, info = env.step(a)
        ok = info["success"].cpu()
        assert ok[0] and ok[1], (step, info["obj_to_goal_dist"].cpu(), info["obj_to_goal_angle"].cpu())
        if step >= 5:
            assert not ok[2] and not ok[3], (step, info["obj_to_goal_dist"].cpu(), info["obj_to_goal_angle"].cpu())
    dist, angle = info["obj_to_goal_dist"].cpu(), info["obj_to_goal_angle"].cpu()
    speed = torch.linalg.norm(base.charger.linear_velocity, dim=1).cpu()
    print(f"\nafter {steps} zero-action steps, chargers {[1e3 * s for s in SHORT]} mm short: dist {[round(1e3 * float(d), 3) for d in dist]} mm, "
          f"angle {[round(float(x), 4) for x in angle]} rad, speed {[float(s) for s in speed]} m/s")
    assert speed[0] < 1e-3 and speed[1] < 1e-3
    assert angle[2] > 1 and angle[3] > 1
    assert px.overflow_count() == 0
    return dist, angle
