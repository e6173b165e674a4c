"""Constructed states for the RollBall and PullCube epilogues, one case per env index (the table repeats over the batch),
and the glue between an env (oracle-backed on the CPU, HIP on the GPU), tests/roll_pull_reference.py and the native task
structs. Test infrastructure only; snapshot / buffer helpers and the comparison are those of tests/task_cases.py.

Every case is built so that the float64 reference decides each predicate by at least MIN_MARGIN (thresholds are approached
to EDGE = 1e-3, absolute: float32 decides them). `check` compares an implementation with the reference and returns how
many envs it had to leave out, which the tests assert to be 0."""
import numpy as np
import torch

import maniskill_amd.envs  # noqa: F401
from tests import task_cases as tc
from tests.task_cases import DIAG, _set, f32

ENV_IDS = dict(roll="RollBall-v1", pull="PullCube-v1")
TOP_REWARD = dict(roll=30.0, pull=3.0)
OBS_EXTRA = dict(roll=26, pull=17)
EDGE = 1e-3
MIN_MARGIN = 1e-4

# max |torch f32 path (CPU) - f64 reference| of the reward over the case tables, recorded from the output of
# tests/test_roll_pull.py::test_torch_path_matches_reference (which asserts that they still bound what it measures),
# rounded up:
#   dense reward       roll 6.80e-7, pull 7.10e-8
#   normalised reward  roll 5.22e-8, pull 4.00e-8
MEASURED = dict(roll=6.8e-7, pull=7.2e-8)
MEASURED_NORMALIZED = dict(roll=5.3e-8, pull=4.0e-8)


def make_env(task, N, backend, seed=7, **kw):
    import gymnasium as gym

    env = gym.make(ENV_IDS[task], num_envs=N, sim_backend=backend, **kw)
    env.reset(seed=seed)
    return env


def snapshot(base, task):
    S = tc.snapshot(base)
    if task == "roll":
        S["reached"] = base.reached_status.detach().cpu().numpy().astype(f32).copy()
    return S


def params(task, base, normalized=False):
    """task parameters as the env's own fused path states them; every float rounded to float32, the value the native
    struct carries"""
    a = base.agent
    r = lambda o: int(o._body_row)
    F = lambda x: float(f32(x))
    scale = F(1 / TOP_REWARD[task]) if normalized else F(1)
    if task == "roll":
        return dict(tcp_row=r(a.tcp), ball_row=r(base.ball), goal_row=r(base.goal_region), goal_radius=F(base.goal_radius), ball_radius=F(base.ball_radius),
                    hit_offset=F(base.hit_offset), reach_thresh=F(base.reach_thresh), reward_scale=scale, update_reached=1)
    return dict(tcp_row=r(a.tcp), obj_row=r(base.obj), goal_row=r(base.goal_region), goal_radius=F(base.goal_radius), cube_half_size=F(base.cube_half_size),
                reward_scale=scale)


def native_task(task, P, reached=None):
    """the ctypes struct of `P`; `reached`: the device latch tensor RollBall's struct points to (kept by the caller)"""
    from maniskill_amd import native

    if task == "roll":
        return native.RollTask(**P, reached=reached.data_ptr())
    return native.PullTask(**P)


def torch_outputs(task, base, S):
    """the torch path on the env's current buffers (and, RollBall, the latch of S): what `check` takes"""
    if task == "roll":
        base.reached_status[:] = torch.from_numpy(S["reached"]).to(base.device)
    info = base.evaluate()
    obs = base.get_obs(info)
    rew = base.get_reward(obs=obs, action=None, info=info)
    out = dict(obs=obs.cpu().numpy(), reward=rew.cpu().numpy(), flags=dict(success=info["success"].cpu().numpy().astype(bool)))
    if task == "roll":
        out["reached"] = base.reached_status.cpu().numpy().copy()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# case tables: (label, fn(S, e, link_rows)); link_rows=False leaves the tcp row alone (the copy-out form recomputes the link
# rows from qpos: there the tcp stays where the arm is, half a metre from either task's point)
def _cases_roll(P):
    t, b, g = P["tcp_row"], P["ball_row"], P["goal_row"]
    rad, thr, off = P["goal_radius"], P["reach_thresh"], float(P["ball_radius"]) + float(P["hit_offset"])

    def state(d_hit, latch, d_goal=None, above=False):
        """the tcp at distance d_hit from the hit point; the goal moved to d_goal from the ball in xy (None: where the reset put
        it, more than a metre away; above: exactly under the ball's centre)"""
        def f(S, e, link_rows):
            pb = S["rigid"][b, e, :3].astype(np.float64)
            if above:
                _set(S, g, e, p=[pb[0], pb[1], 1e-3])
            elif d_goal is not None:
                _set(S, g, e, p=[pb[0] + 0.6 * d_goal, pb[1] - 0.8 * d_goal, 1e-3])
            away = pb - S["rigid"][g, e, :3].astype(np.float64)
            hit = pb + away / np.linalg.norm(away) * off
            if link_rows:
                _set(S, t, e, p=hit + d_hit * DIAG)
            S["reached"][e] = latch
        return f

    return [
        ("far, latch 0", state(0.3, 0)),
        ("hit distance inside", state(thr - EDGE, 0)),
        ("hit distance outside", state(thr + EDGE, 0)),
        ("latch 1, tcp far", state(0.3, 1)),
        ("latch 1, tcp at the hit point", state(0.5 * thr, 1)),
        ("success, latch 0", state(0.3, 0, d_goal=0.5 * rad)),
        ("success, latch 1", state(0.3, 1, d_goal=0.5 * rad)),
        ("above the goal centre", state(0.3, 0, above=True)),
        ("above the goal centre, tcp at the hit point", state(thr - EDGE, 0, above=True)),
        ("goal radius inside", state(0.3, 1, d_goal=rad - EDGE)),
        ("goal radius outside", state(0.3, 1, d_goal=rad + EDGE)),
        ("goal radius outside, latch 0", state(thr + EDGE, 0, d_goal=rad + EDGE)),
    ]


FLIPS = ("hit distance inside", "above the goal centre, tcp at the hit point")  # the cases whose latch goes 0 -> 1


def _cases_pull(P):
    t, o, g = P["tcp_row"], P["obj_row"], P["goal_row"]
    rad, half = P["goal_radius"], float(P["cube_half_size"])

    def state(d_pull, d_goal, z=None):
        def f(S, e, link_rows):
            po = S["rigid"][o, e, :3].astype(np.float64)
            if z is not None:
                po[2] = z
                _set(S, o, e, p=po)
                po = S["rigid"][o, e, :3].astype(np.float64)
            _set(S, g, e, p=[po[0] - 0.6 * d_goal, po[1] + 0.8 * d_goal, 1e-3])
            if link_rows:
                _set(S, t, e, p=po + np.array([half + 0.01, 0, 0]) + d_pull * DIAG)
        return f

    return [
        ("far, outside", state(0.05, 2 * rad)),
        ("pull distance inside", state(0.01 - EDGE, 2 * rad)),
        ("pull distance outside", state(0.01 + EDGE, 2 * rad)),
        ("goal radius inside", state(0.05, rad - EDGE)),
        ("goal radius outside", state(0.05, rad + EDGE)),
        ("success, not reached", state(0.05, 0.5 * rad)),
        ("success, reached", state(0.004, 0.5 * rad)),
        ("reached, goal radius outside", state(0.004, rad + EDGE)),
        ("inside, lifted (no height condition)", state(0.05, 0.5 * rad, z=half + 0.06)),
    ]


TABLES = dict(roll=_cases_roll, pull=_cases_pull)


def build_batch(task, S0, P, start=0, link_rows=True):
    """-> (S, labels): env e holds case (start + e) modulo the table's length, built on the state env e has in S0"""
    S = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in S0.items()}
    C = TABLES[task](P)
    N = S["qpos"].shape[0]
    labels = []
    for e in range(N):
        label, fn = C[(start + e) % len(C)]
        fn(S, e, link_rows)
        labels.append(label)
    return S, labels


def write_buffers(base, S):
    tc.write_buffers(base, S)


# ---------------------------------------------------------------------------------------------------------------------
def tolerance(task, P):
    """4 x the measured difference of the torch path and the reference, for the dense or the normalised reward"""
    f = P["reward_scale"]
    assert f == 1.0 or abs(f * TOP_REWARD[task] - 1) < 1e-6
    return 4 * (MEASURED if f == 1.0 else MEASURED_NORMALIZED)[task]


def check(task, got, R, labels, tol_reward, what):
    """`got` (obs, reward, flags{success}, RollBall: reached) against the reference's result: flags equal, copied / single
    subtraction observation entries bit-exact, rewards within tol_reward, the latch equal. Every predicate of every env
    must be decided by MIN_MARGIN. Returns (measured reward difference, number of envs left out)."""
    for name, (m, band) in R["margins"].items():
        small = np.nonzero(np.abs(m) < MIN_MARGIN)[0]
        assert len(small) == 0, (what, task, name, "decided by less than MIN_MARGIN", [(int(e), labels[e], float(m[e])) for e in small[:4]])
    excluded = int((~R["reward_decided"]).sum() + sum(int((~d).sum()) for d in R["decided"].values()))
    out = tc.compare(task, got, R, labels, tol_reward, what=what)
    if task == "roll":
        excluded += int((~R["reached_decided"]).sum())
        bad = np.nonzero(got["reached"].astype(np.float64) != R["reached_new"])[0]
        assert len(bad) == 0, (what, "latch", [(int(e), labels[e], float(got["reached"][e]), float(R["reached_new"][e])) for e in bad[:4]])
    return out["reward"], excluded
