"""Float64 statement of the RollBall and PullCube epilogues: plain numpy, written from what the task classes
(envs/tasks/tabletop/roll_ball.py, pull_cube.py) state, independent of both the torch path and the HIP kernels. Test
infrastructure only; the conventions are those of tests/task_reference.py (snapshot `S`, parameters `P`, three-valued
predicates with their margins), whose helpers it uses.

  S["rigid"] [R, N, 13], S["qpos"], S["qvel"] [N, n_dof]  as in tests/task_reference.py
  S["reached"] [N]   RollBall's latch before the call (0 or 1)

Both return the dict of task_reference._finish: obs, exact, reward, flags, decided, margins {predicate: (margin, band)},
reward_decided. RollBall adds `reached_new` [N] (the latch after the call) and `reached_decided` [N]."""
import numpy as np

from tests.task_reference import _and, _f64, _finish, _norm, _pred, _val, Tri


def roll(S, P):
    """RollBall: success = |ball - goal|_xy < goal_radius. u = (ball - goal) / |ball - goal|, hit = ball + u (ball_radius +
    hit_offset), d = |hit - tcp|. With update_reached and d < reach_thresh the latch becomes 1. With the latch L after
    that: r = 20 (1 - tanh |ball - goal|_xy) L + (1 - tanh 2 d) (1 - L) + L; success: 30; times reward_scale."""
    latch = np.asarray(S["reached"], np.float64)
    S = _f64(S)
    R, qpos, qvel = S["rigid"], S["qpos"], S["qvel"]
    tcp, ball, goal = R[P["tcp_row"]], R[P["ball_row"]], R[P["goal_row"]]
    m = {}
    d_xy = _norm(ball[:, :2] - goal[:, :2])
    success = _pred(m, "inside", d_xy, P["goal_radius"], "<")
    away = ball[:, :3] - goal[:, :3]
    unit = away / _norm(away)[:, None]
    hit = ball[:, :3] + unit * (float(P["ball_radius"]) + float(P["hit_offset"]))
    d = _norm(hit - tcp[:, :3])
    at_hit = _pred(m, "at_hit", d, P["reach_thresh"], "<")
    update = bool(P.get("update_reached", 1))
    new = np.where(update & _val(at_hit), 1.0, latch)
    # the latch is decided where the predicate is, or where it cannot change anything (no update, latch already 1)
    latch_decided = at_hit.decided | (not update) | (latch == 1.0)
    obs = np.concatenate([qpos, qvel, tcp[:, :7], goal[:, :3], ball[:, :7], ball[:, 7:10], ball[:, :3] - tcp[:, :3], goal[:, :3] - ball[:, :3]], 1)
    r = 20 * (1 - np.tanh(d_xy)) * new + (1 - np.tanh(2 * d)) * (1 - new) + new
    r = np.where(_val(success), 30.0, r) * P["reward_scale"]
    moves = Tri(latch_decided, np.ones_like(latch_decided))  # (carried as a flag so that reward_decided reads it)
    moves._exact = np.ones_like(latch_decided)
    out = _finish(obs, np.ones(obs.shape[1], bool), r, dict(success=success, at_hit=at_hit, latch=moves), m, ("success", "latch"),
                  dict(reached_new=new, reached_decided=latch_decided, dist=d, d_xy=d_xy))
    return out


def pull(S, P):
    """PullCube: success = |obj - goal|_xy < goal_radius (no height condition). Reward: 1 - tanh 5 d with d the distance
    of the tcp to the pull point obj + (half + 10 mm) x; d < 0.01: + 1 - tanh 5 |obj - goal|_xy; success: 3."""
    S = _f64(S)
    R, qpos, qvel = S["rigid"], S["qpos"], S["qvel"]
    tcp, obj, goal = R[P["tcp_row"]], R[P["obj_row"]], R[P["goal_row"]]
    m = {}
    half = float(P["cube_half_size"])
    d_xy = _norm(obj[:, :2] - goal[:, :2])
    success = _pred(m, "inside", d_xy, P["goal_radius"], "<")
    pull_p = obj[:, :3] + np.array([half + 0.01, 0.0, 0.0])
    dist = _norm(pull_p - tcp[:, :3])
    reached = _pred(m, "reached", dist, 0.01, "<")
    obs = np.concatenate([qpos, qvel, tcp[:, :7], goal[:, :3], obj[:, :7]], 1)
    r = 1 - np.tanh(5 * dist) + np.where(_val(reached), 1 - np.tanh(5 * d_xy), 0.0)
    r = np.where(_val(success), 3.0, r) * P["reward_scale"]
    return _finish(obs, np.ones(obs.shape[1], bool), r, dict(success=success, reached=reached), m, ("success", "reached"), dict(dist=dist, d_xy=d_xy))


TASKS = dict(roll=roll, pull=pull)
