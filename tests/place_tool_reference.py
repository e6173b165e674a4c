"""Float64 statement of the PlaceSphere and PullCubeTool epilogues: plain numpy, written from the task definitions (what
envs/tasks/tabletop/place_sphere.py and pull_cube_tool.py restate) and Panda.is_grasping / is_static, Actor.is_static,
independent of both the torch path and the HIP kernels. Test infrastructure only; the conventions are those of
tests/task_reference.py (snapshot `S`, parameters `P`, three-valued predicates with their margins), whose helpers it uses.

Both return the dict of task_reference._finish: obs, exact, reward, flags, decided, margins {predicate: (margin, band)},
reward_decided, forces. PullCubeTool adds `metrics` [N, 3] = cube_to_workspace_dist, 1 - tanh 3 cube_to_workspace_dist,
dense reward / 5 (whatever reward_scale is: the `reward` entry of the task's info)."""
import numpy as np

from tests.task_reference import BAND, Tri, _and, _f64, _finish, _norm, _not, _pred, _val, grasp


def place(S, P):
    """PlaceSphere. off = obj - bin; on_bin = |off|_xy <= tol and |off_z - radius - bin_base_half| <= tol;
    static = |v| <= lin and |w| <= ang; success = on_bin and static and not grasped.
    r = 2 (1 - tanh 5 |tcp - obj|); grasped: 4 + (1 - tanh 5 |bin + (bin_base_half + radius) z - obj|); on_bin: 6 +
    (ungrasp + (1 - tanh(10 |v| + |w|)) + robot_static) / 3, ungrasp = (the two finger joints' sum) / gripper_width if
    grasped else 16, robot_static = 1 where max |qvel[:n_static]| <= robot_static_thresh else 0; success: 13."""
    S = _f64(S)
    R, qpos, qvel = S["rigid"], S["qpos"], S["qvel"]
    tcp, obj, bn = R[P["tcp_row"]], R[P["obj_row"]], R[P["bin_row"]]
    rad, bh, tol = float(P["radius"]), float(P["bin_base_half"]), float(P["on_bin_tol"])
    m = {}
    grasped, lflag, rflag, forces = grasp(S, m, P["obj_row"], P["finger1_row"], P["finger2_row"], P["min_force"], P["max_angle_deg"])
    off = obj[:, :3] - bn[:, :3]
    on_xy = _pred(m, "on_xy", _norm(off[:, :2]), tol, "<=")
    on_z = _pred(m, "on_z", np.abs(off[:, 2] - rad - bh), tol, "<=")
    # (the z predicate subtracts two lengths from a difference of heights: its band is that of the operands)
    m["on_z"] = (m["on_z"][0], BAND * (np.abs(obj[:, 2]) + np.abs(bn[:, 2]) + rad + bh + tol))
    und = np.abs(m["on_z"][0]) <= m["on_z"][1]
    ex = _val(on_z)
    on_z = Tri(ex & ~und, ex | und)
    on_z._exact = ex
    on = _and(on_xy, on_z)
    v, av = _norm(obj[:, 7:10]), _norm(obj[:, 10:13])
    lin = _pred(m, "static_lin", v, P["static_lin_thresh"], "<=")
    ang = _pred(m, "static_ang", av, P["static_ang_thresh"], "<=")
    static = _and(lin, ang)
    success = _and(_and(on, static), _not(grasped))
    robot_static = _pred(m, "robot_static", np.abs(qvel[:, : P["n_static_dofs"]]).max(1), P["robot_static_thresh"], "<=")
    g = _val(grasped)
    obs = np.concatenate([qpos, qvel, g[:, None].astype(np.float64), tcp[:, :7], bn[:, :3], obj[:, :7], obj[:, :3] - tcp[:, :3]], 1)
    r = 2 * (1 - np.tanh(5 * _norm(tcp[:, :3] - obj[:, :3])))
    top = bn[:, :3] + np.array([0.0, 0.0, bh + rad])
    r = np.where(g, 4 + (1 - np.tanh(5 * _norm(top - obj[:, :3]))), r)
    ungrasp = np.where(g, (qpos[:, -2] + qpos[:, -1]) / P["gripper_width"], 16.0)
    r = np.where(_val(on), 6 + (ungrasp + (1 - np.tanh(10 * v + av)) + _val(robot_static).astype(np.float64)) / 3, r)
    r = np.where(_val(success), 13.0, r) * P["reward_scale"]
    # (the robot's is_static is read by the reward on the bin only, and not where success writes over it)
    reads_rs = Tri(robot_static.lo | ~on.hi | success.lo, robot_static.hi | ~on.hi | success.lo)
    reads_rs._exact = _val(robot_static)
    flags = dict(success=success, is_obj_grasped=grasped, is_obj_on_bin=on, is_obj_static=static, left=lflag, right=rflag, on_xy=on_xy, on_z=on_z,
                 static_lin=lin, static_ang=ang, robot_static=robot_static, robot_static_if_read=reads_rs)
    return _finish(obs, np.ones(obs.shape[1], bool), r, flags, m, ("success", "is_obj_grasped", "is_obj_on_bin", "robot_static_if_read"), dict(forces=forces))


def pulltool(S, P):
    """PullCubeTool. success = |cube - base|_xy < pulled_close_dist; d_w = |cube - (base + (0.1 arm_reach, 0, 0))|.
    d_t = |tcp - (tool + (0.02, 0, 0))|; g = is_grasping(tool, max_angle_deg); d_p = |tool - (cube + (-(hook_length +
    cube_half_size), -0.067, 0))|, positioned = d_p < 0.05; target = base + (0.05, 0, 0), d_c = |cube - target|, d_0 =
    |(arm_reach + 0.1, 0, cube_size / 2) - target|.
    r = 2 (1 - tanh 5 d_t) + 2 g + 1.5 (1 - tanh 3 d_p) g + 3 (d_0 - d_c) / d_0 positioned g; cube_x > arm_reach + 0.15:
    - 2; success: + 5."""
    S = _f64(S)
    R, qpos, qvel = S["rigid"], S["qpos"], S["qvel"]
    tcp, cube, tool, base = R[P["tcp_row"]][:, :3], R[P["cube_row"]][:, :3], R[P["tool_row"]][:, :3], R[P["base_row"]][:, :3]
    reach, hook, half, size = (float(P[k]) for k in ("arm_reach", "hook_length", "cube_half_size", "cube_size"))
    m = {}
    grasped, lflag, rflag, forces = grasp(S, m, P["tool_row"], P["finger1_row"], P["finger2_row"], P["min_force"], P["max_angle_deg"])
    success = _pred(m, "pulled_close", _norm(cube[:, :2] - base[:, :2]), P["pulled_close_dist"], "<")
    d_w = _norm(cube - (base + np.array([0.1 * reach, 0.0, 0.0])))
    progress = 1 - np.tanh(3 * d_w)
    d_t = _norm(tcp - (tool + np.array([0.02, 0.0, 0.0])))
    d_p = _norm(tool - (cube + np.array([-(hook + half), -0.067, 0.0])))
    positioned = _pred(m, "positioned", d_p, 0.05, "<")
    target = base + np.array([0.05, 0.0, 0.0])
    d_c = _norm(cube - target)
    d_0 = _norm(np.array([reach + 0.1, 0.0, size / 2]) - target)
    pushed = _pred(m, "pushed_away", cube[:, 0], reach + 0.15, ">=")
    # (strictly greater: `>=` with the margin recorded; the two differ at equality only, which MIN_MARGIN excludes)
    pushed._exact = cube[:, 0] > reach + 0.15
    g = _val(grasped).astype(np.float64)
    r = 2 * (1 - np.tanh(5 * d_t)) + 2 * g
    r = r + 1.5 * (1 - np.tanh(3 * d_p)) * g
    r = r + 3 * ((d_0 - d_c) / d_0) * _val(positioned) * g
    r = r - np.where(_val(pushed), 2.0, 0.0)
    r = r + np.where(_val(success), 5.0, 0.0)
    R7 = lambda k: R[P[k]][:, :7]
    obs = np.concatenate([qpos, qvel, R7("tcp_row"), R7("cube_row"), R7("tool_row")], 1)
    # (ungrasped: the positioning predicate is not read)
    reads_pos = Tri(positioned.lo | ~grasped.hi, positioned.hi | ~grasped.hi)
    reads_pos._exact = _val(positioned)
    flags = dict(success=success, is_grasped=grasped, left=lflag, right=rflag, positioned=positioned, pushed_away=pushed, positioned_if_grasped=reads_pos)
    return _finish(obs, np.ones(obs.shape[1], bool), r * P["reward_scale"], flags, m, ("success", "is_grasped", "positioned_if_grasped", "pushed_away"),
                   dict(metrics=np.stack([d_w, progress, r / 5], 1), forces=forces))


TASKS = dict(place=place, tool=pulltool)
