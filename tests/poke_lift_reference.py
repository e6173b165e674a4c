"""Float64 statement of the PokeCube and LiftPegUpright epilogues: plain numpy, written from the task definitions (what
envs/tasks/tabletop/poke_cube.py and lift_peg_upright.py restate) and Panda.is_grasping / is_static, independent of both
the torch path and the HIP kernels. Test infrastructure only; the conventions are those of tests/task_reference.py
(snapshot `S`, parameters `P`, three-valued predicates with their margins), whose helpers it uses.

Both return the dict of task_reference._finish: obs, exact, reward, flags, decided, margins {predicate: (margin, band)},
reward_decided; and `hypot` [N]: the smallest hypot(R00, R01) over the orientations whose angle atan2(-R01, R00) the task
reads (below 0.1 that angle is ill-conditioned in any precision; the case builder asserts it stays above). PokeCube adds
`metrics` [N, 2] = angle_diff, head_to_cube_dist."""
import numpy as np

from tests.task_reference import _and, _f64, _finish, _norm, _pred, _val, grasp, pose_mul


def rot_entries(q):
    """(R00, R01, R20) of a quaternion's rotation matrix (wxyz), the entries scaled by 2 / |q|^2: no unit norm assumed"""
    q = np.asarray(q, np.float64)
    w, x, y, z = q.T
    two_s = 2.0 / (q * q).sum(-1)
    return 1 - two_s * (y * y + z * z), two_s * (x * y - z * w), two_s * (x * z - y * w)


def euler_z(q):
    """the third angle of the XYZ Tait-Bryan decomposition R = Rx(a) Ry(b) Rz(c): c = atan2(-R01, R00); and hypot(R00, R01)"""
    r00, r01, _ = rot_entries(q)
    return np.arctan2(-r01, r00), np.hypot(r00, r01)


def poke(S, P):
    """PokeCube. head position = peg + (half_length, 0, 0), unrotated; head pose = peg * (half_length, 0, 0), of which only
    the quaternion is read. angle_diff = |c(head pose) - c(cube)|, not wrapped; head_to_cube_dist = |head - cube|_xy.
    placed = |cube - goal|_xy < goal_radius; fit = angle_diff < 0.05 and head_to_cube_dist <= half + 0.005;
    static = max |qvel[:n_static]| <= 0.2; success = placed and static.
    r = 2 (1 - tanh 5 |tcp - peg|); grasped and |tcp - peg| < 0.01: 4 + (1 - tanh 5 head_to_cube_dist) + (1 - tanh 5
    angle_diff); and fit: 7 + (1 - tanh 5 |goal - cube|); placed: + 1 - tanh 5 |qvel[:n_static]|; success: 10."""
    S = _f64(S)
    R, qpos, qvel = S["rigid"], S["qpos"], S["qvel"]
    N = qpos.shape[0]
    tcp, peg, cube, goal = R[P["tcp_row"]], R[P["peg_row"]], R[P["cube_row"]], R[P["goal_row"]]
    hl = float(P["peg_half_length"])
    m = {}
    grasped, lflag, rflag, forces = grasp(S, m, P["peg_row"], P["finger1_row"], P["finger2_row"], P["min_force"], P["max_angle_deg"])
    off = (np.tile([hl, 0.0, 0.0], (N, 1)), np.tile([1.0, 0, 0, 0], (N, 1)))
    head_p = peg[:, :3] + off[0]
    head_q = pose_mul((peg[:, :3], peg[:, 3:7]), off)[1]
    c_head, h_head = euler_z(head_q)
    c_cube, h_cube = euler_z(cube[:, 3:7])
    angle_diff = np.abs(c_head - c_cube)
    head_to_cube = _norm(head_p[:, :2] - cube[:, :2])
    placed = _pred(m, "placed", _norm(cube[:, :2] - goal[:, :2]), P["goal_radius"], "<")
    aligned = _pred(m, "aligned", angle_diff, P["align_thresh"], "<")
    close = _pred(m, "close", head_to_cube, float(P["cube_half_size"]) + 0.005, "<=")
    fit = _and(aligned, close)
    qs = qvel[:, : P["n_static_dofs"]]
    static = _pred(m, "static", np.abs(qs).max(1), P["static_thresh"], "<=")
    success = _and(placed, static)
    d_tcp = _norm(tcp[:, :3] - peg[:, :3])
    reached = _pred(m, "reached", d_tcp, P["reach_thresh"], "<")
    held = _and(grasped, reached)
    # the head's position is a float32 quantity of the observation (peg + offset, rounded, before the cube is subtracted):
    # with that rounding stated, every column is a copy or one subtraction of float32 values
    head32 = (peg[:, :3].astype(np.float32) + np.array([hl, 0, 0], np.float32)).astype(np.float64)
    obs = np.concatenate([qpos, qvel, tcp[:, :7], cube[:, :7], peg[:, :7], peg[:, :3], peg[:, :3] - tcp[:, :3], cube[:, :3] - peg[:, :3],
                          goal[:, :3] - cube[:, :3], head32 - cube[:, :3]], 1)
    r = 2 * (1 - np.tanh(5 * d_tcp))
    r = np.where(_val(held), 4 + (1 - np.tanh(5 * head_to_cube)) + (1 - np.tanh(5 * angle_diff)), r)
    r = np.where(_val(fit) & _val(held), 7 + (1 - np.tanh(5 * _norm(goal[:, :3] - cube[:, :3]))), r)
    r = r + np.where(_val(placed), 1 - np.tanh(5 * _norm(qs)), 0.0)
    r = np.where(_val(success), 10.0, r) * P["reward_scale"]
    flags = dict(success=success, is_cube_placed=placed, is_peg_cube_fit=fit, is_peg_grasped=grasped, left=lflag, right=rflag, aligned=aligned,
                 close=close, static=static, reached=reached, held=held)
    return _finish(obs, np.ones(obs.shape[1], bool), r, flags, m, ("success", "is_cube_placed", "is_peg_cube_fit", "held"),
                   dict(metrics=np.stack([angle_diff, head_to_cube], 1), hypot=np.minimum(h_head, h_cube), forces=forces))


def lift(S, P):
    """LiftPegUpright. success = | |c(peg)| - pi/2 | < 0.08 and |peg_z - half_length| < 0.005, c the third XYZ angle.
    r = |R20| (the z component of the peg's x axis) + (1 - tanh 5 |peg_z - half_length|) + g / 5 with g = 1 where the peg is
    grasped, else 1 - tanh 5 |peg - tcp|; success: 3."""
    S = _f64(S)
    R, qpos, qvel = S["rigid"], S["qpos"], S["qvel"]
    tcp, peg = R[P["tcp_row"]], R[P["peg_row"]]
    m = {}
    grasped, lflag, rflag, forces = grasp(S, m, P["peg_row"], P["finger1_row"], P["finger2_row"], P["min_force"], P["max_angle_deg"])
    c, h = euler_z(peg[:, 3:7])
    upright = _pred(m, "upright", np.abs(np.abs(c) - np.pi / 2), P["upright_thresh"], "<")
    z_dist = np.abs(peg[:, 2] - float(P["peg_half_length"]))
    low = _pred(m, "close_to_table", z_dist, P["height_thresh"], "<")
    success = _and(upright, low)
    obs = np.concatenate([qpos, qvel, tcp[:, :7], peg[:, :7]], 1)
    r = np.abs(rot_entries(peg[:, 3:7])[2]) + (1 - np.tanh(5 * z_dist))
    r = r + np.where(_val(grasped), 1.0, 1 - np.tanh(5 * _norm(peg[:, :3] - tcp[:, :3]))) / 5
    r = np.where(_val(success), 3.0, r) * P["reward_scale"]
    flags = dict(success=success, upright=upright, close_to_table=low, is_grasped=grasped, left=lflag, right=rflag)
    return _finish(obs, np.ones(obs.shape[1], bool), r, flags, m, ("success", "is_grasped"), dict(hypot=h, forces=forces))


TASKS = dict(poke=poke, lift=lift)
