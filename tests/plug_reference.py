"""Float64 statement of the PlugCharger epilogue: plain numpy, written from the task definition (what the numbers mean),
not from the torch code or the kernel. The inputs are the float32 values the epilogue reads, promoted to float64.

The rotation angle is taken from the relative rotation itself: with r = conj(goal.q) * charger.q, the rotation that r
stands for turns by 2 atan2(|r.xyz|, |r.w|), a number in [0, pi] that r and -r share and that needs no unit norm (both
arguments scale alike). The torch path reaches it through an axis-angle vector and a min(a, 2 pi - a).

`outputs(S, P)`: S = dict(rigid [rows, N, 13], qpos [N, n], qvel [N, n], goal [N, 7]) float32; P = dict(tcp_row,
charger_row, receptacle_row, dist_thresh, angle_thresh, reward_scale). Returns obs [N, 2 n + 28] (qpos, qvel, tcp,
charger, receptacle and goal poses: all copies), reward [N] (zero), metrics [N, 2] = dist, angle, success [N] bool, and the
margins dist - dist_thresh and angle - angle_thresh that tell how far a case lies from either threshold."""
import numpy as np


def quat_mul(a, b):
    aw, ax, ay, az = (a[..., i] for i in range(4))
    bw, bx, by, bz = (b[..., i] for i in range(4))
    return np.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)


def quat_conj(q):
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def rotation_angle(q_goal, q_obj):
    """the angle in [0, pi] of the rotation that takes the goal's frame to the object's"""
    r = quat_mul(quat_conj(np.asarray(q_goal, np.float64)), np.asarray(q_obj, np.float64))
    return 2.0 * np.arctan2(np.linalg.norm(r[..., 1:], axis=-1), np.abs(r[..., 0]))


def evaluate(obj_pose, goal_pose, dist_thresh=5e-3, angle_thresh=0.2):
    """-> dist, angle, success; poses [..., 7] = p, q(wxyz). A NaN makes the comparison, hence success, false."""
    obj_pose, goal_pose = np.asarray(obj_pose, np.float64), np.asarray(goal_pose, np.float64)
    dist = np.linalg.norm(goal_pose[..., :3] - obj_pose[..., :3], axis=-1)
    angle = rotation_angle(goal_pose[..., 3:], obj_pose[..., 3:])
    with np.errstate(invalid="ignore"):
        success = (dist <= dist_thresh) & (angle <= angle_thresh)
    return dist, angle, success


def outputs(S, P):
    rigid = np.asarray(S["rigid"], np.float64)
    tcp, ch, rc = (rigid[P[k], :, :7] for k in ("tcp_row", "charger_row", "receptacle_row"))
    goal = np.asarray(S["goal"], np.float64)
    dist, angle, success = evaluate(ch, goal, P["dist_thresh"], P["angle_thresh"])
    obs = np.concatenate([np.asarray(S["qpos"], np.float64), np.asarray(S["qvel"], np.float64), tcp, ch, rc, goal], 1)
    with np.errstate(invalid="ignore"):
        dist_ok, angle_ok = dist <= P["dist_thresh"], angle <= P["angle_thresh"]
    return dict(obs=obs, reward=np.zeros(len(goal)) * P["reward_scale"], metrics=np.stack([dist, angle], 1), success=success,
                dist_ok=dist_ok, angle_ok=angle_ok, margins=np.stack([dist - P["dist_thresh"], angle - P["angle_thresh"]], 1))
