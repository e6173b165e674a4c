"""Float64 statement of what the Fetch changes in the task epilogues, in plain numpy, written from Fetch.is_grasping /
Fetch.is_static (agents/robots/fetch/fetch.py) and from the one reward that names a robot (pick_cube.py), independent of
both the torch path and the HIP kernels. Test infrastructure only; conventions (snapshot `S`, parameters `P`, the result
dict, three-valued predicates) are those of tests/task_reference.py.

The three robot-dependent rules:

  grasp    the force on the LEFT finger within max_angle of -y(l_gripper_finger_link), the force on the RIGHT finger within
           max_angle of +y(r_gripper_finger_link), each of at least min_force (the Panda: +y of its finger 1, -y of its finger 2)
  static   all(qvel[3:n-2] <= threshold) and all(qvel[:3] <= 0.05): SIGNED comparisons -- a joint moving fast in the
           negative direction counts as static -- and the two gripper joints are not read (the Panda: max |qvel[:n-2]| <=
           threshold)
  norm     PickCube's static reward takes |qvel[:n-2]| for the robot "panda" and |qvel| (all n joints) for any other; every
           other task slices [:n-2] for every robot

`evaluate(task, S, P)` composes them with the task references that exist (tests/task_reference.py, poke_lift_reference.py,
place_tool_reference.py). Those compute the Panda's rules from the snapshot themselves, so the composition is:
  * the grasp: the existing reference is called with the right finger as its finger 1 and the left as its finger 2, and its
    per-finger flags are asserted to equal fetch_grasp's, which is written from the Fetch's rule directly;
  * the static rule: the existing reference is called with a threshold no velocity meets (-1: its own static flag is false
    everywhere, so its reward is the one before the success overwrite) -- for PlaceSphere also with one every velocity
    meets -- and the Fetch's flag then selects, per env, what the task definition selects with it.
"""
import numpy as np

from tests import place_tool_reference as ptr
from tests import poke_lift_reference as plr
from tests import task_reference as tr
from tests.task_reference import Tri, _and, _angle_deg, _norm, _pred, _val, _y_axis, finger_forces

BASE_THRESHOLD = 0.05
TOP_REWARD = dict(pick=5.0, stack=8.0, poke=10.0, lift=3.0, place=13.0, tool=5.0)
BASE_REFERENCE = dict(pick=tr.pick, stack=tr.stack, poke=plr.poke, lift=plr.lift, place=ptr.place, tool=ptr.pulltool)
GRASPED_OBJECT = dict(pick="obj_row", stack="cubeA_row", poke="peg_row", lift="peg_row", place="obj_row", tool="tool_row")
GRASP_FLAG = dict(pick="is_grasped", stack="is_cubeA_grasped", poke="is_peg_grasped", lift="is_grasped", place="is_obj_grasped", tool="is_grasped")


def fetch_grasp(S, margins, obj_row, left_row, right_row, min_force=0.5, max_angle_deg=85.0):
    """Fetch.is_grasping -> (grasped, left flag, right flag) as three-valued predicates"""
    S = tr._f64(S)
    lf, rf = finger_forces(S, obj_row, left_row, right_row)
    ldir, rdir = -_y_axis(S["rigid"][left_row][:, 3:7]), _y_axis(S["rigid"][right_row][:, 3:7])
    lflag = _and(_pred(margins, "fetch_left_force", _norm(lf), min_force, ">="), _pred(margins, "fetch_left_angle", _angle_deg(ldir, lf), max_angle_deg, "<="))
    rflag = _and(_pred(margins, "fetch_right_force", _norm(rf), min_force, ">="), _pred(margins, "fetch_right_angle", _angle_deg(rdir, rf), max_angle_deg, "<="))
    return _and(lflag, rflag), lflag, rflag


def fetch_static(qvel, margins, threshold=0.2, base_threshold=BASE_THRESHOLD):
    """Fetch.is_static: signed; qvel [N, n]"""
    qvel = np.asarray(qvel, np.float64)
    n = qvel.shape[1]
    # all(x <= t) is max(x) <= t (no absolute value)
    body = _pred(margins, "fetch_static_body", qvel[:, 3 : n - 2].max(1), threshold, "<=")
    base = _pred(margins, "fetch_static_base", qvel[:, :3].max(1), base_threshold, "<=")
    return _and(body, base)


def reward_norm_dofs(task, robot_uid, n_dof):
    """how many leading joints the velocity norm of a task's static reward covers (PickCube and PokeCube have one)"""
    if task == "pick":
        return n_dof - 2 if robot_uid == "panda" else n_dof
    return n_dof - 2


def evaluate(task, S, P):
    """the epilogue of `task` for a Fetch. P: the task's parameters as its native record carries them, with the Fetch's
    fingers under `left_row` / `right_row` instead of finger1_row / finger2_row, `static_thresh` (pick, poke) or
    `robot_static_thresh` (place) as the task passes it to is_static, and no n_static_dofs (the rules above fix it)."""
    n = np.asarray(S["qpos"]).shape[1]
    Pb = {k: v for k, v in P.items() if k not in ("left_row", "right_row")}
    Pb.update(finger1_row=P["right_row"], finger2_row=P["left_row"])
    top = TOP_REWARD[task] * float(P["reward_scale"])
    if task in ("pick", "poke"):
        R = BASE_REFERENCE[task](S, {**Pb, "n_static_dofs": reward_norm_dofs(task, "fetch", n), "static_thresh": -1.0})
    elif task == "place":
        R = BASE_REFERENCE[task](S, {**Pb, "n_static_dofs": n - 2, "robot_static_thresh": -1.0})
        R1 = BASE_REFERENCE[task](S, {**Pb, "n_static_dofs": n - 2, "robot_static_thresh": 1e30})
    else:
        R = BASE_REFERENCE[task](S, Pb)
    m = R["margins"]
    # the grasp, stated from the Fetch's rule, against the composed one
    grasped, lflag, rflag = fetch_grasp(S, m, P[GRASPED_OBJECT[task]], P["left_row"], P["right_row"], P["min_force"], P["max_angle_deg"])
    assert np.array_equal(_val(lflag), R["flags"]["right"]) and np.array_equal(_val(rflag), R["flags"]["left"]), "finger order of the composition"
    assert np.array_equal(_val(grasped), R["flags"][GRASP_FLAG[task]])
    R["flags"].update(fetch_left=_val(lflag), fetch_right=_val(rflag))
    if task in ("pick", "poke", "place"):
        static = fetch_static(S["qvel"], m, P["static_thresh" if task != "place" else "robot_static_thresh"])
        R["flags"]["fetch_static"], R["decided"]["fetch_static"] = _val(static), static.decided
    if task in ("pick", "poke"):
        placed_name = "is_obj_placed" if task == "pick" else "is_cube_placed"
        placed = Tri(R["flags"][placed_name] & R["decided"][placed_name], R["flags"][placed_name] | ~R["decided"][placed_name])
        placed._exact = R["flags"][placed_name]
        success = _and(placed, static)
        assert not R["flags"]["success"].any()
        R["reward"] = np.where(_val(success), top, R["reward"])
        R["flags"]["success"], R["decided"]["success"] = _val(success), success.decided
        if task == "pick":
            R["flags"]["is_robot_static"], R["decided"]["is_robot_static"] = _val(static), static.decided
        else:
            R["flags"]["static"], R["decided"]["static"] = _val(static), static.decided
        R["reward_decided"] = R["reward_decided"] & success.decided
    elif task == "place":
        assert np.array_equal(R["flags"]["success"], R1["flags"]["success"])  # (the robot's is_static is no part of success)
        R["reward"] = np.where(_val(static), R1["reward"], R["reward"])
        on, ok = R["flags"]["is_obj_on_bin"], R["flags"]["success"]
        R["flags"]["robot_static"], R["decided"]["robot_static"] = _val(static), static.decided
        # (read by the reward on the bin only, and not where success writes over it)
        read = static.decided | (~on & R["decided"]["is_obj_on_bin"]) | (ok & R["decided"]["success"])
        R["flags"]["robot_static_if_read"], R["decided"]["robot_static_if_read"] = _val(static), read
        R["reward_decided"] = R["decided"]["success"] & R["decided"]["is_obj_grasped"] & R["decided"]["is_obj_on_bin"] & read
    return R
