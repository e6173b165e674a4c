"""Constructed states for the PlaceSphere and PullCubeTool epilogues, one case per env index (the table repeats over the
batch), and the glue between an env (oracle-backed on the CPU, HIP on the GPU), tests/place_tool_reference.py and the native
task structs. Test infrastructure only; snapshot / buffer helpers and the comparison are those of tests/task_cases.py.

A batch is made as tests/poke_lift_cases.py makes its own: (1) a scripted grasp (the sphere between the fingers; the tool's
handle between the fingers) in the envs whose case wants one: the finger <-> object impulses of the last substep cannot be
written from outside, so they are produced physically. The envs of a `released` case keep the gripper open through the same
motion, so they end with the hand around the object and no contact: a release that holds in both launch forms. (2) The
poses / velocities of the user-visible buffers are overwritten case by case. The tcp stays where the motion left it and the
objects are placed relative to it, so the same cases serve the copy-out form, which recomputes the link rows from qpos;
there a finger cannot be turned and the base link cannot be moved: `link_rows=False` leaves those cases without that part.

Every case is built so that the float64 reference decides each predicate by at least MIN_MARGIN = 1e-4 (metres, rad/s,
newtons or degrees). That is three orders of magnitude above float32's error on the quantities compared: positions below
2 m carry at most 2^-23 = 1.2e-7, a norm of three of them a few times that; the finger angle in degrees, an acosf of a
cosine below 0.95, about 1e-5. Thresholds are approached to EDGE = 1e-3 (distances of 5 cm and more; relative 5e-3 for
the velocities of 0.2 and 0.5 rad/s) or EDGE_MM = 5e-4 (the 5 mm and 1 cm/s thresholds of PlaceSphere). `check` asserts
the margins, compares an implementation with the reference and returns how many envs it had to leave out, which the tests
assert to be 0."""
import numpy as np
import torch

import maniskill_amd.envs  # noqa: F401
from tests import task_cases as tc
from tests.task_cases import DIAG, _finger_at_angle, _set, _turn_finger, _unit, f32

ENV_IDS = dict(place="PlaceSphere-v1", tool="PullCubeTool-v1")
TOP_REWARD = dict(place=13.0, tool=5.0)
OBS_EXTRA = dict(place=21, tool=21)
N_FLAGS = dict(place=4, tool=1)
FLAG_NAMES = dict(place=("success", "is_obj_grasped", "is_obj_on_bin", "is_obj_static"), tool=("success",))
EDGE = 1e-3
EDGE_MM = 5e-4
MIN_MARGIN = 1e-4

# max |torch f32 path (CPU) - f64 reference| over the case tables, recorded from the output of
# tests/test_place_tool.py::test_torch_path_matches_reference (which asserts that they still bound what it measures),
# rounded up:
#   dense reward       place 8.13e-7 (rewards up to 13), tool 6.77e-7 (up to 12.2)
#   normalised reward  place 6.80e-8, tool 1.47e-7 (up to 2.4: the success bonus is added to the staged reward)
#   PullCubeTool's info floats (`reward` per env; the two batch means) 1.83e-7
# The torch path of PullCubeTool does not give the per-env columns behind its two batch means; the kernel's three metric
# columns (all below 2.5 in magnitude, as the per-env `reward`) are held to 4 x the last figure.
MEASURED = dict(place=8.2e-7, tool=6.8e-7, tool_metrics=1.9e-7)
MEASURED_NORMALIZED = dict(place=6.9e-8, tool=1.5e-7)


def make_env(task, N, backend, seed=7, **kw):
    import gymnasium as gym

    env = gym.make(ENV_IDS[task], num_envs=N, sim_backend=backend, **kw)
    env.reset(seed=seed)
    return env


snapshot = tc.snapshot
write_buffers = tc.write_buffers

# where the scripted motion leaves the object: under the hand, on the table. The tool's origin lies 5 cm behind the
# hand, so the fingers close on its handle (5 cm wide, as the peg of tests/poke_lift_cases.py)
GRASP_Z = dict(place=0.02, tool=0.025)


def scripted_grasp(env, task, released, close_steps=10):
    """the object under the hand in every env, the other body out of the way; the hand descends with the gripper open and
    closes it, except in the envs of `released` (bool [N]), which keep it open"""
    from maniskill_amd.utils.structs.pose import Pose

    base = env.unwrapped
    dev, N = base.device, base.num_envs
    z = GRASP_Z[task]
    grasp_p = torch.tensor([0.0, 0.0, z], device=dev)
    key = ("place_tool", task, round(z, 4))  # (the cache is shared with tests/task_cases.py: the name keeps the entries apart)
    if key not in tc._IK_CACHE:
        q0 = torch.tensor([tc.REST], dtype=torch.float32, device=dev)
        q_pre = tc._ik(base, q0, grasp_p + torch.tensor([0, 0, 0.10], device=dev))
        tc._IK_CACHE[key] = (q_pre.cpu(), tc._ik(base, q_pre, grasp_p).cpu())
    q_pre, q_grasp = (q.to(dev) for q in tc._IK_CACHE[key])
    ident = torch.zeros(N, 4, device=dev)
    ident[:, 0] = 1
    zero = torch.zeros(N, 3, device=dev)
    if task == "place":
        bodies = [(base.obj, [0.0, 0.0, z]), (base.bin, [0.3, 0.2, 0.0025])]
    else:
        bodies = [(base.l_shape_tool, [-0.05, 0.0, z]), (base.cube, [0.3, -0.2, 0.02])]
    for body, p in bodies:
        body.set_pose(Pose.create_from_pq(torch.tensor(p, device=dev).repeat(N, 1), ident))
        if body.px_body_type == "dynamic":
            body.set_linear_velocity(zero)
            body.set_angular_velocity(zero)
    base.agent.robot.set_qpos(q_pre.expand(N, -1).contiguous())
    base.agent.robot.set_qvel(torch.zeros(N, 9, device=dev))
    tc._sync(base)
    base.scene.px.wake_all()
    base.agent.controller.reset()
    grip_closed = torch.where(torch.as_tensor(np.asarray(released, bool), device=dev), 1.0, -1.0)
    # (a sphere on the table has nothing that keeps it from rolling before the pads hold it: it is put back under the hand
    # after every control step of the descent and of the first `pin_steps` of the closing)
    pin_steps = 4 if task == "place" else 0
    for goal, grip, steps, pinned in ((q_grasp, torch.ones(N, device=dev), 25, 25 if pin_steps else 0), (q_grasp, grip_closed, close_steps, pin_steps)):
        for i in range(steps):
            a = torch.zeros(N, 8, device=dev)
            a[:, :7] = ((goal[:, :7] - base.agent.robot.get_qpos()[:, :7]) / 0.1).clamp(-1, 1)
            a[:, 7] = grip
            env.step(a.contiguous())
            if i < pinned:
                body, p = bodies[0]
                body.set_pose(Pose.create_from_pq(torch.tensor(p, device=dev).repeat(N, 1), ident))
                body.set_linear_velocity(zero)
                body.set_angular_velocity(zero)
                base.scene._gpu_apply_all()
                base.scene._gpu_fetch_all()


def params(task, base, normalized=False):
    """task parameters as the env's own fused path states them; every float rounded to float32, the value the native
    struct carries"""
    a = base.agent
    r = lambda o: int(o._body_row)
    F = lambda x: float(f32(x))
    P = dict(tcp_row=r(a.tcp), finger1_row=r(a.finger1_link), finger2_row=r(a.finger2_link), min_force=F(0.5),
             reward_scale=F(1 / TOP_REWARD[task]) if normalized else F(1))
    if task == "place":
        P.update(obj_row=r(base.obj), bin_row=r(base.bin), n_static_dofs=a.robot.max_dof - 2, radius=F(base.radius), bin_base_half=F(base.block_half_size[0]),
                 on_bin_tol=F(0.005), static_lin_thresh=F(1e-2), static_ang_thresh=F(0.5), robot_static_thresh=F(0.2),
                 gripper_width=F(float(base._gripper_width())), max_angle_deg=F(85))
    else:
        P.update(cube_row=r(base.cube), tool_row=r(base.l_shape_tool), base_row=r(a.robot.get_links()[0]), cube_half_size=F(base.cube_half_size),
                 hook_length=F(base.hook_length), arm_reach=F(base.arm_reach), cube_size=F(base.cube_size), pulled_close_dist=F(0.6), max_angle_deg=F(20))
    return P


def native_task(task, P):
    from maniskill_amd import native

    return (native.PlaceTask if task == "place" else native.PullToolTask)(**P)


def torch_outputs(task, base):
    """the torch path on the env's current buffers: what `check` takes. PullCubeTool's torch path gives the per-env
    `reward` of its info and the two batch means, not the per-env columns behind them."""
    info = base.evaluate()
    obs = base.get_obs(info)
    rew = base.get_reward(obs=obs, action=None, info=info)
    out = dict(obs=obs.cpu().numpy(), reward=rew.cpu().numpy(), flags={k: info[k].cpu().numpy().astype(bool) for k in FLAG_NAMES[task]})
    if task == "tool":
        out["info_reward"] = info["reward"].cpu().numpy()
        out["means"] = np.array([float(info["cube_distance"]), float(info["cube_progress"])])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# case tables: (label, fn(S, e, link_rows), released)
def _qvel(kind, ns, thr):
    def f(S, e):
        S["qvel"][e, :] = 0.01
        if kind == "moving":
            S["qvel"][e, 3] = -2.5 * thr
        elif kind == "fingers only":
            S["qvel"][e, ns:] = 5.0
        elif kind != "static":  # a signed factor of the threshold on the last joint that counts
            S["qvel"][e, ns - 1] = kind * thr
    return f


def _cases_place(P):
    t, o, b, ns = P["tcp_row"], P["obj_row"], P["bin_row"], P["n_static_dofs"]
    rad, bh, tol = float(P["radius"]), float(P["bin_base_half"]), float(P["on_bin_tol"])
    lin, ang, rs = float(P["static_lin_thresh"]), float(P["static_ang_thresh"]), float(P["robot_static_thresh"])

    def state(d_tcp=0.004, dxy=0.002, dz=0.001, v=0.0, w=0.0, vel="static", turn=None, released=False):
        """the sphere at distance d_tcp from the tcp; the bin placed so that sphere - bin = (dxy (0.8, -0.6), radius +
        bin_base_half + dz); the sphere's linear / angular speed v / w"""
        def f(S, e, link_rows):
            pt = S["rigid"][t, e, :3].astype(np.float64)
            _set(S, o, e, p=pt + d_tcp * DIAG, q=[1, 0, 0, 0], v=v * _unit([1, 2, -2]), w=w * _unit([2, -1, 2]))
            po = S["rigid"][o, e, :3].astype(np.float64)
            _set(S, b, e, p=po - np.array([0.8 * dxy, -0.6 * dxy, rad + bh + dz]), q=[1, 0, 0, 0])
            _qvel(vel, ns, rs)(S, e)
            if turn and link_rows:
                _turn_finger(P, turn)(S, e)
        return (f, released)

    far = dict(dxy=0.15, dz=-0.01)
    C = [
        ("reaching only", state(d_tcp=0.05, released=True, **far)),
        ("grasped, far from the bin", state(**far)),
        ("grasped, above the bin", state(dz=0.05)),
        ("on bin while grasped", state()),
        ("on bin while grasped, robot moving", state(vel="moving")),
        ("on bin, released, moving (linear)", state(v=3 * lin, w=0.2 * ang, released=True)),
        ("on bin, released, moving (angular)", state(v=0.2 * lin, w=3 * ang, released=True)),
        ("on bin, released, sphere and robot moving", state(v=3 * lin, vel="moving", released=True)),
        ("success", state(released=True)),
        ("success, robot moving (its is_static is no part of success)", state(vel="moving", released=True)),
        ("sphere beside the bin", state(dxy=0.03, released=True)),
        ("xy inside", state(dxy=tol - EDGE_MM, released=True)),
        ("xy outside", state(dxy=tol + EDGE_MM, released=True)),
        ("z inside, above", state(dz=tol - EDGE_MM, released=True)),
        ("z outside, above", state(dz=tol + EDGE_MM, released=True)),
        ("z inside, below", state(dz=-(tol - EDGE_MM), released=True)),
        ("z outside, below", state(dz=-(tol + EDGE_MM), released=True)),
        ("linear speed inside", state(v=lin - EDGE_MM, released=True)),
        ("linear speed outside", state(v=lin + EDGE_MM, released=True)),
        ("angular speed inside", state(w=ang * (1 - 5e-3), released=True)),
        ("angular speed outside", state(w=ang * (1 + 5e-3), released=True)),
        ("on bin while grasped, qvel inside", state(vel=1 - 5e-3)),
        ("on bin while grasped, qvel outside", state(vel=-(1 + 5e-3))),
        ("on bin while grasped, finger joint velocity is not read", state(vel="fingers only")),
        ("on bin, left finger turned away", state(turn="finger1_row")),
        ("on bin, right finger turned away", state(turn="finger2_row")),
    ]
    return [(label, f, rel) for label, (f, rel) in C]


def _cases_tool(P):
    t, cb, tl, bs = P["tcp_row"], P["cube_row"], P["tool_row"], P["base_row"]
    reach, hook, half = float(P["arm_reach"]), float(P["hook_length"]), float(P["cube_half_size"])
    close = float(P["pulled_close_dist"])
    off = np.array([-(hook + half), -0.067, 0.0])

    def state(d_tcp=0.004, d_hook=None, cube_dist=None, cube_x=None, base_dist=None, turn=None, angle=None, released=False):
        """the tool's grasp point (tool + (0.02, 0, 0)) at distance d_tcp from the tcp. The cube either follows the tool (d_hook:
        the tool at that distance from the ideal hook position cube + off), or lies at cube_dist from the base link in xy, or
        at world x = cube_x. base_dist (with the link rows writable): the base link's row moved to that xy distance from the
        cube. turn: a finger's row turned by 90 degrees; angle = (finger, s): that finger's closing axis at max_angle x s from
        the force on it."""
        def f(S, e, link_rows):
            pt = S["rigid"][t, e, :3].astype(np.float64)
            _set(S, tl, e, p=pt - [0.02, 0, 0] + d_tcp * DIAG, q=[1, 0, 0, 0], v=[0, 0, 0], w=[0, 0, 0])
            ptool = S["rigid"][tl, e, :3].astype(np.float64)
            pb = S["rigid"][bs, e, :3].astype(np.float64)
            if d_hook is not None:
                pc = ptool - off - d_hook * DIAG
            elif cube_x is not None:
                pc = np.array([cube_x, pb[1] + 0.3, half])
            else:
                pc = np.array([pb[0] + 0.8 * cube_dist, pb[1] - 0.6 * cube_dist, half])
            _set(S, cb, e, p=pc, q=[1, 0, 0, 0], v=[0, 0, 0], w=[0, 0, 0])
            pc = S["rigid"][cb, e, :3].astype(np.float64)
            if base_dist is not None and link_rows:
                _set(S, bs, e, p=[pc[0] - 0.8 * base_dist, pc[1] + 0.6 * base_dist, 0.0])
            if turn and link_rows:
                _turn_finger(P, turn)(S, e)
            if angle and link_rows:
                _finger_at_angle(P, "tool_row", *angle)(S, e)
        return (f, released)

    C = [
        ("not grasping", state(d_tcp=0.05, cube_dist=0.75, released=True)),
        ("grasping, not positioned", state(d_hook=0.2)),
        ("grasping, cube far away", state(cube_dist=0.9)),
        ("positioned, pulling", state(d_hook=0.02)),
        ("positioned, pulling, base moved near: success", state(d_hook=0.02, base_dist=0.3)),
        ("positioning distance inside", state(d_hook=0.05 - EDGE)),
        ("positioning distance outside", state(d_hook=0.05 + EDGE)),
        ("pushed away", state(cube_x=0.6)),
        ("pushed away, not grasping", state(cube_x=0.6, released=True)),
        ("pushed away: x inside", state(cube_x=reach + 0.15 - EDGE)),
        ("pushed away: x outside", state(cube_x=reach + 0.15 + EDGE)),
        ("success, grasping", state(cube_dist=0.4)),
        ("success, not grasping", state(d_tcp=0.05, cube_dist=0.4, released=True)),
        ("success, cube near the workspace centre", state(cube_dist=0.035, released=True)),
        ("pulled close: inside", state(cube_dist=close - EDGE)),
        ("pulled close: outside", state(cube_dist=close + EDGE)),
        ("positioned, left finger turned away", state(d_hook=0.02, turn="finger1_row")),
        ("positioned, right finger turned away", state(d_hook=0.02, turn="finger2_row")),
        ("positioned, a grasp at 50 degrees: passes at 85, fails at 20", state(d_hook=0.02, angle=("finger1_row", 2.5))),
        ("positioned, left finger angle inside", state(d_hook=0.02, angle=("finger1_row", 1 - 5e-3))),
        ("positioned, left finger angle outside", state(d_hook=0.02, angle=("finger1_row", 1 + 5e-3))),
        ("positioned, right finger angle inside", state(d_hook=0.02, angle=("finger2_row", 1 - 5e-3))),
        ("positioned, right finger angle outside", state(d_hook=0.02, angle=("finger2_row", 1 + 5e-3))),
    ]
    return [(label, f, rel) for label, (f, rel) in C]


TABLES = dict(place=_cases_place, tool=_cases_tool)
# the case a batch of one env holds: on the bin and grasped; positioned and grasping
START_SINGLE = dict(place=3, tool=3)


def released_mask(task, P, N, start=0):
    """bool [N]: env e holds a `released` case"""
    C = TABLES[task](P)
    return np.array([C[(start + e) % len(C)][2] for e in range(N)], bool)


def build_batch(task, S0, P, start=0, link_rows=True):
    """-> (S, labels): env e holds case (start + e) modulo the table's length, built on the state env e has in S0 (whose
    scripted motion must have been made with released_mask(task, P, N, start))"""
    S = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in S0.items()}
    C = TABLES[task](P)
    N = S["qpos"].shape[0]
    labels = []
    for e in range(N):
        label, fn, _ = C[(start + e) % len(C)]
        fn(S, e, link_rows)
        labels.append(label)
    return S, labels


# ---------------------------------------------------------------------------------------------------------------------
def tolerance(task, P):
    """(reward, metrics): 4 x the measured difference of the torch path and the reference, for the dense or the normalised
    reward"""
    f = P["reward_scale"]
    assert f == 1.0 or abs(f * TOP_REWARD[task] - 1) < 1e-6
    return 4 * (MEASURED if f == 1.0 else MEASURED_NORMALIZED)[task], 4 * MEASURED["tool_metrics"]


def check(task, got, R, labels, tol_reward, tol_metrics, what):
    """`got` (obs, reward, flags; PullCubeTool: `metrics` [N, 3] of the kernel, or `info_reward` [N] and `means` [2] of the
    torch path) against the reference's result: flags equal, observation entries bit-exact, rewards within tol_reward,
    metrics within tol_metrics. Every predicate of every env must be decided by MIN_MARGIN. Returns (measured reward
    difference, measured metric difference, number of envs left out)."""
    for name, (m, band) in R["margins"].items():
        small = np.nonzero(np.abs(m) < MIN_MARGIN)[0]
        assert len(small) == 0, (what, task, name, "decided by less than MIN_MARGIN", [(int(e), labels[e], float(m[e])) for e in small[:4]])
    excluded = int((~R["reward_decided"]).sum() + sum(int((~d).sum()) for d in R["decided"].values()))
    out = tc.compare(task, got, R, labels, tol_reward, what=what)
    d_m = 0.0
    if task == "tool":
        if "metrics" in got:
            d = np.abs(got["metrics"].astype(np.float64) - R["metrics"])
            d_m = float(d.max())
            assert d_m <= tol_metrics, (what, task, "metrics", d_m, labels[int(d.max(1).argmax())], int(d.max(0).argmax()))
        else:
            d = np.abs(got["info_reward"].astype(np.float64) - R["metrics"][:, 2])
            d_mean = np.abs(got["means"] - R["metrics"][:, :2].mean(0))
            d_m = float(max(d.max(), d_mean.max()))
            assert d_m <= tol_metrics, (what, task, "info reward / batch means", float(d.max()), d_mean)
    return out["reward"], d_m, excluded
