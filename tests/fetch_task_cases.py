"""The table-top tasks with the Fetch: env ids and shapes, the glue between an env (oracle-backed on the CPU, HIP on the
GPU), tests/fetch_task_reference.py and the native task records, the scripted squeeze and the table of joint velocities
that puts each threshold of Fetch.is_static on both sides. Test infrastructure only; snapshot / buffer helpers and the
comparison are those of tests/task_cases.py."""
import math

import numpy as np
import torch

import maniskill_amd.envs  # noqa: F401
from tests import task_cases as tc
from tests.task_cases import f32

ALL_ENV_IDS = dict(pick="PickCube-v1", push="PushCube-v1", stack="StackCube-v1", pull="PullCube-v1", poke="PokeCube-v1", lift="LiftPegUpright-v1",
                   place="PlaceSphere-v1", tool="PullCubeTool-v1")
GATED = ("pick", "stack", "poke", "lift", "place", "tool")  # tasks whose epilogue reads a robot-dependent rule
OBS_EXTRA = dict(pick=24, push=17, stack=30, pull=17, poke=36, lift=14, place=21, tool=21)
N_FREE = dict(pick=1, push=1, stack=2, pull=1, poke=2, lift=1, place=1, tool=2)
TOP_REWARD = dict(pick=5.0, stack=8.0, poke=10.0, lift=3.0, place=13.0, tool=5.0)
FLAG_NAMES = dict(pick=("success", "is_obj_placed", "is_robot_static", "is_grasped"), stack=("success", "is_cubeA_on_cubeB", "is_cubeA_static", "is_cubeA_grasped"),
                  poke=("success", "is_cube_placed", "is_peg_cube_fit", "is_peg_grasped"), lift=("success",),
                  place=("success", "is_obj_grasped", "is_obj_on_bin", "is_obj_static"), tool=("success",))
GRASPED = dict(pick="is_grasped", stack="is_cubeA_grasped", poke="is_peg_grasped", place="is_obj_grasped")  # the grasp flag where the kernel reports it
N_METRICS = dict(poke=2, tool=3)
FETCH_DOF = 15
FETCH_QPOS = [0, 0, 0, 0.386, 0, 0, 0, -math.pi / 4, 0, math.pi / 4, 0, math.pi / 3, 0, 0.015, 0.015]
FETCH_ROOT = [-1.05, 0.0, -0.9196429]


def make_env(task, N, backend, seed=7, **kw):
    import gymnasium as gym

    env = gym.make(ALL_ENV_IDS[task], robot_uids="fetch", num_envs=N, sim_backend=backend, **kw)
    env.reset(seed=seed)
    return env


def plain_instance(model):
    """(NDOF, NR) of the plain control step mssim_dispatch::plain_step answers for the model, as rows_per_env
    (mssim_model_pack.h) computes it (tests/articulated_lcp_cases.py states the same)"""
    comps = model.n_dof + 6 * model.n_free
    nr = 1 if comps <= 16 else (2 if model.n_free <= 2 else 4)
    ndof = 0 if nr == 4 else (model.n_dof if model.n_dof in (9, 15) or (model.n_dof == 7 and nr == 1) else 0)
    return ndof, nr


def grasped_object(task, base):
    return dict(pick=lambda: base.cube, stack=lambda: base.cubeA, poke=lambda: base.peg, lift=lambda: base.peg, place=lambda: base.obj,
                tool=lambda: base.l_shape_tool)[task]()


def params(task, base, normalized=None):
    """the task's parameters for tests/fetch_task_reference.py `evaluate`: as the env's own fused path states them, every
    float rounded to float32 (the value the native record carries), the Fetch's fingers by name; `normalized`: the reward
    divided by its top value (None: as the env's reward mode has it)"""
    if normalized is None:
        normalized = base._reward_mode == "normalized_dense"
    a = base.agent
    r = lambda o: int(o._body_row)
    F = lambda x: float(f32(x))
    links = a.robot.links_map
    P = dict(tcp_row=r(a.tcp), left_row=r(links["l_gripper_finger_link"]), right_row=r(links["r_gripper_finger_link"]), min_force=F(0.5),
             max_angle_deg=F(20 if task == "tool" else 85), reward_scale=F(1 / TOP_REWARD[task]) if normalized else F(1))
    if task == "pick":
        P.update(obj_row=r(base.cube), goal_row=r(base.goal_site), goal_thresh=F(base.goal_thresh), static_thresh=F(0.2))
    elif task == "stack":
        hs = base.cube_half_size.float()
        P.update(cubeA_row=r(base.cubeA), cubeB_row=r(base.cubeB), cube_half_size=F(float(hs[2])), on_xy_thresh=F(float(torch.linalg.norm(hs[:2]) + 0.005)),
                 on_z_thresh=F(0.005), gripper_width=F(float(base._gripper_width())), static_lin_thresh=F(1e-2), static_ang_thresh=F(0.5))
    elif task == "poke":
        P.update(peg_row=r(base.peg), cube_row=r(base.cube), goal_row=r(base.goal_region), peg_half_length=F(base.peg_half_length),
                 cube_half_size=F(base.cube_half_size), goal_radius=F(base.goal_radius), align_thresh=F(0.05), reach_thresh=F(0.01), static_thresh=F(0.2))
    elif task == "lift":
        P.update(peg_row=r(base.peg), peg_half_length=F(base.peg_half_length), upright_thresh=F(0.08), height_thresh=F(0.005))
    elif task == "place":
        P.update(obj_row=r(base.obj), bin_row=r(base.bin), radius=F(base.radius), bin_base_half=F(base.block_half_size[0]), on_bin_tol=F(0.005),
                 static_lin_thresh=F(1e-2), static_ang_thresh=F(0.5), robot_static_thresh=F(0.2), gripper_width=F(float(base._gripper_width())))
    else:
        P.update(cube_row=r(base.cube), tool_row=r(base.l_shape_tool), base_row=r(a.robot.get_links()[0]), cube_half_size=F(base.cube_half_size),
                 hook_length=F(base.hook_length), arm_reach=F(base.arm_reach), cube_size=F(base.cube_size), pulled_close_dist=F(0.6))
    return P


def native_task(task, P, n_dof=FETCH_DOF):
    """the native record of the reference's parameters: the right finger as finger 1, the left as finger 2"""
    from maniskill_amd import native

    cls = dict(pick=native.PickTask, stack=native.StackTask, poke=native.PokeTask, lift=native.LiftPegTask, place=native.PlaceTask, tool=native.PullToolTask)[task]
    kw = {k: v for k, v in P.items() if k not in ("left_row", "right_row")}
    kw.update(finger1_row=P["right_row"], finger2_row=P["left_row"])
    if task in ("pick", "poke", "place"):
        kw["n_static_dofs"] = n_dof - 2
    return cls(**kw)


def set_fetch_profile(px, n_dof=FETCH_DOF, threshold=0.2):
    px.set_task_robot(ranges=[(0, 3, 0.05), (3, n_dof - 5, threshold)], signed_compare=True, pick_norm_dofs=n_dof)


snapshot = tc.snapshot
write_buffers = tc.write_buffers


def torch_outputs(task, base):
    """the torch path on the env's current buffers, in the layout of the kernels' outputs"""
    info = base.evaluate()
    obs = base.get_obs(info)
    rew = base.get_reward(obs=obs, action=None, info=info)
    return dict(obs=obs.cpu().numpy(), reward=rew.cpu().numpy(), flags={k: info[k].cpu().numpy().astype(bool) for k in FLAG_NAMES[task]})


# ---------------------------------------------------------------------------------------------------------------------
def _quat_mul(a, b):
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)


def _rotate(q, v):
    qv = torch.cat([torch.zeros_like(v[..., :1]), v], -1)
    conj = q * torch.tensor([1.0, -1, -1, -1], device=q.device)
    return _quat_mul(_quat_mul(q, qv), conj)[..., 1:]


# object pose in the gripper frame (x: approach, y: closing, z: up at the rest pose): the offset of its origin from the
# point between the fingers, and its rotation there. Long bodies stand across the hand (their x axis along the gripper's z),
# the tool with the middle of its handle between the pads (held near its end it turns out of the grip).
_S = math.sqrt(0.5)
IN_HAND = dict(pick=([0, 0, 0], [1, 0, 0, 0]), stack=([0, 0, 0], [1, 0, 0, 0]), place=([0, 0, 0], [1, 0, 0, 0]),
               poke=([0, 0, 0], [_S, 0, -_S, 0]), lift=([0, 0, 0], [_S, 0, -_S, 0]), tool=([0, 0, -0.1], [_S, 0, -_S, 0]))


def squeeze(env, task, closed, open_steps=6, close_steps=8, free_steps=2):
    """The Fetch keeps its reset pose. The gripper opens, the task's object is teleported between the fingers -- at the
    pose the env's own link poses give: the midpoint of the two finger links, the gripper link's orientation -- and held
    there while the gripper closes in the envs of `closed` (bool [N]) and stays open in the others; over the last
    `free_steps` control steps nothing is pinned, so the impulses of the last substep are the solver's own. The other
    bodies of the task keep their reset poses on the table. In an open env the object is put back once more at the end:
    hand around it, no contact."""
    from maniskill_amd.utils.structs.pose import Pose

    base = env.unwrapped
    dev, N = base.device, base.num_envs
    agent = base.agent
    obj = grasped_object(task, base)
    closed = torch.as_tensor(np.asarray(closed, bool), device=dev)
    act = torch.zeros(N, base.single_action_space.shape[0], device=dev)
    g = agent.controller.action_mapping["gripper"][0]
    act[:, g] = 1.0
    for _ in range(open_steps):
        env.step(act)
    off, rot = (torch.tensor(x, dtype=torch.float32, device=dev) for x in IN_HAND[task])
    zero = torch.zeros(N, 3, device=dev)

    def pin(mask=None):
        q = agent.tcp.pose.q
        p = agent.tcp_pose.p + _rotate(q, off.expand(N, -1))
        pose = Pose.create_from_pq(p, _quat_mul(q, rot.expand(N, -1)))
        if mask is not None:
            keep = obj.pose
            sel = mask[:, None]
            pose = Pose.create_from_pq(torch.where(sel, pose.p, keep.p), torch.where(sel, pose.q, keep.q))
        obj.set_pose(pose)
        obj.set_linear_velocity(zero if mask is None else torch.where(mask[:, None], zero, obj.linear_velocity))
        obj.set_angular_velocity(zero if mask is None else torch.where(mask[:, None], zero, obj.angular_velocity))
        base.scene._gpu_apply_all()
        base.scene._gpu_fetch_all()

    pin()
    base.scene.px.wake_all()
    act[:, g] = torch.where(closed, -1.0, 1.0)
    for i in range(close_steps + free_steps):
        env.step(act)
        if i < close_steps:
            pin()
        elif i + 1 < close_steps + free_steps:
            pin(~closed)
    return act


def arrange(task, base, where):
    """after the squeeze, without stepping: in the envs of `where` (bool [N]) the body that decides whether the robot's
    is_static is read comes to the object -- PickCube's goal onto the cube in the hand, PokeCube's goal region under its
    cube, PlaceSphere's bin under the sphere in the hand (kinematic bodies: a pose written and applied). The other three
    tasks read no is_static."""
    from maniskill_amd.utils.structs.pose import Pose

    where = torch.as_tensor(np.asarray(where, bool), device=base.device)[:, None]
    if task == "pick":
        body, p = base.goal_site, base.cube.pose.p
    elif task == "poke":
        body = base.goal_region
        p = torch.cat([base.cube.pose.p[:, :2], body.pose.p[:, 2:]], 1)
    elif task == "place":
        body = base.bin
        p = base.obj.pose.p - torch.tensor([0.0, 0.0, base.radius + base.block_half_size[0]], device=base.device)
    else:
        return
    body.set_pose(Pose.create_from_pq(torch.where(where, p, body.pose.p), body.pose.q))
    base.scene._gpu_apply_all()
    base.scene._gpu_fetch_all()


# ---------------------------------------------------------------------------------------------------------------------
# joint velocities of a Fetch (15 joints: base 0..2, body and arm 3..12, gripper 13, 14) that put each threshold of
# Fetch.is_static on both sides: (label, {joint: velocity}, static). Every other joint moves at 0.01.
QVEL_CASES = [
    ("at rest", {}, True),
    ("base x at 0.04", {0: 0.04}, True),
    ("base x at 0.06", {0: 0.06}, False),
    ("base yaw at 0.04", {2: 0.04}, True),
    ("base yaw at 0.06", {2: 0.06}, False),
    ("base y at -1 (signed: static)", {1: -1.0}, True),
    ("torso at 0.19", {3: 0.19}, True),
    ("torso at 0.21", {3: 0.21}, False),
    ("wrist roll at 0.19", {12: 0.19}, True),
    ("wrist roll at 0.21", {12: 0.21}, False),
    ("elbow at -1 (signed: static)", {9: -1.0}, True),
    ("a body joint between the two thresholds", {5: 0.1}, True),
    ("gripper joints fast (not read)", {13: 5.0, 14: -5.0}, True),
    ("gripper fast and base at 0.06", {13: 5.0, 0: 0.06}, False),
    ("every arm joint at -0.5 and the base at -0.3 (signed: static)", {j: (-0.3 if j < 3 else -0.5) for j in range(13)}, True),
]


def qvel_batch(N, n_dof=FETCH_DOF, start=0):
    """-> (qvel [N, n_dof] f32, labels, static [N] bool): env e holds case (start + e) modulo the table's length"""
    q = np.full((N, n_dof), 0.01, np.float32)
    labels, static = [], np.zeros(N, bool)
    for e in range(N):
        label, joints, st = QVEL_CASES[(start + e) % len(QVEL_CASES)]
        for j, v in joints.items():
            q[e, j] = v
        labels.append(label)
        static[e] = st
    return q, labels, static


def compare(task, got, R, labels, tol_reward, what):
    """flags equal where the reference decides them, observations bit-exact, rewards within tol_reward (tests/task_cases.py
    `compare`); returns the measured reward difference"""
    return tc.compare(task if task == "pick" else "fetch_" + task, got, R, labels, tol_reward, what=what)["reward"]
