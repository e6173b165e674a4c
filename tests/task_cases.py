"""Constructed states for the five task epilogues, one case per env index, and the glue between an env (oracle-backed on
the CPU, HIP on the GPU), tests/task_reference.py and the native task structs. Test infrastructure only.

A batch is made in two steps: (1) optionally a scripted grasp in ALL envs of the batch (the finger <-> object impulses of
the last substep cannot be written from outside, so they are produced physically); (2) the poses / velocities of the
user-visible buffers are overwritten case by case. The impulses stay, so `grasped` is computed by both sides from the
same raw impulses and the case's finger poses. Cases left over after the constructed ones are seeded random states."""
import math

import numpy as np
import torch

import maniskill_amd.envs  # noqa: F401
from tests import task_reference as ref

ENV_IDS = dict(pick="PickCube-v1", push="PushCube-v1", peg="PegInsertionSide-v1", stack="StackCube-v1", pusht="PushT-v1")
TOP_REWARD = dict(pick=5.0, push=3.0, peg=10.0, stack=8.0, pusht=3.0)
OBJ = dict(pick="cube", peg="peg", stack="cubeA")
f32 = np.float32


def make_env(task, N, backend, **kw):
    import gymnasium as gym

    env = gym.make(ENV_IDS[task], num_envs=N, sim_backend=backend, **kw)
    env.reset(seed=7)
    return env


def up(x):
    return float(np.nextafter(f32(x), f32(np.inf)))


def down(x):
    return float(np.nextafter(f32(x), f32(-np.inf)))


# ---------------------------------------------------------------------------------------------------------------------
# env <-> snapshot
def snapshot(base):
    """what an epilogue reads, as numpy float32 (tests/task_reference.py `S`)"""
    px = base.scene.px
    m = px.model
    N = base.num_envs
    npair = int(m.n_pair)
    imp = px.read_internal("pair_impulse", max(3 * npair, 1)).cpu().numpy()[: 3 * npair].reshape(npair, 3, N).transpose(0, 2, 1)
    cnt = px.read_internal("contact_count", max(npair, 1)).cpu().numpy()[:npair]
    return dict(
        rigid=px.cuda_rigid_body_data.torch().cpu().numpy().reshape(-1, N, 13).copy(), qpos=px.cuda_articulation_qpos.torch().cpu().numpy().copy(),
        qvel=px.cuda_articulation_qvel.torch().cpu().numpy().copy(), imp=imp.copy(), cnt=cnt.copy(),
        pair_shape=np.asarray(m.arrays["pair_shape"]).reshape(-1, 2), shape_row=np.asarray(m.arrays["shape_row"]), dt=float(f32(px.timestep)),
    )


def write_buffers(base, S):
    """the case batch into the user-visible buffers (nothing is applied to the simulation state)"""
    px = base.scene.px
    dev = base.device
    px.cuda_rigid_body_data.torch()[:] = torch.from_numpy(S["rigid"].reshape(-1, 13)).to(dev)
    px.cuda_articulation_qpos.torch()[:] = torch.from_numpy(S["qpos"]).to(dev)
    px.cuda_articulation_qvel.torch()[:] = torch.from_numpy(S["qvel"]).to(dev)


def params(task, base, variant=0, forces=None):
    """task parameters as the env's own fused path states them (variant 0), or a second set with every parameter off
    its default (variant 1; `forces`: measured (left, right) finger forces of a grasped env, min_force goes between).
    Every float is rounded to float32: the value the native struct carries."""
    a = base.agent
    r = lambda o: int(o._body_row)
    F = lambda x: float(f32(x))
    if task in ("pick", "peg", "stack"):
        fr = dict(finger1_row=r(a.finger1_link), finger2_row=r(a.finger2_link))
        mf = F(0.5) if not variant or forces is None else F(0.5 * (forces[0] + forces[1]))
    if task == "pick":
        P = dict(tcp_row=r(a.tcp), obj_row=r(base.cube), goal_row=r(base.goal_site), n_static_dofs=a.robot.max_dof - 2, **fr)
        P.update(dict(goal_thresh=F(0.025), static_thresh=F(0.2), min_force=mf, max_angle_deg=F(85), reward_scale=F(1)) if not variant else
                 dict(goal_thresh=F(0.04), static_thresh=F(0.3), min_force=mf, max_angle_deg=F(60), reward_scale=F(0.2)))
    elif task == "push":
        P = dict(tcp_row=r(a.tcp), obj_row=r(base.obj), goal_row=r(base.goal_region))
        P.update(dict(goal_radius=F(base.goal_radius), cube_half_size=F(base.cube_half_size), reward_scale=F(1)) if not variant else
                 dict(goal_radius=F(0.15), cube_half_size=F(0.03), reward_scale=F(1 / 3)))
    elif task == "peg":
        P = dict(tcp_row=r(a.tcp), peg_row=r(base.peg), box_row=r(base.box), **fr,
                 peg_half_sizes=base.peg_half_sizes.float().cpu().numpy(), box_hole_offsets=base.box_hole_offsets.p.float().cpu().numpy(),
                 box_hole_radii=base.box_hole_radii.float().cpu().numpy())
        P.update(dict(min_force=mf, max_angle_deg=F(20), reward_scale=F(1)) if not variant else dict(min_force=mf, max_angle_deg=F(45), reward_scale=F(0.1)))
    elif task == "stack":
        hs = base.cube_half_size.float().cpu()
        P = dict(tcp_row=r(a.tcp), cubeA_row=r(base.cubeA), cubeB_row=r(base.cubeB), **fr, cube_half_size=F(hs[2]), gripper_width=F(float(base._gripper_width())))
        P.update(dict(on_xy_thresh=F(torch.linalg.norm(hs[:2]) + 0.005), on_z_thresh=F(0.005), static_lin_thresh=F(1e-2), static_ang_thresh=F(0.5),
                      min_force=mf, max_angle_deg=F(85), reward_scale=F(1)) if not variant else
                 dict(on_xy_thresh=F(0.02), on_z_thresh=F(0.01), static_lin_thresh=F(0.05), static_ang_thresh=F(0.25), min_force=mf, max_angle_deg=F(60),
                      reward_scale=F(0.125)))
    elif task == "pusht":
        uv = base.uv_grid.detach().cpu().float().numpy()
        consts = dict(w2g=base.world_to_goal_trans.detach().cpu().float().numpy().reshape(9), u=uv[0, 0, :].copy(), v=uv[1, :, 0].copy(),
                      template=base.tee_render.detach().cpu().bool().numpy())
        P = dict(tcp_row=r(a.tcp), tee_row=r(base.tee), goal_row=r(base.goal_tee), consts=consts)
        tmpl = consts["template"]
        edge = float(f32(int((tmpl[1:] & tmpl[:-1]).sum())) / f32(tmpl.sum()))  # the on-goal fraction, see _cases_pusht
        P.update(dict(goal_z_rot=F(base.goal_z_rot), intersection_thresh=F(0.9), reward_div=F(1)) if not variant else
                 dict(goal_z_rot=F(1.0), intersection_thresh=edge if variant == 1 else up(edge), reward_div=F(3)))
    return P


def native_task(task, base, P, keep):
    """the ctypes struct of `P`; device arrays it points to are appended to `keep`"""
    from maniskill_amd import native

    dev = base.device
    scalars = {k: v for k, v in P.items() if isinstance(v, (int, float))}
    if task == "pick":
        return native.PickTask(**scalars)
    if task == "push":
        return native.PushTask(**scalars)
    if task == "stack":
        return native.StackTask(**scalars)
    if task == "peg":
        g = [torch.from_numpy(np.ascontiguousarray(P[k], f32)).to(dev) for k in ("peg_half_sizes", "box_hole_offsets", "box_hole_radii")]
        keep.extend(g)
        return native.PegTask(**scalars, peg_half_sizes=g[0].data_ptr(), box_hole_offsets=g[1].data_ptr(), box_hole_radii=g[2].data_ptr())
    consts = base.pusht_consts()
    keep.append(consts)
    return native.PushTTask(**scalars, consts=consts.data_ptr())


OBS_EXTRA = dict(pick=24, push=17, peg=25, stack=30, pusht=17)
N_FLAGS = dict(pick=4, push=1, peg=1, stack=4, pusht=1)
FLAG_NAMES = dict(pick=("success", "is_obj_placed", "is_robot_static", "is_grasped"), push=("success",), peg=("success",),
                  stack=("success", "is_cubeA_on_cubeB", "is_cubeA_static", "is_cubeA_grasped"), pusht=("success",))


def torch_outputs(task, base):
    """the torch path on the env's current buffers: obs [N, D], reward [N], flags {name: bool [N]}, extras"""
    info = base.evaluate()
    obs = base.get_obs(info)
    rew = base.get_reward(obs=obs, action=None, info=info)
    out = dict(obs=obs.cpu().numpy(), reward=rew.cpu().numpy(), flags={k: info[k].cpu().numpy().astype(bool) for k in FLAG_NAMES[task]})
    if task == "peg":
        out["head_at_hole"] = info["peg_head_pos_at_hole"].cpu().numpy()
    if task == "pusht":
        out["count"] = base.pseudo_render_intersection_count().cpu().numpy()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# scripted grasp (Panda, default pd_joint_delta_pos control): the same joint waypoints in every env
_IK_CACHE = {}
REST = [0, math.pi / 8, 0, -math.pi * 5 / 8, 0, math.pi * 3 / 4, math.pi / 4, 0.04, 0.04]


def _sync(base):
    base.scene._gpu_apply_all()
    base.scene.px.gpu_update_articulation_kinematics()
    base.scene._gpu_fetch_all()


def _ik(base, q0, target):
    """joints 1, 3, 5 such that the tcp of env 0 reaches `target` (Gauss-Newton on finite differences of the FK)"""
    dev, robot, N = base.device, base.agent.robot, base.num_envs

    def tcp_at(q):
        robot.set_qpos(q.expand(N, -1).contiguous())
        _sync(base)
        return base.agent.tcp.pose.p[0].clone()

    q, idx = q0.clone(), [1, 3, 5]
    for _ in range(25):
        p = tcp_at(q)
        J = torch.zeros(3, 3, device=dev)
        for k, j in enumerate(idx):
            dq = q.clone()
            dq[0, j] += 1e-3
            J[:, k] = (tcp_at(dq) - p) / 1e-3
        step = torch.linalg.solve(J.T @ J + 1e-6 * torch.eye(3, device=dev), J.T @ (target - p))
        for k, j in enumerate(idx):
            q[0, j] += step[k]
    assert torch.norm(tcp_at(q) - target) < 2e-3
    return q


def scripted_grasp(env, task, close_steps=10):
    """places the task's object under the hand in every env, descends with the gripper open and closes it; the envs end
    with both fingers pressing the object (the last substep's impulses are what the epilogues read). Returns the hold
    action."""
    from maniskill_amd.utils.structs.pose import Pose

    base = env.unwrapped
    dev, N = base.device, base.num_envs
    obj = getattr(base, OBJ[task])
    z = 0.02
    if task == "peg":
        z = float(base.peg_half_sizes[:, 2].min())
    if task == "stack":  # cube A stands on cube B: the grasp is the on-and-grasped state, a release leaves A stacked
        z = 0.06
    grasp_p = torch.tensor([0.0, 0.0, z], device=dev)
    key = (round(z, 4),)
    if key not in _IK_CACHE:
        q0 = torch.tensor([REST], dtype=torch.float32, device=dev)
        q_pre = _ik(base, q0, grasp_p + torch.tensor([0, 0, 0.10], device=dev))
        _IK_CACHE[key] = (q_pre.cpu(), _ik(base, q_pre, grasp_p).cpu())
    q_pre, q_grasp = (q.to(dev) for q in _IK_CACHE[key])
    p = torch.zeros(N, 3, device=dev)
    q = torch.zeros(N, 4, device=dev)
    q[:, 0] = 1
    if task == "peg":  # the peg along x, grasped 6 cm behind its centre
        p[:, 0] = 0.06
        p[:, 2] = base.peg_half_sizes[:, 2]
    else:
        p[:, 2] = z
    obj.set_pose(Pose.create_from_pq(p, q))
    if task == "peg":  # the box out of the way (a tail case may have left it around the peg)
        pb = torch.zeros(N, 3, device=dev)
        pb[:, 1], pb[:, 2] = 0.4, base.peg_half_sizes[:, 0]
        base.box.set_pose(Pose.create_from_pq(pb, q))
    obj.set_linear_velocity(torch.zeros(N, 3, device=dev))
    obj.set_angular_velocity(torch.zeros(N, 3, device=dev))
    if task == "stack":
        pb = p.clone()
        pb[:, 2] = 0.02
        base.cubeB.set_pose(Pose.create_from_pq(pb, q))
        base.cubeB.set_linear_velocity(torch.zeros(N, 3, device=dev))
        base.cubeB.set_angular_velocity(torch.zeros(N, 3, device=dev))
    base.agent.robot.set_qpos(q_pre.expand(N, -1).contiguous())
    base.agent.robot.set_qvel(torch.zeros(N, 9, device=dev))
    _sync(base)
    base.scene.px.wake_all()
    base.agent.controller.reset()
    for goal, grip, steps in ((q_grasp, 1.0, 25), (q_grasp, -1.0, close_steps)):
        for _ in range(steps):
            a = torch.zeros(N, 8, device=dev)
            a[:, :7] = ((goal[:, :7] - base.agent.robot.get_qpos()[:, :7]) / 0.1).clamp(-1, 1)
            a[:, 7] = grip
            env.step(a.contiguous())
    hold = torch.zeros(N, 8, device=dev)
    hold[:, 7] = -1.0
    return hold


def apply_tail_cases(env, task, hold):
    """constructed states for the tail form, set through the actors' setters + apply + FK from the state the scripted grasp
    (pick, stack, peg) or the reset (push, pusht) left, one case per env index modulo the table's length; returns the
    per-env action of the one control step that follows. Everything here is physically steppable: kinematic goals / boxes
    are moved to where the held object is, the gripper is opened in some envs (a release), the arm is moved in some (not
    static)."""
    from maniskill_amd.utils.structs.pose import Pose

    base = env.unwrapped
    dev, N = base.device, base.num_envs
    e = torch.arange(N, device=dev)
    act = hold.clone()
    ident = torch.zeros(N, 4, device=dev)
    ident[:, 0] = 1
    if task == "pick":  # goal on / off the held cube x hold / move the arm x hold / release
        g = base.cube.pose.p.clone()
        g[(e % 2) == 1] += torch.tensor([0.1, 0.1, 0.1], device=dev)
        base.goal_site.set_pose(Pose.create_from_pq(g))
        act[((e // 2) % 2) == 1, 0] = 1.0
        act[((e // 4) % 2) == 1, 7] = 1.0
    elif task == "stack":  # A held on B: B stays / is moved away x hold / release
        away = (e % 2) == 1
        pb = base.cubeB.pose.p.clone()
        pb[away] += torch.tensor([0.15, 0.2, 0.0], device=dev)
        base.cubeB.set_pose(Pose.create_from_pq(pb, base.cubeB.pose.q.clone()))
        act[((e // 2) % 2) == 1, 7] = 1.0
    elif task == "peg":  # the box brought to the held peg: head inserted / aligned in front of the hole / off the axis / released
        S = snapshot(base)
        P = params(task, base)
        table = _cases_peg(P)[0]
        by_label = {lab: fns for lab, fns in table}
        names = ["inserted", "aligned, far", "not aligned", "inserted"]
        for i in range(N):
            for fn in by_label[names[i % 4]]:
                fn(S, i)
        box = torch.from_numpy(S["rigid"][P["box_row"], :, :7].copy()).to(dev)
        base.box.set_pose(Pose.create_from_pq(box[:, :3], box[:, 3:]))
        act[(e % 4) == 3, 7] = 1.0
    elif task == "push":  # the hand low over the table, the cube in front of it (near) or 10 cm off x the goal on / off the cube
        grasp_p = torch.tensor([0.0, 0.0, 0.02], device=dev)
        key = (0.02,)
        if key not in _IK_CACHE:
            q_pre = _ik(base, torch.tensor([REST], dtype=torch.float32, device=dev), grasp_p + torch.tensor([0, 0, 0.10], device=dev))
            _IK_CACHE[key] = (q_pre.cpu(), _ik(base, q_pre, grasp_p).cpu())
        q = _IK_CACHE[key][1].to(dev).expand(N, -1).contiguous()
        base.agent.robot.set_qpos(q)
        base.agent.robot.set_qvel(torch.zeros(N, 9, device=dev))
        _sync(base)
        half = float(base.cube_half_size)
        po = base.agent.tcp.pose.p.clone() + torch.tensor([half + 0.005, 0.0, 0.0], device=dev)
        po[:, 2] = half
        po[(e % 2) == 1, 1] += 0.1
        base.obj.set_pose(Pose.create_from_pq(po, ident))
        base.obj.set_linear_velocity(torch.zeros(N, 3, device=dev))
        base.obj.set_angular_velocity(torch.zeros(N, 3, device=dev))
        pg = po.clone()
        pg[:, 2] = 1e-3
        pg[((e // 2) % 2) == 1, 0] += 0.3
        base.goal_region.set_pose(Pose.create_from_pq(pg, base.goal_region.pose.q.clone()))
        act = torch.zeros_like(hold)
        act[:, 7] = 1.0
        base.agent.controller.reset()
    elif task == "pusht":  # the tee on the goal in every other env
        gp = base.goal_tee.pose.raw_pose
        tp = base.tee.pose.raw_pose.clone()
        on = (e % 2) == 0
        tp[on, :2] = gp[on, :2]
        tp[on, 2] = 0.021
        tp[on, 3:] = gp[on, 3:]
        base.tee.set_pose(Pose.create_from_pq(tp[:, :3], tp[:, 3:]))
        base.tee.set_linear_velocity(torch.zeros(N, 3, device=dev))
        base.tee.set_angular_velocity(torch.zeros(N, 3, device=dev))
    _sync(base)
    base.scene.px.wake_all()
    return act.contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# case tables. A case is (label, [fn(S, e)]) writing env e of the snapshot; `expect` collects the hand-written booleans
# of the exact-edge cases: {env: {flag: bool}}.
def _rot_x90(q):
    """q * (rotation by 90 degrees about x): the frame's y axis goes to its old z axis"""
    s = math.sqrt(0.5)
    w, x, y, z = (float(v) for v in q)
    return np.array([s * (w - x), s * (x + w), s * (y + z), s * (z - y)], f32)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


DIAG = _unit([0.36, -0.48, 0.8])


def _set(S, row, e, p=None, q=None, v=None, w=None):
    R = S["rigid"]
    if p is not None:
        R[row, e, 0:3] = np.asarray(p, f32)
    if q is not None:
        R[row, e, 3:7] = np.asarray(q, f32)
    if v is not None:
        R[row, e, 7:10] = np.asarray(v, f32)
    if w is not None:
        R[row, e, 10:13] = np.asarray(w, f32)


def _turn_finger(P, which):
    row = P[which]
    return lambda S, e: _set(S, row, e, q=_rot_x90(S["rigid"][row, e, 3:7]))


def _quat_y_to(d):
    """a unit quaternion whose frame has its y axis along the unit vector d (shortest arc from (0, 1, 0))"""
    y = np.array([0.0, 1.0, 0.0])
    c = float(y @ d)
    if c < -1 + 1e-9:
        return np.array([0, 1.0, 0, 0])
    ax = np.cross(y, d)
    q = np.array([1 + c, *ax])
    return q / np.linalg.norm(q)


def _finger_at_angle(P, obj_key, which, s):
    """turns one finger's row so that its closing axis makes max_angle * s with the force measured on it (nothing to do in
    a batch without contact forces)"""
    def f(S, e):
        lf, rf = ref.finger_forces(ref._f64(S), P[obj_key], P["finger1_row"], P["finger2_row"])
        force = (lf if which == "finger1_row" else rf)[e]
        n = np.linalg.norm(force)
        if n < 1e-6:
            return
        fdir = force / n
        u = np.cross(fdir, [0.3, 0.5, 0.81])
        u /= np.linalg.norm(u)
        th = math.radians(P["max_angle_deg"] * s)
        d = math.cos(th) * fdir + math.sin(th) * u
        _set(S, P[which], e, q=_quat_y_to(d if which == "finger1_row" else -d))
    return f


def _grasp_cases(P, obj_key, pre=()):
    """the finger predicates: one finger turned away, each finger's angle at max_angle x (1 +- 1e-3). (The force
    predicate's two sides are reached by task structs whose min_force is a measured force x (1 +- 1e-3).)"""
    C = [("left finger turned away", [*pre, _turn_finger(P, "finger1_row")]), ("right finger turned away", [*pre, _turn_finger(P, "finger2_row")])]
    for which in ("finger1_row", "finger2_row"):
        for s in (1 - 1e-3, 1 + 1e-3):
            C.append((f"{which} angle x {s}", [*pre, _finger_at_angle(P, obj_key, which, s)]))
    return C


def _cases_pick(P):
    thr, st = P["goal_thresh"], P["static_thresh"]
    o, g, ns = P["obj_row"], P["goal_row"], P["n_static_dofs"]
    C, X = [], {}

    def goal_at(d, direction=DIAG):
        return lambda S, e: _set(S, g, e, p=S["rigid"][o, e, :3].astype(np.float64) + d * np.asarray(direction))

    def qv(v, j=3):
        def f(S, e):
            S["qvel"][e, :] = 0.01
            S["qvel"][e, j] = v
        return f

    for placed in (True, False):
        for static in (True, False):
            C.append((f"placed={placed} static={static}", [goal_at(0.5 * thr if placed else 3 * thr), qv(0.5 * st if static else -2.5 * st)]))
    for s in (1 - 1e-3, 1 + 1e-3):
        C.append((f"goal distance x {s}", [goal_at(s * thr), qv(0.0)]))
        C.append((f"qvel x {s}", [goal_at(0.5 * thr), qv(s * st, j=ns - 1)]))
    C.append(("finger joint velocity is not read", [goal_at(0.5 * thr), qv(5.0, j=ns)]))
    C += _grasp_cases(P, "obj_row")
    # exact edges: object at the origin, goal on an axis at the threshold (<=), one joint at the static threshold (<=)
    for k, (d, v, exp) in enumerate(((thr, st, (True, True)), (up(thr), st, (False, True)), (thr, up(st), (True, False)), (down(thr), -st, (True, True)))):
        def f(S, e, d=d, v=v):
            _set(S, o, e, p=[0, 0, 0])
            _set(S, g, e, p=[0, d, 0])
            S["qvel"][e, :] = 0
            S["qvel"][e, 2] = v
        C.append((f"exact edge {k}", [f]))
        X[len(C) - 1] = dict(is_obj_placed=exp[0], is_robot_static=exp[1], success=exp[0] and exp[1])
    return C, X


def _cases_push(P):
    rad, half = P["goal_radius"], P["cube_half_size"]
    t, o, g = P["tcp_row"], P["obj_row"], P["goal_row"]
    C, X = [], {}

    def state(d_goal, z, d_push, direction=(0.6, 0.8)):
        def f(S, e):
            po = S["rigid"][o, e, :3].astype(np.float64)
            po[2] = z
            _set(S, o, e, p=po)
            po = S["rigid"][o, e, :3].astype(np.float64)
            _set(S, g, e, p=[po[0] + d_goal * direction[0], po[1] + d_goal * direction[1], 1e-3])
            _set(S, t, e, p=po + np.array([-half - 0.005, 0, 0]) + d_push * DIAG)
        return f

    zt = half + 5e-3
    for near in (True, False):
        for inside in (True, False):
            for low in (True, False):
                C.append((f"near={near} inside={inside} low={low}", [state(0.5 * rad if inside else 2 * rad, half if low else half + 0.03, 0.004 if near else 0.05)]))
    for s in (1 - 1e-3, 1 + 1e-3):
        C.append((f"goal radius x {s}", [state(s * rad, half, 0.05)]))
        C.append((f"lift x {s}", [state(0.5 * rad, s * zt, 0.05)]))
        C.append((f"push distance x {s}", [state(2 * rad, half, s * 0.01)]))
    # exact edges (<): cube at the origin, goal on the x axis exactly at / next to the radius
    for k, (d, exp) in enumerate(((rad, False), (down(rad), True), (up(rad), False))):
        def f(S, e, d=d):
            _set(S, o, e, p=[0, 0, half])
            _set(S, g, e, p=[d, 0, 0.001])
            _set(S, t, e, p=[0.25, 0.25, 0.25])
        C.append((f"exact edge {k}", [f]))
        X[len(C) - 1] = dict(inside=exp, success=exp)
    # the lift predicate z < half + 5 mm: the threshold is float32(half + 0.005) as the torch path forms it (the sum in
    # double, rounded once); a cube exactly there is not low, one float below it is
    zt32 = float(f32(float(half) + 5e-3))
    for k, (z, exp) in enumerate(((zt32, False), (down(zt32), True))):
        def f(S, e, z=z):
            _set(S, o, e, p=[0, 0, z])
            _set(S, g, e, p=[0, 0, 0.001])
            _set(S, t, e, p=[0.25, 0.25, 0.25])
        C.append((f"exact edge lift {k}", [f]))
        X[len(C) - 1] = dict(low=exp, success=exp)
    return C, X


def _cases_stack(P):
    half = P["cube_half_size"]
    a, b = P["cubeA_row"], P["cubeB_row"]
    C, X = [], {}

    def b_under(dxy, dz, direction=(0.8, -0.6)):
        """cube B placed so that A - B = (dxy * direction, dz)"""
        return lambda S, e: _set(S, b, e, p=S["rigid"][a, e, :3].astype(np.float64) - np.array([dxy * direction[0], dxy * direction[1], dz]))

    vel = lambda v, w: (lambda S, e: _set(S, a, e, v=v * _unit([1, 2, -2]), w=w * _unit([2, -1, 2])))
    lin, ang, xy, zt = P["static_lin_thresh"], P["static_ang_thresh"], P["on_xy_thresh"], P["on_z_thresh"]
    for on in (True, False):
        C.append((f"on={on} static", [b_under(0.3 * xy if on else 3 * xy, 2 * half), vel(0.0, 0.0)]))
        C.append((f"on={on} moving, linear only", [b_under(0.3 * xy if on else 3 * xy, 2 * half), vel(3 * lin, 0.2 * ang)]))
        C.append((f"on={on} moving, angular only", [b_under(0.3 * xy if on else 3 * xy, 2 * half), vel(0.2 * lin, 3 * ang)]))
        C.append((f"on={on} moving, both", [b_under(0.3 * xy if on else 3 * xy, 2 * half), vel(3 * lin, 3 * ang)]))
    C.append(("too high", [b_under(0.0, 2 * half + 3 * zt), vel(0, 0)]))
    C.append(("too low", [b_under(0.0, 2 * half - 3 * zt), vel(0, 0)]))
    for s in (1 - 1e-3, 1 + 1e-3):
        C.append((f"xy x {s}", [b_under(s * xy, 2 * half), vel(0, 0)]))
        C.append((f"z above x {s}", [b_under(0.0, 2 * half + s * zt), vel(0, 0)]))
        C.append((f"z below x {s}", [b_under(0.0, 2 * half - s * zt), vel(0, 0)]))
        C.append((f"linear x {s}", [b_under(0.0, 2 * half), vel(s * lin, 0)]))
        C.append((f"angular x {s}", [b_under(0.0, 2 * half), vel(0, s * ang)]))
    C += _grasp_cases(P, "cubeA_row", pre=(b_under(0.0, 2 * half), vel(0, 0)))
    # exact edges (<=): B at the origin, A on an axis; one velocity component at the threshold
    for k, (dx, v, w, exp) in enumerate(((xy, lin, 0.0, (True, True)), (up(xy), 0.0, ang, (False, True)), (xy, up(lin), 0.0, (True, False)), (0.0, 0.0, up(ang), (True, False)))):
        def f(S, e, dx=dx, v=v, w=w):
            _set(S, b, e, p=[0, 0, 0])
            _set(S, a, e, p=[dx, 0, float(f32(2) * f32(half))], v=[0, v, 0], w=[0, 0, w])
        C.append((f"exact edge {k}", [f]))
        X[len(C) - 1] = dict(is_cubeA_on_cubeB=exp[0], is_cubeA_static=exp[1])
    return C, X


def _qz(yaw):
    return np.array([math.cos(yaw / 2), 0, 0, math.sin(yaw / 2)], f32)


def _cases_peg(P):
    C, X = [], {}
    pg, bx = P["peg_row"], P["box_row"]

    def place(dx=0.0, dy=0.0, dz=0.0, tilt=0.0):  # (each may be a function of the env index)
        """the peg stays where it is (as grasped); the BOX is moved so that the peg's head sits at (dx, dy, dz) in the hole
        frame, the hole frame being the world frame turned by `tilt` about z (misaligns body and head differently)"""
        def f(S, e):
            hs, hoff = np.asarray(P["peg_half_sizes"][e], np.float64), np.asarray(P["box_hole_offsets"][e], np.float64)
            pq = (S["rigid"][pg, e, :3].astype(np.float64)[None], S["rigid"][pg, e, 3:7].astype(np.float64)[None])
            head = ref.pose_mul(pq, (np.array([[hs[0], 0, 0]]), np.array([[1.0, 0, 0, 0]])))[0][0]
            tl = tilt(e) if callable(tilt) else tilt
            Rb = np.array([[math.cos(tl), -math.sin(tl), 0], [math.sin(tl), math.cos(tl), 0], [0, 0, 1]])
            dd = np.array([dx(e) if callable(dx) else dx, dy(e) if callable(dy) else dy, dz(e) if callable(dz) else dz])
            _set(S, bx, e, p=head - Rb @ dd - Rb @ hoff, q=_qz(tl))
        return f

    rad = lambda s: (lambda e: s * float(P["box_hole_radii"][e]))
    C.append(("inserted", [place(0.0, 0.0, 0.0)]))
    C.append(("right finger turned away", [place(-0.2, 0.004, 0.003), _turn_finger(P, "finger2_row")]))
    C.append(("too shallow", [place(-0.03, 0.0, 0.0)]))
    C.append(("y outside", [place(0.0, rad(2), 0.0)]))
    C.append(("z outside", [place(0.0, 0.0, rad(-2))]))
    C.append(("aligned, far", [place(-0.2, 0.004, 0.003)]))
    C.append(("head aligned, body not", [place(-0.2, 0.002, 0.0, tilt=0.12)]))
    C.append(("not aligned", [place(-0.2, 0.05, 0.02)]))
    for s in (1 - 1e-3, 1 + 1e-3):
        C.append((f"depth x {s}", [place(-0.015 * s, 0.0, 0.0)]))
        C.append((f"y x {s}", [place(0.0, rad(s), 0.0)]))
        C.append((f"z x {s}", [place(0.0, 0.0, rad(-s))]))
        C.append((f"alignment x {s}", [place(-0.2, 0.006 * s, 0.008 * s)]))
        # one alignment predicate at a time: in the hole frame turned by t the peg's axis is (cos t, -sin t, 0), so the
        # body's offset is the head's plus half_x sin t
        hsx = lambda e: float(P["peg_half_sizes"][e][0])
        C.append((f"head alignment x {s}", [place(-0.2, 0.01 * s, 0.0, tilt=lambda e, s=s: -math.asin((0.01 * s - 0.002) / hsx(e)))]))
        C.append((f"body alignment x {s}", [place(-0.2, 0.002, 0.0, tilt=lambda e, s=s: math.asin((0.01 * s - 0.002) / hsx(e)))]))
    C += _grasp_cases(P, "peg_row", pre=(place(-0.2, 0.004, 0.003),))[2:]
    # exact edges (>= for the depth): peg and box unrotated, the head at the origin (peg at -half_x), the hole centre on the x
    # axis at c: head_in_hole.x = 0 - c exactly
    for k, (c, exp) in enumerate(((float(f32(0.015)), True), (up(0.015), False), (down(0.015), True))):
        def f(S, e, c=c):
            hs, hoff = P["peg_half_sizes"][e], P["box_hole_offsets"][e]
            _set(S, pg, e, p=[-float(hs[0]), 0, 0], q=[1, 0, 0, 0])
            _set(S, bx, e, p=[c - float(hoff[0]), -float(hoff[1]), -float(hoff[2])], q=[1, 0, 0, 0])
        C.append((f"exact edge {k}", [f]))
        X[len(C) - 1] = dict(deep=exp, success=exp)
    return C, X


def _cases_pusht(P, goal_pose):
    """goal_pose: the goal T's row [7] (position, wxyz). A pose of the tee is given in the goal frame, in pixels."""
    C, X = [], {}
    tr = P["tee_row"]
    gz = 2 * math.acos(float(goal_pose[3]) if goal_pose[6] >= 0 else -float(goal_pose[3]))
    px_m = 1.0 / ref.PUSHT_SCALE

    def tee(dx_px=0.0, dy_px=0.0, dyaw=0.0, neg=False):
        def f(S, e):
            c, s = math.cos(gz), math.sin(gz)
            d = np.array([c * dx_px - s * dy_px, s * dx_px + c * dy_px]) * px_m
            q = _qz(gz + dyaw)
            _set(S, tr, e, p=[goal_pose[0] + d[0], goal_pose[1] + d[1], 0.021], q=-q if neg else q)
        return f

    C.append(("on the goal", [tee()]))
    # exact edge (>=) of the fraction: on the goal the render is the template moved up one row (index y lands on image row
    # 63 - y, the pixel centre of row i has y = 64.5 - i), k = |template & template shifted| pixels; the boolean is written
    # with upstream's float32 division. The second / third parameter sets put the threshold at float32(k / area) and one
    # float above it.
    tmpl = np.asarray(P["consts"]["template"], bool)
    k_on = int((tmpl[1:] & tmpl[:-1]).sum())
    X[0] = dict(success=bool(f32(k_on) / f32(tmpl.sum()) >= f32(P["intersection_thresh"])))
    C.append(("on the goal, -q", [tee(neg=True)]))
    C.append(("turned by pi", [tee(dyaw=math.pi)]))
    for k in (1, 3, 4, 5, 29):  # (pixel centres stay centres or a quarter pixel off them)
        C.append((f"shifted {k}/4 px", [tee(dx_px=0.25 * k, dy_px=-0.25 * k)]))
    C.append(("half in the image", [tee(dx_px=32.25)]))
    C.append(("outside", [tee(dx_px=200.25, dy_px=-150.25)]))
    # (the two cases below exercise the truncation of coordinates in (-1, 0) to index 0, but cannot tell it from floor:
    # index 0 is an image row / column the template does not cover, so the count is the same either way)
    C.append(("columns in (-1, 0)", [tee(dx_px=-21.25, dy_px=0.25)]))
    C.append(("rows in (-1, 0)", [tee(dx_px=0.25, dy_px=-14.25)]))
    for qw in (1.0, -1.0, 0.0):
        qz = math.sqrt(1 - qw * qw)
        C.append((f"q_w = {qw}", [lambda S, e, qw=qw, qz=qz: _set(S, tr, e, q=[qw, 0, 0, qz])]))
        C.append((f"q_w = {qw}, q_z <= -0", [lambda S, e, qw=qw, qz=qz: _set(S, tr, e, q=[qw, 0, 0, -qz])]))
    C.append(("on the goal, yaw with q_z < 0", [tee(dyaw=-2 * math.pi, neg=True)]))
    return C, X


def _random_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _randomize(task, S, e, P, rng, goal_pose=None):
    """one seeded random case over the workspace: positions in a 0.4 m box, unit quaternions of either sign"""
    pos = lambda: rng.uniform([-0.2, -0.2, 0.0], [0.2, 0.2, 0.3])
    S["qpos"][e] += rng.normal(0, 0.05, S["qpos"].shape[1]).astype(f32)
    S["qvel"][e] = rng.normal(0, 0.1, S["qvel"].shape[1]).astype(f32)
    _set(S, P["tcp_row"], e, p=pos(), q=_random_quat(rng))
    if task == "pick":
        po = pos()
        _set(S, P["obj_row"], e, p=po, q=_random_quat(rng))
        _set(S, P["goal_row"], e, p=po + rng.normal(0, 0.02, 3) if rng.random() < 0.5 else pos())
    elif task == "push":
        po = pos()
        po[2] = rng.uniform(0.015, 0.035)
        _set(S, P["obj_row"], e, p=po, q=_random_quat(rng))
        _set(S, P["goal_row"], e, p=[po[0] + rng.normal(0, 0.08), po[1] + rng.normal(0, 0.08), 1e-3])
        if rng.random() < 0.5:
            _set(S, P["tcp_row"], e, p=po + [-P["cube_half_size"] - 0.005, 0, 0] + rng.normal(0, 0.006, 3))
    elif task == "stack":
        pa = pos()
        _set(S, P["cubeA_row"], e, p=pa, q=_random_quat(rng), v=rng.normal(0, 0.008, 3), w=rng.normal(0, 0.3, 3))
        _set(S, P["cubeB_row"], e, p=pa - [rng.normal(0, 0.02), rng.normal(0, 0.02), 0.04 + rng.normal(0, 0.004)] if rng.random() < 0.6 else pos(), q=_random_quat(rng))
    elif task == "peg":
        s1, s2 = 1 + rng.uniform(-1e-3, 1e-3, 2)
        _set(S, P["peg_row"], e, p=pos(), q=_random_quat(rng) * s1)
        qb = _random_quat(rng) * s2
        if rng.random() < 0.5:  # near the hole: the box placed about the peg's head, loosely aligned
            qp = S["rigid"][P["peg_row"], e, 3:7].astype(np.float64)
            qb = (qp + rng.normal(0, 0.02, 4)) * s2
            hs = float(P["peg_half_sizes"][e][0])
            pq = (S["rigid"][P["peg_row"], e, :3].astype(np.float64)[None], qp[None])
            head = ref.pose_mul(pq, (np.array([[hs, 0, 0]]), np.array([[1.0, 0, 0, 0]])))[0][0]
            off = ref._qapply(qb[None], np.asarray(P["box_hole_offsets"][e], np.float64)[None])[0]
            _set(S, P["box_row"], e, p=head - off + rng.normal(0, 0.01, 3), q=qb)
        else:
            _set(S, P["box_row"], e, p=pos(), q=qb)
    elif task == "pusht":
        sign = 1 if rng.random() < 0.5 else -1
        if rng.random() < 0.5:  # near the goal
            g = 2 * math.acos(float(goal_pose[3]) if goal_pose[6] >= 0 else -float(goal_pose[3]))
            q, d = _qz(g + rng.normal(0, 0.15)) * sign, rng.normal(0, 0.004, 2)
        else:
            q, d = _qz(rng.uniform(0, 2 * math.pi)) * sign, rng.normal(0, 0.06, 2)
        _set(S, P["tee_row"], e, p=[goal_pose[0] + d[0], goal_pose[1] + d[1], 0.021], q=q)


def _table(task, P, goal_pose):
    if task == "pusht":
        return _cases_pusht(P, goal_pose)
    return {"pick": _cases_pick, "push": _cases_push, "stack": _cases_stack, "peg": _cases_peg}[task](P)


def build_batch(task, S0, P, seed=0, n_random=None, pick=None):
    """-> (S, labels, expect): the constructed cases in envs 0 .. k-1 (as many as fit; `pick`: only every pick-th case, the
    reduced list of the ragged batches), seeded random cases behind them (`n_random` caps their number; the remaining
    envs keep the state of S0)"""
    S = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in S0.items()}
    N = S["qpos"].shape[0]
    goal_pose = S["rigid"][P["goal_row"], 0, :7].copy() if task == "pusht" else None
    C, X = _table(task, P, goal_pose)
    idx = list(range(len(C)))[:: (pick or 1)][:N]
    labels, expect = [], {}
    for e, k in enumerate(idx):
        for fn in C[k][1]:
            fn(S, e)
        labels.append(C[k][0])
        if k in X:
            expect[e] = X[k]
    rng = np.random.default_rng(seed)
    n_rand = N - len(labels) if n_random is None else min(n_random, N - len(labels))
    for e in range(len(labels), len(labels) + n_rand):
        _randomize(task, S, e, P, rng, goal_pose)
        labels.append("random")
    labels += ["as simulated"] * (N - len(labels))
    return S, labels, expect


# ---------------------------------------------------------------------------------------------------------------------
# comparison of an implementation's outputs with the reference's result, shared by the CPU and GPU test files
# max |torch f32 path - f64 reference| of the reward over all cases of a task, recorded from the output of
# tests/test_task_reference.py (which asserts that they still bound what it measures), rounded up:
#   dense reward       pick 1.63e-7, push 1.26e-7, peg 5.53e-7, stack 2.83e-7, pusht 1.52e-7
#   normalised reward  pick 4.42e-8, push 5.83e-8, peg 7.62e-8, stack 3.53e-8, pusht 4.39e-8
#   Peg's hole pose / head position 7.8e-8
MEASURED = dict(pick=1.7e-7, push=1.3e-7, peg=5.6e-7, stack=2.9e-7, pusht=1.6e-7, peg_pose=8.0e-8)
MEASURED_NORMALIZED = dict(pick=4.5e-8, push=5.9e-8, peg=7.7e-8, stack=3.6e-8, pusht=4.4e-8)


def reward_factor(task, P):
    """what the parameter set multiplies the dense reward by"""
    return 1.0 / P["reward_div"] if task == "pusht" else P["reward_scale"]


def gpu_tolerance(task, P):
    """4 x the measured difference of the two references, for the dense reward or, for a parameter set that scales the
    reward down to [0, 1], the normalised one; never above 2e-5 x the top reward of that parameter set"""
    f = reward_factor(task, P)
    assert f == 1.0 or abs(f * TOP_REWARD[task] - 1) < 1e-6, "a reward factor other than 1 and 1 / top reward has no measured tolerance"
    tol = 4 * (MEASURED if f == 1.0 else MEASURED_NORMALIZED)[task]
    assert tol <= 2e-5 * TOP_REWARD[task] * f
    return tol


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def compare(task, got, R, labels, tol_reward, tol_pose=None, what="torch"):
    """`got` (obs, reward, flags, extras as float32 / bool arrays) against the reference's result R; returns the measured
    float differences"""
    N = len(R["reward"])
    for name, val in got["flags"].items():
        dec = R["decided"][name]
        bad = np.nonzero(dec & (val != R["flags"][name]))[0]
        assert len(bad) == 0, (what, task, name, [(int(e), labels[e], {k: float(m[0][e]) for k, m in R["margins"].items()}) for e in bad[:4]])
    ok = R["reward_decided"] & np.isfinite(R["reward"])
    ex = R["exact"]
    want = R["obs"].astype(np.float32)
    if task == "pick":  # (the is_grasped column where decided)
        n = (want.shape[1] - 24) // 2
        und = ~R["decided"]["is_grasped"]
        want[und, 2 * n] = got["obs"][und, 2 * n]
    fin = np.isfinite(want).all(1)
    bad = np.nonzero(fin[:, None] & ex[None, :] & (_bits(got["obs"]) != _bits(want)) & ~((got["obs"] == 0) & (want == 0)))
    assert len(bad[0]) == 0, (what, task, "obs not bit-exact", [(int(e), int(c), labels[e], float(got["obs"][e, c]), float(want[e, c])) for e, c in zip(*bad)][:4])
    d_r = np.abs(got["reward"].astype(np.float64) - R["reward"])[ok]
    out = dict(reward=float(d_r.max()) if len(d_r) else 0.0)
    assert out["reward"] <= tol_reward, (what, task, "reward", out["reward"], labels[int(np.nonzero(ok)[0][int(d_r.argmax())])])
    if task == "peg":
        d_p = np.abs(got["obs"].astype(np.float64) - R["obs"])[:, ~ex][fin]
        d_h = np.abs(got["head_at_hole"].astype(np.float64) - R["head_at_hole"])[fin]
        out["pose"] = float(max(d_p.max(), d_h.max()))
        assert out["pose"] <= tol_pose, (what, task, "hole pose / head", out["pose"])
    if task == "pusht":
        c = got["count"]
        bad = np.nonzero(fin & ((c < R["count_min"]) | (c > R["count_max"])))[0]
        assert len(bad) == 0, (what, task, "count outside its interval", [(int(e), labels[e], float(c[e]), int(R["count_min"][e]), int(R["count_max"][e])) for e in bad[:4]])
    return out


def assert_expect(R_or_flags, expect, labels, what, decided=None):
    """the hand-written booleans of the exact-edge cases; `decided`: only where that flag is decided (the reference's own
    float64 fraction of PushT at a float32 threshold)"""
    for e, x in expect.items():
        for name, val in x.items():
            if name not in R_or_flags or (decided is not None and not decided[name][e]):
                continue
            assert bool(R_or_flags[name][e]) == val, (what, labels[e], name, val)
