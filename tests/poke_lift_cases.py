"""Constructed states for the PokeCube and LiftPegUpright epilogues, one case per env index (the table repeats over the
batch), and the glue between an env (oracle-backed on the CPU, HIP on the GPU), tests/poke_lift_reference.py and the native
task structs. Test infrastructure only; snapshot / buffer helpers and the comparison are those of tests/task_cases.py.

A batch is made as tests/task_cases.py makes PickCube's: (1) a scripted grasp of the peg in ALL envs (the finger <-> peg
impulses of the last substep cannot be written from outside, so they are produced physically); (2) the poses / velocities
of the user-visible buffers are overwritten case by case. The impulses stay; an ungrasped case turns a finger's row away.
The tcp stays where the grasp left it and the PEG is placed relative to it, so the same cases serve the copy-out form,
which recomputes the link rows from qpos (there a finger cannot be turned: `link_rows=False` leaves those cases grasped).

Every case is built so that the float64 reference decides each predicate by at least MIN_MARGIN (thresholds are approached
to EDGE = 1e-3, absolute: float32 decides them), and every orientation whose angle atan2(-R01, R00) is read has
hypot(R00, R01) >= MIN_HYPOT. `check` asserts both, compares an implementation with the reference and returns how many envs
it had to leave out, which the tests assert to be 0."""
import math

import numpy as np
import torch

import maniskill_amd.envs  # noqa: F401
from tests import task_cases as tc
from tests.task_cases import DIAG, _set, _turn_finger, f32

ENV_IDS = dict(poke="PokeCube-v1", lift="LiftPegUpright-v1")
TOP_REWARD = dict(poke=10.0, lift=3.0)
OBS_EXTRA = dict(poke=36, lift=14)
N_FLAGS = dict(poke=4, lift=1)
FLAG_NAMES = dict(poke=("success", "is_cube_placed", "is_peg_cube_fit", "is_peg_grasped"), lift=("success",))
EDGE = 1e-3
MIN_MARGIN = 1e-4
MIN_HYPOT = 0.1

# max |torch f32 path (CPU) - f64 reference| over the case tables, recorded from the output of
# tests/test_poke_lift.py::test_torch_path_matches_reference (which asserts that they still bound what it measures),
# rounded up:
#   dense reward       poke 5.07e-7, lift 1.37e-7
#   normalised reward  poke 3.11e-8, lift 6.66e-8
#   PokeCube's metrics (angle_diff up to 3.4 rad, head_to_cube_dist) 1.64e-7
MEASURED = dict(poke=5.1e-7, lift=1.4e-7, poke_metrics=1.7e-7)
MEASURED_NORMALIZED = dict(poke=3.2e-8, lift=6.7e-8)


def make_env(task, N, backend, seed=7, **kw):
    import gymnasium as gym

    env = gym.make(ENV_IDS[task], num_envs=N, sim_backend=backend, **kw)
    env.reset(seed=seed)
    return env


snapshot = tc.snapshot
write_buffers = tc.write_buffers


def scripted_grasp(env, task, close_steps=10):
    """the peg along x under the hand in every env (PokeCube: the cube out of the way), the hand descends with the gripper
    open and closes it on the peg's 5 cm width: the envs end with both fingers pressing the peg"""
    from maniskill_amd.utils.structs.pose import Pose

    base = env.unwrapped
    dev, N = base.device, base.num_envs
    z = float(base.peg_half_width)
    grasp_p = torch.tensor([0.0, 0.0, z], device=dev)
    key = ("poke_lift peg along x", round(z, 4))  # (the cache is shared with tests/task_cases.py: the name keeps the entries apart)
    if key not in tc._IK_CACHE:
        q0 = torch.tensor([tc.REST], dtype=torch.float32, device=dev)
        q_pre = tc._ik(base, q0, grasp_p + torch.tensor([0, 0, 0.10], device=dev))
        tc._IK_CACHE[key] = (q_pre.cpu(), tc._ik(base, q_pre, grasp_p).cpu())
    q_pre, q_grasp = (q.to(dev) for q in tc._IK_CACHE[key])
    ident = torch.zeros(N, 4, device=dev)
    ident[:, 0] = 1
    zero = torch.zeros(N, 3, device=dev)
    bodies = [(base.peg, [0.0, 0.0, z])] + ([(base.cube, [0.3, 0.2, float(base.cube_half_size)])] if task == "poke" else [])
    for body, p in bodies:
        body.set_pose(Pose.create_from_pq(torch.tensor(p, device=dev).repeat(N, 1), ident))
        body.set_linear_velocity(zero)
        body.set_angular_velocity(zero)
    base.agent.robot.set_qpos(q_pre.expand(N, -1).contiguous())
    base.agent.robot.set_qvel(torch.zeros(N, 9, device=dev))
    tc._sync(base)
    base.scene.px.wake_all()
    base.agent.controller.reset()
    for goal, grip, steps in ((q_grasp, 1.0, 25), (q_grasp, -1.0, close_steps)):
        for _ in range(steps):
            a = torch.zeros(N, 8, device=dev)
            a[:, :7] = ((goal[:, :7] - base.agent.robot.get_qpos()[:, :7]) / 0.1).clamp(-1, 1)
            a[:, 7] = grip
            env.step(a.contiguous())


def params(task, base, normalized=False):
    """task parameters as the env's own fused path states them; every float rounded to float32, the value the native
    struct carries"""
    a = base.agent
    r = lambda o: int(o._body_row)
    F = lambda x: float(f32(x))
    P = dict(tcp_row=r(a.tcp), peg_row=r(base.peg), finger1_row=r(a.finger1_link), finger2_row=r(a.finger2_link), peg_half_length=F(base.peg_half_length),
             min_force=F(0.5), max_angle_deg=F(85), reward_scale=F(1 / TOP_REWARD[task]) if normalized else F(1))
    if task == "poke":
        P.update(cube_row=r(base.cube), goal_row=r(base.goal_region), n_static_dofs=a.robot.max_dof - 2, cube_half_size=F(base.cube_half_size),
                 goal_radius=F(base.goal_radius), align_thresh=F(0.05), reach_thresh=F(0.01), static_thresh=F(0.2))
    else:
        P.update(upright_thresh=F(0.08), height_thresh=F(0.005))
    return P


def native_task(task, P):
    from maniskill_amd import native

    return (native.PokeTask if task == "poke" else native.LiftPegTask)(**P)


def torch_outputs(task, base):
    """the torch path on the env's current buffers: what `check` takes"""
    info = base.evaluate()
    obs = base.get_obs(info)
    rew = base.get_reward(obs=obs, action=None, info=info)
    out = dict(obs=obs.cpu().numpy(), reward=rew.cpu().numpy(), flags={k: info[k].cpu().numpy().astype(bool) for k in FLAG_NAMES[task]})
    if task == "poke":
        out["metrics"] = torch.stack([info["angle_diff"], info["head_to_cube_dist"]], 1).cpu().numpy()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# case tables: (label, fn(S, e, link_rows))
def _quat(a, b, c, scale=1.0):
    """the quaternion (wxyz) of Rx(a) Ry(b) Rz(c), times `scale` (a slightly non-unit quaternion, as users set them)"""
    def ax(i, t):
        q = np.zeros(4)
        q[0], q[1 + i] = math.cos(t / 2), math.sin(t / 2)
        return q

    def mul(p, q):
        return np.array([p[0] * q[0] - p[1:] @ q[1:], *(p[0] * q[1:] + q[0] * p[1:] + np.cross(p[1:], q[1:]))])

    return mul(mul(ax(0, a), ax(1, b)), ax(2, c)) * scale


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


def _cases_poke(P):
    t, pg, cb, g = P["tcp_row"], P["peg_row"], P["cube_row"], P["goal_row"]
    hl, half, rad, ns = float(P["peg_half_length"]), float(P["cube_half_size"]), float(P["goal_radius"]), P["n_static_dofs"]
    al, rt, st = float(P["align_thresh"]), float(P["reach_thresh"]), float(P["static_thresh"])
    near = half + 0.005

    def state(d_tcp=0.004, d_head=0.08, dyaw=0.3, d_goal=0.12, vel="static", peg_q=(0.0, 0.0, 0.4), scale=1.0, turn=None):
        """the peg at distance d_tcp from the tcp with orientation Rx Ry Rz(peg_q); the cube at d_head (xy) from the peg's
        (unrotated) head, its yaw the peg head's third angle + dyaw; the goal at d_goal (xy) from the cube"""
        def f(S, e, link_rows):
            pt = S["rigid"][t, e, :3].astype(np.float64)
            _set(S, pg, e, p=pt + d_tcp * DIAG, q=_quat(*peg_q, scale), v=[0, 0, 0], w=[0, 0, 0])
            head = S["rigid"][pg, e, :3].astype(np.float64) + [hl, 0, 0]
            from tests.poke_lift_reference import euler_z
            c = float(euler_z(S["rigid"][pg, e, 3:7][None])[0][0])
            _set(S, cb, e, p=[head[0] + 0.6 * d_head, head[1] - 0.8 * d_head, half], q=_quat(0, 0, c + dyaw), v=[0, 0, 0], w=[0, 0, 0])
            pc = S["rigid"][cb, e, :3].astype(np.float64)
            _set(S, g, e, p=[pc[0] + 0.8 * d_goal, pc[1] + 0.6 * d_goal, 1e-3])
            _qvel(vel, ns, st)(S, e)
            if turn and link_rows:
                _turn_finger(P, turn)(S, e)
        return f

    fit = dict(d_head=0.01, dyaw=0.01)
    C = [
        ("reaching only", state(d_tcp=0.05)),
        ("reach distance inside", state(d_tcp=rt - EDGE)),
        ("reach distance outside", state(d_tcp=rt + EDGE)),
        ("held, far from the cube", state()),
        ("held, angle inside", state(d_head=0.01, dyaw=al - EDGE)),
        ("held, angle outside", state(d_head=0.01, dyaw=al + EDGE)),
        ("held, angle inside (negative)", state(d_head=0.01, dyaw=-(al - EDGE))),
        ("held, angle outside (negative)", state(d_head=0.01, dyaw=-(al + EDGE))),
        ("held, head distance inside", state(d_head=near - EDGE, dyaw=0.01)),
        ("held, head distance outside", state(d_head=near + EDGE, dyaw=0.01)),
        ("fit and held", state(**fit)),
        ("fit, left finger turned away", state(**fit, turn="finger1_row")),
        ("fit, right finger turned away", state(**fit, turn="finger2_row")),
        ("fit, not reached", state(d_tcp=0.05, **fit)),
        ("placed, robot moving", state(**fit, d_goal=0.5 * rad, vel="moving")),
        ("placed, robot moving, not held", state(d_tcp=0.05, d_goal=0.5 * rad, vel="moving")),
        ("placed and static", state(**fit, d_goal=0.5 * rad)),
        ("placed and static, not held", state(d_tcp=0.05, d_goal=0.5 * rad)),
        ("goal radius inside, moving", state(**fit, d_goal=rad - EDGE, vel="moving")),
        ("goal radius outside", state(**fit, d_goal=rad + EDGE)),
        ("placed, qvel inside", state(d_goal=0.5 * rad, vel=1 - 5e-3)),
        ("placed, qvel outside", state(d_goal=0.5 * rad, vel=-(1 + 5e-3))),
        ("placed, finger joint velocity is not read", state(d_goal=0.5 * rad, vel="fingers only")),
        ("angle difference is not wrapped", state(d_head=0.01, dyaw=-3.4, peg_q=(0.0, 0.0, 1.7))),
        ("tilted peg, non-unit quaternions, fit", state(**fit, peg_q=(0.3, -0.4, 1.1), scale=1.0007)),
        ("tilted peg, non-unit quaternions, not aligned", state(d_head=0.01, dyaw=0.2, peg_q=(-0.5, 0.6, -2.0), scale=0.9994)),
    ]
    return C


def _cases_lift(P):
    t, pg = P["tcp_row"], P["peg_row"]
    hl, up, ht = float(P["peg_half_length"]), float(P["upright_thresh"]), float(P["height_thresh"])
    H = math.pi / 2

    def state(q, z=hl, d_tcp=0.004, turn=None, scale=1.0):
        def f(S, e, link_rows):
            pt = S["rigid"][t, e, :3].astype(np.float64)
            p = pt + d_tcp * DIAG
            p[2] = z
            _set(S, pg, e, p=p, q=_quat(*q, scale), v=[0, 0, 0], w=[0, 0, 0])
            if turn and link_rows:
                _turn_finger(P, turn)(S, e)
        return f

    C = [
        ("lying flat, grasped", state((H, 0, 0), z=0.025)),
        ("lying flat, not grasped", state((H, 0, 0), z=0.025, turn="finger1_row")),
        ("upright, angle +", state((H, 0, H))),
        ("upright, angle -", state((H, 0, -H))),
        ("upright, upside down", state((-H, 0, H))),
        ("upright, not grasped", state((H, 0, H), turn="finger2_row")),
        ("upright, too high", state((H, 0, H), z=hl + 0.02)),
        ("upright, too low", state((H, 0, -H), z=hl - 0.02)),
        ("height inside, above", state((H, 0, H), z=hl + ht - EDGE)),
        ("height outside, above", state((H, 0, H), z=hl + ht + EDGE)),
        ("height inside, below", state((H, 0, -H), z=hl - ht + EDGE)),
        ("height outside, below", state((H, 0, -H), z=hl - ht - EDGE)),
        ("tilt inside", state((H, 0, H - (up - EDGE)))),
        ("tilt outside", state((H, 0, H - (up + EDGE)))),
        ("tilt inside, beyond, angle -", state((H, 0.3, -H - (up - EDGE)), scale=1.0006)),
        ("tilt outside, beyond, angle -, not grasped", state((H, 0.3, -H - (up + EDGE)), scale=0.9995, turn="finger1_row")),
        ("leaning, halfway up, far", state((0.7, -0.5, 0.9), z=0.07, d_tcp=0.06, turn="finger2_row")),
        ("leaning, halfway up, far, grasped", state((0.7, -0.5, 0.9), z=0.07, d_tcp=0.06)),
    ]
    return C


TABLES = dict(poke=_cases_poke, lift=_cases_lift)


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


# ---------------------------------------------------------------------------------------------------------------------
def tolerance(task, P):
    """(reward, metrics): 4 x the measured difference of the torch path and the reference, for the dense or the normalised
    reward"""
    f = P["reward_scale"]
    assert f == 1.0 or abs(f * TOP_REWARD[task] - 1) < 1e-6
    return 4 * (MEASURED if f == 1.0 else MEASURED_NORMALIZED)[task], 4 * MEASURED["poke_metrics"]


def check(task, got, R, labels, tol_reward, tol_metrics, what):
    """`got` (obs, reward, flags, PokeCube: metrics) against the reference's result: flags equal, observation entries
    bit-exact, rewards within tol_reward, metrics within tol_metrics. Every predicate of every env must be decided by
    MIN_MARGIN and every angle well-conditioned. Returns (measured reward difference, measured metric difference, number of
    envs left out)."""
    for name, (m, band) in R["margins"].items():
        small = np.nonzero(np.abs(m) < MIN_MARGIN)[0]
        assert len(small) == 0, (what, task, name, "decided by less than MIN_MARGIN", [(int(e), labels[e], float(m[e])) for e in small[:4]])
    flat = np.nonzero(R["hypot"] < MIN_HYPOT)[0]
    assert len(flat) == 0, (what, task, "hypot(R00, R01) below MIN_HYPOT", [(int(e), labels[e], float(R["hypot"][e])) for e in flat[:4]])
    excluded = int((~R["reward_decided"]).sum() + sum(int((~d).sum()) for d in R["decided"].values()))
    out = tc.compare(task, got, R, labels, tol_reward, what=what)
    d_m = 0.0
    if task == "poke":
        d = np.abs(got["metrics"].astype(np.float64) - R["metrics"])
        d_m = float(d.max())
        assert d_m <= tol_metrics, (what, task, "metrics", d_m, labels[int(d.max(1).argmax())])
    return out["reward"], d_m, excluded
