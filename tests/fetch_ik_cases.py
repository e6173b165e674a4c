"""Seeded case tables for the end-effector blocks with held joints (tests/held_ik_reference.py states what must come
out), on the Fetch: `gripper_link`, whose path holds dofs 0, 1, 2 (base x, y, yaw), 3 (torso) -- HELD -- and 5, 7 .. 12
(the seven arm joints) -- SOLVED. The tables mirror tests/ik_cases.py: env counts 128, 1, 17, 67, the table of N envs
is the first N rows of one seeded sequence per (set, rows).

  near  solved q0 = centre + 0.3 u, target = FK(held, clip(q0 + d u', limits -+ 0.05)), d = 0.1 (even) / 0.5 (odd envs);
  wide  solved q0 = centre + 1.0 u, d = 1.0.
The centre is the rest keyframe with shoulder_lift (dof 7) and wrist_flex (dof 11) moved to mid-range -- at rest they sit
0.19 rad and 0.08 rad from a limit, where the clipped iteration stalls at the limit and half of a *near* table would end
at the iteration cap -- and the elbow (dof 9) bent a little further, away from the edge of the arm's reach. Around the
centre *near* never touches a limit and converges in every env; *wide* does touch them.
Held positions are seeded per env: base x, y within +-1 m, yaw within +-pi, the torso within its limits; the target is
the forward kinematics at the SAME held positions, so it is reachable by the arm alone. Unlimited arm joints (the three
rolls) are drawn around the centre like the others and never clipped.
`nan="target"` puts NaN into one position component of the LAST env's target, `nan="held"` into its yaw.

Map form (`build_map`): mode 1 (target-delta, normalised columns; the Fetch has no absolute pose mode). The columns are
those of tests/ik_cases.build_map: seeded uniform in [-1.3, 1.3], so some are clipped, every 5th env commands zero. The
previous target is built backwards from them, so that the NEW target is reachable as the *near* targets are: it is the
forward kinematics of q0 with the arm joints moved by a seeded 0.15 u, and the previous target is that pose with the
clipped and scaled command taken off again (three saturated columns ask for 17 cm at once: from a previous target at
the gripper itself, one env in twenty would be sent beyond the arm's reach with its orientation kept)."""
import numpy as np

from tests import action_cases as ac
from tests import action_reference as ar
from tests import ik_reference as ik

# (chosen so that under the default settings no env of the 128-env tables, *near* or map form, passes within 3 % of the
# tolerance at any iteration of the reference: there one float32 rounding decides whether another step is taken)
SEED = 20261052
HELD = [0, 1, 2, 3]
SOLVED = [5, 7, 8, 9, 10, 11, 12]
PATH = HELD + SOLVED
REST = np.array([0, 0, 0, 0.386, 0, -0.370, 0.562, -1.032, 0.695, 0.955, -0.1, 2.077, 0, 0.015, 0.015])
CENTER = REST.copy()
CENTER[7], CENTER[9], CENTER[11] = 0.15, 1.2, 1.0
ROWS = (3, 6)
SETS = {"near": (0.3, (0.1, 0.5)), "wide": (1.0, (1.0, 1.0))}
ENV_COUNTS = ac.ENV_COUNTS
MAX_N = 1024
K_FORMS = (1, 2, 5)
MODE_OF_ROWS = {3: "pd_ee_target_delta_pos", 6: "pd_ee_target_delta_pose"}
DELTA_MODE_OF_ROWS = {3: "pd_ee_delta_pos", 6: "pd_ee_delta_pose"}

_TABLES = None


def fetch_tables(base=None):
    """(model arrays, gripper_link's index) of the Fetch in Empty-v1; from `base` (an env of that kind) or, without
    one, from an env made on the float64 oracle backend once"""
    global _TABLES
    if base is None and _TABLES is None:
        import maniskill_amd.envs  # noqa: F401  (first: installs the gymnasium stand-in where the real module is absent)
        import gymnasium as gym
        from tests import oracle_backend as ob

        env = gym.make("Empty-v1", robot_uids="fetch", num_envs=1, sim_backend=ob.register("f64", "oracle_f64_fetch_tables"))
        _TABLES = _of(env.unwrapped)
        env.close()
    return _TABLES if base is None else _of(base)


def _of(base):
    A = {k: np.array(v) for k, v in base.scene.model.arrays.items() if k in ("dof_frame", "dof_axis", "dof_type", "dof_parent", "dof_limit", "link_body", "link_frame")}
    link = base.agent.robot.links.index(base.agent.robot.links_map["gripper_link"])
    assert ar.path_dofs(A, link) == PATH
    return A, link


def _fk_pose(A, link, q):
    pe, qe, _ = ar.link_fk_jacobian(A, q, link)
    return np.concatenate([pe, qe], 1)


def _sequence(A, link, name, rows, count):
    spread, ds = SETS[name]
    lim = np.asarray(A["dof_limit"], dtype=np.float64)
    n = len(REST)
    rng = np.random.default_rng([SEED, sum(map(ord, name)), rows])
    u, u2, uh = rng.uniform(-1.0, 1.0, (count, n)), rng.uniform(-1.0, 1.0, (count, n)), rng.uniform(-1.0, 1.0, (count, 4))
    q0 = np.tile(CENTER, (count, 1))
    q0[:, SOLVED] = np.clip(CENTER[SOLVED] + spread * u[:, SOLVED], lim[SOLVED, 0], lim[SOLVED, 1])
    q0[:, 0], q0[:, 1], q0[:, 2] = uh[:, 0], uh[:, 1], np.pi * uh[:, 2]
    q0[:, 3] = 0.5 * (lim[3, 0] + lim[3, 1]) + 0.5 * (lim[3, 1] - lim[3, 0]) * uh[:, 3]
    q0 = q0.astype(np.float32)  # the target is the forward kinematics at the held positions the solver will read
    d = np.where(np.arange(count) % 2 == 0, ds[0], ds[1])[:, None]
    q1 = q0.astype(np.float64)
    q1[:, SOLVED] = np.clip(q1[:, SOLVED] + d * u2[:, SOLVED], lim[SOLVED, 0] - 0.05, lim[SOLVED, 1] + 0.05)
    return q0, _fk_pose(A, link, q1).astype(np.float32)


_CACHE = {}


def build(A, link, name, rows, N, nan=None):
    """-> dict q0 [N, n_dof] f32, target [N, 7] f32 (root frame), labels"""
    key = (name, rows, N > max(ENV_COUNTS))
    if key not in _CACHE:
        _CACHE[key] = _sequence(A, link, name, rows, MAX_N if key[2] else max(ENV_COUNTS))
    q0, target = (x[:N].copy() for x in _CACHE[key])
    labels = [f"fetch {name} rows={rows} N={N} env {e}" for e in range(N)]
    if nan == "target":
        target[N - 1, 1] = np.nan
        labels[N - 1] += " NAN target"
    elif nan == "held":
        q0[N - 1, 2] = np.nan
        labels[N - 1] += " NAN held yaw"
    else:
        assert nan is None
    return dict(q0=q0, target=target, labels=labels, nan=nan)


def build_map(A, link, ikspec, N):
    """ikspec = (link, column0, rows, 1, low, high, rot_scale, flags) -> dict q0, prev_pose [N, 7] f32, columns [N, rows]
    f32 (the block's own columns), labels; see the module docstring"""
    rows, mode, low, high, rot_scale, flags = ikspec[2:]
    assert ikspec[0] == link and mode == 1
    near = build(A, link, "near", rows, N)
    rng = np.random.default_rng([SEED, 77, rows, mode])
    r = rng.uniform(-1.0, 1.0, (max(ENV_COUNTS), 16))[:N]
    cols = (1.3 * r[:, :rows]).astype(np.float32)
    cols[np.arange(N) % 5 == 4] = 0.0
    f = lambda x: float(np.float32(x))
    cmd = ar.ee_command((link, 0, rows, f(low), f(high), f(rot_scale), flags), cols.astype(np.float64))
    q1 = near["q0"].astype(np.float64)
    q1[:, SOLVED] += 0.15 * r[:, 8:15]
    new = _fk_pose(A, link, q1)
    prev = new.copy()
    prev[:, :3] -= cmd[:, :3]
    if rows == 6:
        prev[:, 3:] = ar._qmul(ik.euler_xyz_quat(cmd[:, 3:6]) * np.array([1.0, -1.0, -1.0, -1.0]), new[:, 3:])
    return dict(q0=near["q0"], prev_pose=prev.astype(np.float32), columns=cols,
                labels=[f"fetch map rows={rows} N={N} env {e}" for e in range(N)])
