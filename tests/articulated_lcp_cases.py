"""Scene tables of the articulated contact rows against a direct LCP solution (tests/indep_lcp.py::solve_substep_generalized).

Used by tests/test_oracle_articulated_lcp.py (f64 and f32 oracle, CPU) and tests/test_gpu_articulated_lcp.py (HIP kernel).
Every scene is one fixed-base articulation carrying ONE box per contacting link, plus free boxes; it runs as a batch of
N = 5 envs (a full 4-env wave plus a lone env) that differ in one swept parameter, so that neighbours in a wave take different
branches (stick / slide, limit row active or not, drive saturated or not). One substep from the scene's state, compiled with
`position_iterations = SWEEPS, sleep_threshold = 0`; the reference is solved env by env.

All contacts are box faces (or a box on the ground plane) with gap 0 up to the float32 rounding of the state: a penetrating
gap is never used (the velocity the solver keeps is then one unbiased sweep after the biased ones, not an LCP solution). The
contact points are the corners of the overlap rectangle of the two faces, computed in float64 by the reference's own FK
(tests/indep_dynamics.py::urdf_link_poses) from the float32-rounded state the solvers are given.

Why the scenes are what they are -- a scene is of use only if the problem has ONE velocity solution to compare with:
  * A body held between TWO faces can turn about the faces' normal: such a rotation moves no corner along the normal, so the split
    of a face's normal force over its four corners is free; put on two corners alone it leaves the others without friction and the
    body pivots about that edge (Lemke found this for a two-pad hold: 1.65 rad/s). Every pair of such a body carries a torsional row
    that HOLDS (patch_radius 0.1, as the Panda's fingers have): its bound depends on the sum of the normal multipliers only.
  * The torsional row is driven past its bound where the body has ONE loaded face (turntable_twist: a cube resting on the pad of a
    revolute link and spinning about its axis; the row has a joint column). There the split is fixed by the body's own balance up
    to the diagonal mode, which moves neither the net friction force nor its moment. A squeezed cube twisted past the bound has
    several solutions (Lemke from two covering vectors: 0.07 rad/s and 0.03 m/s apart) and is not used. The step API has a force
    per body but no torque: the envs sweep the cube's initial spin (the same LCP: the impulse needed to stop it).
  * slider_push / slider_limit: the pad-cube pair is frictionless (pad and cube mu 0, ground mu 0.6: the pair averages are 0 and
    0.3). With friction on the pad's face the sliding cube's weight could be carried by the ground or, in part, by friction on
    that face, and the ground's friction bound would change with it. Friction on link rows is in all the other scenes.
  * Of the pair impulses of a held body only some parts are unique (the faces share the load as they like): each pair's normal
    part, a friction axis the pair slides along, and the net impulse on the body. `compared_parts` picks them; `Scene.tangent_unique`
    marks the envs whose whole pair impulses are unique. tests/test_oracle_articulated_lcp.py constructs a second solution
    wherever a part is left out.
  * The drive force limit belongs to the model, not to an env: every env of two_pad_hold / two_pad_slip has it, the first three
    stay below it, then one pad saturates, then both.
  * two_pad_* and panda_pinch_* squeeze with unequal targets, so that pads and box move: at rest neither a saturated joint's A nor
    the tendon's off-diagonal would show in any velocity.
  * A scene is admitted only if the f64 oracle meets TOL_V_F64 / TOL_I_F64 within `Scene.sweeps` sweeps at the product's
    MSSIM_PGS_EXIT_TOLERANCE. A stiff arm whose pad can rock on what it presses (the Fetch's arm pressing a pad on the ground,
    hung 0.98 m below the gripper and pressed through shoulder_lift, or 0.09 m below it and pressed with J^T f by every joint;
    panda_stick pressing a 1 kg cube on the ground, or pushing one along the ground) leaves the sweeps at that tolerance while
    they still crawl (1.6e-4, 2.9e-4, 3.9e-4 and 1.5e-4 off, unchanged by 16 times the sweeps; 4.8e-7 with the tolerance at 1e-10):
    such scenes pin nothing and are not here. The Fetch touches the ground with a pad under its torso, which
    cannot rock; panda_stick pushes a cube that floats.
  * panda_stick's hand has no <inertial>: the compiled model gives it the mass of its collision shapes at 1000 kg/m^3 -- here the
    pad alone. The reference states the same in closed form (`shape_inertial`: the box's mass and inertia at the pad's pose), it
    does not read the compiled model.
  * The cube under the level arm weighs 1 kg and the arm's revolute drives are 200 / 20: with a 0.064 kg cube under kp 1e3 the
    sweeps stop at their exit tolerance while the cube still rocks by 1e-3 rad/s.
"""
import copy
import os
from dataclasses import dataclass, field, replace
from typing import Dict, List, Optional, Tuple

import numpy as np

from maniskill_amd.model import geom
from maniskill_amd.model.compile import SHAPE_TRIMESH, ActorRecord, ArticulationRecord, SceneModelBuilder, ShapeRecord
from maniskill_amd.model.scenes import PANDA_URDF, ground_record
from maniskill_amd.model.urdf import parse_urdf
from tests import indep_lcp
from tests.indep_dynamics import active_joint_names, link_point_jacobian, mass_matrix_and_bias, urdf_link_poses

DT, G, N = 0.01, 9.81, 5
SWEEPS = 400   # position_iterations: the sweeps must have stopped at MSSIM_PGS_EXIT_TOLERANCE before (asserted on the oracle)
H = 0.02       # half size of the free cubes unless a scene says otherwise
INF = float("inf")

# ---- bounds ---------------------------------------------------------------------------------------------------------
# f64 oracle against the direct solution: the free-body test's bounds (tests/test_oracle_lcp.py): the sweeps stop once one
# moves no velocity component by more than 1e-6, what is left is a small multiple of that.
TOL_V_F64, TOL_I_F64 = 2e-5, 2e-6
# Per-scene exceptions of the f64 bounds: a scene that does not meet them gets TWICE its own measured figure, no more.
# Both are impulses on a driven pad, whose A = m + dt kd + dt^2 kp = 2.1 kg turns the sweeps' velocity residual into 33 times the
# impulse it is on a 0.064 kg cube, for which the 2e-6 was set:
TOL_F64: Dict[str, Tuple[float, float]] = {
    "slider_push": (TOL_V_F64, 2 * 3.26e-6),   # measured 3.26e-6 N s (the pad-cube pair of the sliding envs)
    "two_pad_hold": (TOL_V_F64, 2 * 1.11e-5),  # measured 1.11e-5 N s (the normal part of a pad-cube pair)
}
# f32 oracle against the direct solution, largest error over the scene's envs (velocity: joint, linear and angular
# components alike [m/s | rad/s]; impulse per body pair [N s]), measured on the CPU by
# `pytest tests/test_oracle_articulated_lcp.py -k f32 -s`: from the f32 oracle alone, no figure of the HIP kernel enters a bound.
F32_ORACLE_ERROR: Dict[str, Tuple[float, float]] = {
    "slider_push": (1.38e-05, 2.90e-06),
    "slider_limit": (4.44e-06, 1.07e-06),
    "level_arm_press": (6.73e-06, 2.74e-06),
    "level_arm_three_cubes": (1.70e-05, 2.74e-06),
    "two_pad_hold": (3.37e-05, 1.96e-05),
    "two_pad_slip": (1.52e-05, 1.64e-06),
    "turntable_twist": (2.12e-06, 3.06e-09),
    "panda_pinch_tendon": (6.75e-05, 4.32e-06),
    "panda_pinch_no_tendon": (6.76e-05, 4.33e-06),
    "panda_pinch_two_cubes": (2.16e-05, 2.47e-06),
    # the scenes of the other plain instances, measured the same way
    "fetch_pinch": (3.19e-06, 2.87e-07),
    "fetch_pinch_two_cubes": (1.20e-05, 7.87e-08),
    "fetch_ground_press": (2.11e-09, 2.39e-07),
    "fetch_limits": (1.05e-08, 0.0),   # (no contact: no impulse to compare)
    "stick_drag": (6.76e-06, 2.83e-06),
    "branch_arm_two_cubes": (1.70e-05, 2.74e-06),
    "slider_push_on_mesh": (5.32e-06, 2.18e-06),
    "level_arm_press_on_mesh": (9.41e-07, 1.40e-06),
}
FACTOR = 4.0  # the project's convention: a kernel's bound is four times the f32 ORACLE's error, never the kernel's own
# a family's bound is that of its worst scene
FAMILY = {
    "slider_push": "slider", "slider_limit": "slider",
    "level_arm_press": "level_arm", "level_arm_three_cubes": "level_arm",
    "two_pad_hold": "two_pad", "two_pad_slip": "two_pad", "turntable_twist": "turntable",
    "panda_pinch_tendon": "panda", "panda_pinch_no_tendon": "panda", "panda_pinch_two_cubes": "panda",
    "fetch_pinch": "fetch", "fetch_pinch_two_cubes": "fetch", "fetch_ground_press": "fetch", "fetch_limits": "fetch",
    "stick_drag": "stick", "branch_arm_two_cubes": "branch_arm",
    "slider_push_on_mesh": "mesh_ground", "level_arm_press_on_mesh": "mesh_ground",
}
# The families above the first ten scenes' have a floor under their bound: the f64 allowance. That allowance is there because the
# sweeps stop at MSSIM_PGS_EXIT_TOLERANCE, and the kernel stops at the same tolerance: a scene whose f32 oracle happens to land
# 1e-9 from the answer (fetch_ground_press, fetch_limits) must not become a 1e-8 bound on float32 hardware.
FLOORED = ("fetch", "stick", "branch_arm", "mesh_ground")


def measured_bounds(name):
    fam = [s for s, f in FAMILY.items() if f == FAMILY[name]]
    v, i = FACTOR * max(F32_ORACLE_ERROR[s][0] for s in fam), FACTOR * max(F32_ORACLE_ERROR[s][1] for s in fam)
    return (max(v, TOL_V_F64), max(i, TOL_I_F64)) if FAMILY[name] in FLOORED else (v, i)


MESH_GROUND = [[-2.0, -2.0, 0.0], [4.0, -2.0, 0.0], [-2.0, 4.0, 0.0]]  # the one triangle of the "ground" variants, seen from +z counter-clockwise
MEASURED_V = {s: measured_bounds(s)[0] for s in FAMILY}
MEASURED_I = {s: measured_bounds(s)[1] for s in FAMILY}


# ---- scene description ------------------------------------------------------------------------------------------------
@dataclass
class FreeBox:
    name: str
    half: Tuple[float, float, float]
    gravity: bool = True
    mu: float = 0.3
    patch_radius: float = 0.0


@dataclass
class Scene:
    name: str
    urdf: Optional[str]                      # URDF text of a custom robot; None: the vendored Panda
    pads: Dict[str, ShapeRecord]             # link -> its one box
    drives: Dict[str, Tuple[float, float, float, int]]
    frees: List[FreeBox]
    ground_mu: Optional[float]               # None: no ground
    pairs: List[Tuple[object, object, int]]  # face contacts (side a, side b, axis of the normal): a link name, a free index, or -1 = ground
    q: np.ndarray                            # [N, n_dof]
    q_target: np.ndarray                     # [N, n_dof]
    pos: np.ndarray                          # [N, n_free, 3] box centres
    force: np.ndarray                        # [N, n_free, 3]
    spin: np.ndarray                         # [N, n_free, 3]
    swept: str = ""                          # which of q_target / force / spin / q the envs sweep (the +-1 % test scales it)
    root_p: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    mimic: bool = False
    instance: Tuple[int, int, bool] = (0, 1, False)  # (NDOF, NR, TRI) of the k_solve16 instance the scene runs
    sweeps: int = SWEEPS
    swept_dofs: Optional[Tuple[int, ...]] = None  # swept == "q_target": the joints whose target the envs sweep (None: all)
    # One static triangle mesh in the model, so that plain_step picks the TRI instance. "far": one small triangle metres away
    # from everything (the problem is the base scene's); "ground": the ground plane is replaced by one large triangle at z = 0
    mesh: Optional[str] = None
    base: str = ""                           # the scene whose problem, reference and bounds this one shares (itself unless a variant)
    shape_inertial: Tuple[str, ...] = ()     # links without <inertial>: the reference gives them their pad's mass at 1000 kg/m^3
    # Held between two faces at rest a body's pair impulses are not unique (the faces share the load as they like: an internal
    # stress moves nothing), only each pair's normal component and the net impulse on each body are. False: those are compared
    tangent_unique: Tuple[bool, ...] = (True,) * 5  # per env; where False, a friction axis is still compared if the pair slides along it
    robot: object = field(default=None, repr=False)


def _link(name, mass, i):
    return f'<link name="{name}"><inertial><origin xyz="0 0 0"/><mass value="{mass}"/><inertia ixx="{i}" iyy="{i}" izz="{i}" ixy="0" ixz="0" iyz="0"/></inertial></link>'


def _joint(name, jtype, parent, child, xyz, axis, lower=-10.0, upper=10.0):
    return (f'<joint name="{name}" type="{jtype}"><parent link="{parent}"/><child link="{child}"/><origin xyz="{xyz[0]} {xyz[1]} {xyz[2]}"/>'
            f'<axis xyz="{axis[0]} {axis[1]} {axis[2]}"/><limit lower="{lower}" upper="{upper}" effort="1000" velocity="100"/></joint>')


def _robot(*parts):
    return '<?xml version="1.0"?>\n<robot name="r"><link name="base"/>\n' + "\n".join(parts) + "\n</robot>\n"


def _box(half, mu=0.3, patch_radius=0.0, p=(0, 0, 0)):
    return ShapeRecord("box", geom.pose(list(p)), half_size=np.array(half, dtype=np.float64), static_friction=mu, dynamic_friction=mu,
                       patch_radius=patch_radius, min_patch_radius=patch_radius)


def _rep(x):
    return np.repeat(np.asarray(x, dtype=np.float64)[None], N, axis=0)


PAD_M, KP, KD = 1.0, 1e3, 1e2
A_PAD = PAD_M + DT * KD + DT * DT * KP  # 2.1: the scalar A of a driven 1 kg pad


def slider(name):
    """a 1-DOF prismatic pad along +x at cube height pushes a cube (H = 0.04, 0.512 kg) that rests on the ground"""
    h = 0.04
    upper = 0.0002 if name == "slider_limit" else 10.0
    urdf = _robot(_link("pad", PAD_M, 0.01), _joint("j", "prismatic", "base", "pad", (0, 0, h), (1, 0, 0), -10.0, upper))
    m = 1000.0 * (2 * h) ** 3
    fric = 0.3 * m * G  # 1.507 N
    # the pad's drive force at rest is KP * target
    if name == "slider_push":  # sticks below 1.507 N, slides above
        force = np.array([0.5, 1.2, 1.9, 3.0, 6.0])
    else:  # the limit row (C / dt = 0.02 m/s) takes over once the common velocity (KP t - fric) dt / (A + m) passes 0.02: KP t > 6.73 N
        force = np.array([1.0, 3.0, 5.5, 8.5, 20.0])
    return Scene(
        name, urdf, {"pad": _box((0.01, 0.015, 0.015), mu=0.0)}, {"j": (KP, KD, INF, 0)}, [FreeBox("c0", (h, h, h), mu=0.0)], 0.6,
        [(0, -1, 2), (0, "pad", 0)], np.zeros((N, 1)), (force / KP)[:, None], _rep([[0.01 + h, 0, h]]), np.zeros((N, 1, 3)), np.zeros((N, 1, 3)),
        swept="q_target",
    )


def two_pad(name):
    """two opposed prismatic pads along x squeeze a free cube (0.064 kg, weight 0.628 N) in mid-air. Held iff 2 mu F > m g:
    F > 1.046 N. The one-pass force limit looks at the drive torque of the contact-free solution, KP t (1 - 1.1 / 2.1):
    a pad saturates when 0.476 KP t > fmax, and then presses with fmax.
    The pads carry patch_radius 0.1 in all three scenes (as the Panda's fingers do). Without a torsional row a face-held cube has
    MORE THAN ONE velocity solution: a rotation about the pad axis moves no corner along the normal, so the split of a face's
    normal force over its four corners is free; put on the two lower corners alone it leaves the upper ones without friction
    and the cube pivots about the lower edge under its weight -- a valid solution of the same LCP, which Lemke found (1.65 rad/s).
    The torsional bound mu r F = 0.03 F per pad depends on the SUM of the normal multipliers only and exceeds the weight's
    moment about an edge, m g H = 0.0126 N m, from F = 0.21 N on: with it the velocity is unique."""
    pad_half = (0.01, 0.03, 0.03)
    urdf = _robot(
        _link("padl", PAD_M, 0.01), _link("padr", PAD_M, 0.01),
        _joint("jl", "prismatic", "base", "padl", (-(H + pad_half[0]), 0, 0.5), (1, 0, 0)),
        _joint("jr", "prismatic", "base", "padr", (H + pad_half[0], 0, 0.5), (-1, 0, 0)),
    )
    spin = np.zeros((N, 1, 3))
    # The right pad's target is a tenth of the left's: the cube and both pads move along x with v = dt (F_l - F_r) / (A_l + m + A_r), so
    # a saturated pad's A (1 kg instead of 2.1) shows in every velocity; the faces press with N_l = F_l - A_l v / dt, N_r = F_r + A_r v / dt
    if name == "two_pad_hold":  # fmax 5 N: left 3, 4, 5 N free; then left saturated against a free right pad (1.3 N), then both saturated
        fmax, t, r, grav = 5.0, np.array([3e-3, 4e-3, 5e-3, 13e-3, 120e-3]), 0.1, True
    else:  # fmax 0.8 N: left 0.3, 0.5, 0.8 N free; then left saturated against a free right pad (0.22 N), then both saturated
        fmax, t, r, grav = 0.8, np.array([0.3e-3, 0.5e-3, 0.8e-3, 2.2e-3, 20e-3]), 0.1, True
    return Scene(
        name, urdf, {"padl": _box(pad_half, patch_radius=r), "padr": _box(pad_half, patch_radius=r)},
        {"jl": (KP, KD, fmax, 0), "jr": (KP, KD, fmax, 0)}, [FreeBox("c0", (H, H, H), gravity=grav)], None,
        [(0, "padl", 0), ("padr", 0, 0)], np.zeros((N, 2)), np.stack([t, 0.1 * t], axis=1), _rep([[0, 0, 0.5]]), np.zeros((N, 1, 3)), spin,
        swept="q_target", tangent_unique=(False,) * N,
    )


def turntable(name):
    """a cube rests, under gravity, on the pad of a turntable link (revolute about z, PD-driven to rest) and spins about z. The
    pair's torsional row (patch_radius 0.1 on the pad) and the four corners' pyramid stop the relative spin if
    w0 / (1 / I + 1 / A) <= mu m g dt (r + 2 H): with I = 1.707e-5 and A = 0.02 + 1.1 up to 15.7 rad/s. ONE loaded face: the split of
    the normal force over its corners is fixed by the cube's own balance up to the diagonal mode, which moves neither the
    net friction force nor its moment, so the velocity is unique on both sides of the threshold."""
    pad_half = (0.03, 0.03, 0.01)
    urdf = _robot(_link("table", PAD_M, 0.02), _joint("j", "revolute", "base", "table", (0, 0, 0.5), (0, 0, 1), -3.0, 3.0))
    spin = np.zeros((N, 1, 3))
    spin[:, 0, 2] = [4.0, 8.0, 12.0, 19.0, 26.0]
    return Scene(
        name, urdf, {"table": _box(pad_half, patch_radius=0.1)}, {"j": (KP, KD, INF, 0)}, [FreeBox("c0", (H, H, H))], None,
        [(0, "table", 2)], np.zeros((N, 1)), np.zeros((N, 1)), _rep([[0, 0, 0.5 + pad_half[2] + H]]), np.zeros((N, 1, 3)), spin, swept="spin",
    )


L1, L2, Z0 = 0.3, 0.2, 0.4


def level_arm(name):
    """two revolute joints about y with q2 = -q1 keep link 2 level; link 3 slides down from its end and presses its pad on a
    cube on the ground while a side force acts on that cube; in level_arm_three_cubes two more cubes lie beside it, each
    pushed along the ground by a force of its own (21 velocity components: the four-row layout).
    The pad and the pressed cube carry patch_radius 0.1, so both of the cube's loaded faces have a torsional row: a body held
    between two faces has no unique velocity without (see two_pad): it may slide straight or pivot about the normal. The envs sweep q1: the cube(s) stand under the pad of their env."""
    pad_half = (0.03, 0.03, 0.01)
    urdf = _robot(
        _link("l1", 1.0, 0.02), _link("l2", 0.7, 0.01), _link("l3", 0.3, 0.002),
        _joint("j1", "revolute", "base", "l1", (0, 0, Z0), (0, 1, 0), -2.0, 2.0),
        _joint("j2", "revolute", "l1", "l2", (L1, 0, 0), (0, 1, 0), -2.0, 2.0),
        _joint("j3", "prismatic", "l2", "l3", (L2, 0, 0), (0, 0, -1), -1.0, 1.0),
    )
    q1 = np.array([-0.4, -0.15, 0.1, 0.3, 0.5])
    stack = name == "level_arm_three_cubes"
    HB = 0.05    # the pressed cube: 1 kg (a 0.064 kg cube under this arm converges too slowly for the sweeps' exit tolerance)
    top = 2 * HB  # where the pad's lower face has to be
    x = L1 * np.cos(q1) + L2
    z = Z0 - L1 * np.sin(q1)
    q3 = z - pad_half[2] - top
    q = np.stack([q1, -q1, q3], axis=1)
    press = np.array([0.5, 1.0, 2.0, 3.0, 1.5])  # N the slide drive presses with at rest
    qt = q.copy()
    qt[:, 2] += press / KP
    side = np.array([1.5, 5.0, 2.5, 7.0, 2.0])  # N on the cube under the pad; the faces above and below it hold 0.3 P + 0.3 (P + m g) = 3.24, 3.54, 4.14, 4.74, 3.84 N
    frees = [FreeBox("c0", (HB, HB, HB), patch_radius=0.1)]
    pos = [np.stack([x, 0 * x, 0 * x + HB], 1)]
    pairs = [(0, -1, 2), ("l3", 0, 2)]
    if stack:  # the two cubes beside it slide above mu m g = 0.188 N
        frees += [FreeBox("c1", (H, H, H)), FreeBox("c2", (H, H, H))]
        pos += [np.stack([x, 0 * x + 0.15, 0 * x + H], 1), np.stack([x - 0.15, 0 * x - 0.1, 0 * x + H], 1)]
        pairs += [(1, -1, 2), (2, -1, 2)]
    pos = np.stack(pos, axis=1)
    force = np.zeros((N, len(frees), 3))
    force[:, 0, 1] = side
    if stack:
        force[:, 1, 0] = [0.1, 0.4, 0.1, 0.4, 0.1]
        force[:, 2, 1] = [0.3, 0.05, 0.3, 0.12, 0.25]
    nf = len(frees)
    return Scene(
        name, urdf, {"l3": _box(pad_half, patch_radius=0.1)}, {"j1": (200.0, 20.0, INF, 0), "j2": (200.0, 20.0, INF, 0), "j3": (KP, KD, INF, 0)}, frees, 0.3,
        pairs, q, qt, pos, force, np.zeros((N, nf, 3)), swept="force", instance=(0, 4 if stack else 1, False),
        tangent_unique=(False, True, False, True, False),  # the pressed cube slides in envs 1 and 3: everything at its bound
    )


PANDA_ROOT = (-0.615, 0.0, 0.0)
W = 0.02  # finger opening = half width of the pinched box


def panda(name):
    """the vendored Panda, hand pointing down, one box per finger link and nothing else; a box 2 W wide between the pads, no
    ground, gravity on the box, drives kp 1e3, kd 1e2, limit 100. The envs sweep the finger target: the pads press with about
    KP (W - target) each; mu = (2.0 + 0.3) / 2 = 1.15 holds the 0.064 kg box above 0.27 N."""
    rb = parse_urdf(PANDA_URDF)
    two = name == "panda_pinch_two_cubes"
    qa = np.array([0, 0, 0, -np.pi / 2, 0, np.pi / 2, np.pi / 4, W, W])
    pad_half = (0.008, 0.005, 0.008)
    pad_z = 0.045  # along the finger, towards its tip
    pads = {"panda_leftfinger": _box(pad_half, mu=2.0, patch_radius=0.1, p=(0, pad_half[1], pad_z)),
            "panda_rightfinger": _box(pad_half, mu=2.0, patch_radius=0.1, p=(0, -pad_half[1], pad_z))}
    T = urdf_link_poses(rb, qa.astype(np.float32).astype(np.float64), _root_T(PANDA_ROOT))
    tip = 0.5 * (T["panda_leftfinger"][:3, 3] + T["panda_rightfinger"][:3, 3]) + T["panda_leftfinger"][:3, :3] @ np.array([0, 0, pad_z])
    # the box is H_BOX tall; the pads hold its lower part when a second cube rests on it (that one stays clear of the pads by 0.032)
    hz = 0.04 if two else H
    c0 = tip + np.array([0, 0, hz - H]) if two else tip
    frees = [FreeBox("c0", (H, W, hz))] + ([FreeBox("c1", (H, H, H))] if two else [])
    pos = [c0] + ([c0 + np.array([0, 0, hz + H])] if two else [])
    squeeze = np.array([0.1, 0.2, 0.6, 6.0, 60.0]) if not two else np.array([0.2, 0.4, 1.2, 4.0, 12.0])  # N per pad at rest; slip below 0.27 / 0.68 N
    q = _rep(qa)
    qt = q.copy()
    qt[:, 7] = W - squeeze / KP
    qt[:, 8] = W - 0.6 * squeeze / KP  # unequal: the fingers want to move apart by different amounts, which the tendon resists
    pairs = [("panda_leftfinger", 0, 1), (0, "panda_rightfinger", 1)] + ([(1, 0, 2)] if two else [])
    nf = len(frees)
    drives = {j.name: (KP, KD, 100.0, 0) for j in rb.joints if j.type != "fixed"}
    return Scene(
        name, None, pads, drives, frees, None, pairs, q, qt, _rep(np.array(pos)), np.zeros((N, nf, 3)), np.zeros((N, nf, 3)),
        swept="q_target", tangent_unique=(False,) * N, root_p=PANDA_ROOT, mimic=name != "panda_pinch_no_tendon", instance=(9, 2 if two else 1, False), robot=rb,
    )


def branch_arm(name):
    """the level arm (three joints) with a second branch of two revolute links on the same base, driven and moving but touching
    nothing (n_dof = 5: the branch's joints lie in the row, their columns of every contact row are zero and the ancestor masks
    must say so), pressing its pad on a 1 kg cube while a second cube slides beside it: 5 + 12 = 17 velocity components, two free
    bodies -- the generic two-row instance. The envs sweep the side force on the pressed cube, as level_arm_press does."""
    pad_half = (0.03, 0.03, 0.01)
    urdf = _robot(
        _link("l1", 1.0, 0.02), _link("l2", 0.7, 0.01), _link("l3", 0.3, 0.002), _link("b1", 0.8, 0.015), _link("b2", 0.4, 0.004),
        _joint("j1", "revolute", "base", "l1", (0, 0, Z0), (0, 1, 0), -2.0, 2.0),
        _joint("j2", "revolute", "l1", "l2", (L1, 0, 0), (0, 1, 0), -2.0, 2.0),
        _joint("j3", "prismatic", "l2", "l3", (L2, 0, 0), (0, 0, -1), -1.0, 1.0),
        _joint("k1", "revolute", "base", "b1", (0, -0.4, Z0), (0, 0, 1), -2.0, 2.0),
        _joint("k2", "revolute", "b1", "b2", (0.25, 0, 0), (0, 1, 0), -2.0, 2.0),
    )
    q1 = np.array([-0.4, -0.15, 0.1, 0.3, 0.5])
    HB = 0.05
    x = L1 * np.cos(q1) + L2
    z = Z0 - L1 * np.sin(q1)
    q3 = z - pad_half[2] - 2 * HB
    J1, K1, J2, K2, J3 = range(5)  # the joints' rows (links are numbered breadth first): the two branches interleave
    q = np.stack([q1, 0 * q1 + 0.3, -q1, 0 * q1 - 0.2, q3], axis=1)
    press = np.array([0.5, 1.0, 2.0, 3.0, 1.5])
    qt = q.copy()
    qt[:, J3] += press / KP
    qt[:, K1] += 0.01   # the branch is under way: its velocities (0.01 * 200 dt / A) are part of what is compared
    qt[:, K2] -= 0.02
    side = np.array([1.5, 5.0, 2.5, 7.0, 2.0])  # the two faces hold 3.24, 3.54, 4.14, 4.74, 3.84 N (level_arm)
    frees = [FreeBox("c0", (HB, HB, HB), patch_radius=0.1), FreeBox("c1", (H, H, H))]
    pos = np.stack([np.stack([x, 0 * x, 0 * x + HB], 1), np.stack([x, 0 * x + 0.15, 0 * x + H], 1)], axis=1)
    force = np.zeros((N, 2, 3))
    force[:, 0, 1] = side
    force[:, 1, 0] = [0.1, 0.4, 0.1, 0.4, 0.1]  # slides above mu m g = 0.188 N
    drives = {"j1": (200.0, 20.0, INF, 0), "j2": (200.0, 20.0, INF, 0), "j3": (KP, KD, INF, 0), "k1": (200.0, 20.0, INF, 0), "k2": (200.0, 20.0, INF, 0)}
    return Scene(
        name, urdf, {"l3": _box(pad_half, patch_radius=0.1)}, drives, frees, 0.3, [(0, -1, 2), ("l3", 0, 2), (1, -1, 2)], q, qt, pos, force,
        np.zeros((N, 2, 3)), swept="force", instance=(0, 2, False), tangent_unique=(False, True, False, True, False),
    )  # (make_scene asserts the joint order above)


FETCH_URDF = os.path.normpath(os.path.join(os.path.dirname(PANDA_URDF), "..", "fetch", "fetch.urdf"))
FETCH_TORSO, FETCH_R, FETCH_L = 3, 13, 14  # rows of torso_lift and of the two finger joints among the Fetch's 15
FETCH_HALF_GAP = 0.035425  # |y| of a finger frame at q = 0.02: 0.015425 + 0.02


def fetch(name):
    """the vendored Fetch (15 joints: x, y, yaw of the base, torso, head pan, shoulder pan, head tilt, shoulder lift .. wrist roll,
    two fingers; the head branches off the torso between the arm's joints), arm stretched out along +x (q = 0 but torso_lift and the
    fingers), no gravity on the links, every joint driven at 1e3 / 1e2 with force limit 100, no tendon.
      fetch_pinch            a (0.008, 0.005, 0.008) box on each finger link, inner face at the finger frame's origin, mu 2.0,
                             patch_radius 0.1; a free box 2 * 0.035425 wide between them, under gravity. Unequal finger targets, the
                             envs sweep the squeeze: mu 1.15 on 1.6 F holds the 0.113 kg box above F = 0.60 N. Each contact row has the
                             columns x, y, yaw, torso, shoulder pan .. wrist roll and its own finger: 12 or 13 of 15 (head pan / tilt: 0).
      fetch_pinch_two_cubes  the same with a taller box and a second cube resting on it.
      fetch_ground_press     NO free body (15 joints + 6 would be two rows). A (0.03, 0.03, 0.01) pad on torso_lift_link, under
                             the base with its bottom on the ground; the torso drive presses it down with 20 N, the envs sweep the
                             root_y target (swept_dofs): mu 0.45 sticks below 9 N. The pad is centred on the base's yaw axis and has
                             patch_radius 0.1: the links take every tipping moment, so the split of the 20 N over the four corners is
                             free, and a pad that turned about z (0.087 m off the axis it does: the side force's moment) would have a
                             friction moment that depends on the split -- no unique velocity (the f64 oracle and Lemke were 1.3e-3
                             apart); the torsional row, bounded by the SUM, holds the turn. The contact rows' columns: root x, root y,
                             root yaw (per corner) and torso_lift -- 4 of 15; a pad on the arm that reaches the ground through
                             shoulder_lift (11 columns) does not meet the f64 bound, see the module docstring.
      fetch_limits           no contact at all: torso 0.2 mm below its upper limit, the right finger 0.2 mm above its lower, the
                             left one 0.2 mm below its upper, all three targets beyond; the envs scale the three target distances so that
                             the limit rows at dofs 3, 13, 14 of the 15-wide row switch on one after the other."""
    rb = parse_urdf(FETCH_URDF)
    names = active_joint_names(rb)
    assert [names[k] for k in (FETCH_TORSO, FETCH_R, FETCH_L)] == ["torso_lift_joint", "r_gripper_finger_joint", "l_gripper_finger_joint"]
    drives = {j: (KP, KD, 100.0, 0) for j in names}
    qa = np.zeros(15)
    qa[FETCH_TORSO], qa[FETCH_R], qa[FETCH_L] = 0.2, 0.02, 0.02
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    if name == "fetch_limits":
        lim = {k: rb.parent_joint[next(l for l in rb.link_order if l in rb.parent_joint and rb.parent_joint[l].name == names[k])].limit for k in (FETCH_TORSO, FETCH_R, FETCH_L)}
        qa[FETCH_TORSO], qa[FETCH_R], qa[FETCH_L] = lim[FETCH_TORSO][1] - 0.0002, lim[FETCH_R][0] + 0.0002, lim[FETCH_L][1] - 0.0002
        # The contact-free velocity (A^-1 rhs) of a joint whose target is d away is 0.4407 d / s (torso) and 8.49 d / s (a finger): it
        # reaches C / dt = 0.02 m/s at d = 0.0454 m and 0.002356 m. The distances below are those times `scale`: the torso's row
        # switches on from env 1, the right finger's from env 2, the left finger's in env 4; the torso's drive (force limit 100 N: the
        # one-pass check sees 951 d N) saturates in envs 3 and 4, where its row holds a joint that has lost its implicit terms
        scale = np.array([[0.5, 0.5, 0.3], [1.6, 0.7, 0.45], [1.9, 1.5, 0.6], [2.8, 2.2, 0.8], [3.4, 4.0, 1.5]])
        d = scale * np.array([0.0454, 0.002356, 0.002356])
        q = _rep(qa)
        qt = q.copy()
        qt[:, FETCH_TORSO] += d[:, 0]
        qt[:, FETCH_R] -= d[:, 1]
        qt[:, FETCH_L] += d[:, 2]
        return Scene(name, None, {}, drives, [], None, [], q, qt, np.zeros((N, 0, 3)), np.zeros((N, 0, 3)), np.zeros((N, 0, 3)), swept="q_target",
                     instance=(15, 1, False), robot=rb)
    if name == "fetch_ground_press":
        pad_half = (0.03, 0.03, 0.01)
        x_link, _, z_link = urdf_link_poses(rb, f32(qa))["torso_lift_link"][:3, 3]
        pads = {"torso_lift_link": _box(pad_half, mu=0.3, patch_radius=0.1, p=(-x_link, 0, pad_half[2] - z_link))}
        q = _rep(qa)
        qt = q.copy()
        qt[:, FETCH_TORSO] -= 20.0 / KP
        qt[:, 1] = np.array([3.0, 6.0, 8.0, 11.0, 20.0]) / KP  # N sideways at rest; mu (0.3 + 0.6) / 2 on 20 N holds 9 N
        return Scene(name, None, pads, drives, [], 0.6, [("torso_lift_link", -1, 2)], q, qt, np.zeros((N, 0, 3)), np.zeros((N, 0, 3)), np.zeros((N, 0, 3)),
                     swept="q_target", swept_dofs=(1,), instance=(15, 1, False), robot=rb)
    two = name == "fetch_pinch_two_cubes"
    pad_half = (0.008, 0.005, 0.008)
    pads = {"r_gripper_finger_link": _box(pad_half, mu=2.0, patch_radius=0.1, p=(0, pad_half[1], 0)),
            "l_gripper_finger_link": _box(pad_half, mu=2.0, patch_radius=0.1, p=(0, -pad_half[1], 0))}
    T = urdf_link_poses(rb, f32(qa))
    mid = 0.5 * (T["r_gripper_finger_link"][:3, 3] + T["l_gripper_finger_link"][:3, 3])
    hz = 0.04 if two else H
    c0 = mid + np.array([0, 0, hz - H]) if two else mid
    frees = [FreeBox("c0", (H, FETCH_HALF_GAP, hz))] + ([FreeBox("c1", (H, H, H))] if two else [])
    pos = [c0] + ([c0 + np.array([0, 0, hz + H])] if two else [])
    squeeze = np.array([0.2, 0.4, 1.2, 6.0, 60.0]) if not two else np.array([0.4, 0.8, 2.4, 8.0, 24.0])  # N on the right pad at rest; slip below 0.60 / 1.38 N
    q = _rep(qa)
    qt = q.copy()
    qt[:, FETCH_R] = qa[FETCH_R] - squeeze / KP
    qt[:, FETCH_L] = qa[FETCH_L] - 0.6 * squeeze / KP
    pairs = [("r_gripper_finger_link", 0, 1), (0, "l_gripper_finger_link", 1)] + ([(1, 0, 2)] if two else [])
    nf = len(frees)
    return Scene(name, None, pads, drives, frees, None, pairs, q, qt, _rep(np.array(pos)), np.zeros((N, nf, 3)), np.zeros((N, nf, 3)), swept="q_target",
                 tangent_unique=(False,) * N, instance=(15, 2, False), robot=rb)


STICK_URDF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "panda_stick", "panda_stick.urdf")


STICK_DRAG = [0.04, 0.09, 0.14, 0.25, 0.6]  # N along the pad's face: in the first two envs the face's friction rows along y hold, then points slide along them


def stick(name):
    """panda_stick (7 joints, tests/golden/panda_stick), hand pointing down, one (0.015, 0.03, 0.03) box on panda_hand (which has no
    <inertial>: `shape_inertial`), its +x face against a cube (half 0.05, 1 kg) that floats: no ground, no gravity on it. Every
    joint driven at 1e3 / 1e2; the targets are q + J^T f / KP for f = 6 N along x at the pad's face, so the pad pushes the cube away
    with what the arm's inertia leaves of the 6 N, while a force on the cube drags it along the face (y): the envs sweep that
    force, from a cube that goes along with the pad to one that slides on it (mu 0.3). ONE loaded face, as on the turntable: the split of the normal
    force is fixed by the cube's balance up to the diagonal mode. The rows have all seven joint columns (the normal rows none
    for joint 1, the y friction rows one). Pushing a cube ALONG THE GROUND with this pad, the first thing tried, is not here: the
    f64 oracle stays 1.5e-4 from the direct solution at any sweep count, gains 1e3 / 200 / 50, cube 0.5 .. 8 kg, pad face 1 .. 6 cm
    (the cube between the ground's four points and the pad's four rocks by 1e-4 rad/s when the sweeps' exit tolerance stops them)."""
    rb = parse_urdf(STICK_URDF)
    h = 0.05
    qa = np.array([0, 0, 0, -np.pi / 2, 0, np.pi / 2, np.pi / 4])
    qf = qa.astype(np.float32).astype(np.float64)
    pad_half, pad_p = (0.015, 0.03, 0.03), (0.0, 0.0, 0.12)
    Th = urdf_link_poses(rb, qf, _root_T(PANDA_ROOT))["panda_hand"]
    centre = Th[:3, 3] + Th[:3, :3] @ np.array(pad_p)
    face = centre + np.array([pad_half[0], 0, 0])
    Jv, _ = link_point_jacobian(rb, qf, "panda_hand", face, _root_T(PANDA_ROOT))
    q = _rep(qa)
    qt = q + 6.0 * Jv[0][None, :] / KP
    force = np.zeros((N, 1, 3))
    force[:, 0, 1] = STICK_DRAG
    drives = {j: (KP, KD, INF, 0) for j in active_joint_names(rb)}
    return Scene(name, None, {"panda_hand": _box(pad_half, p=pad_p)}, drives, [FreeBox("c0", (h, h, h), gravity=False)], None, [(0, "panda_hand", 0)],
                 q, qt, _rep([[face[0] + h, centre[1], centre[2]]]), force, np.zeros((N, 1, 3)), swept="force", root_p=PANDA_ROOT, instance=(7, 1, False),
                 robot=rb, shape_inertial=("panda_hand",))


SCENES = {
    "slider_push": slider, "slider_limit": slider,
    "level_arm_press": level_arm, "level_arm_three_cubes": level_arm,
    "two_pad_hold": two_pad, "two_pad_slip": two_pad, "turntable_twist": turntable,
    "panda_pinch_tendon": panda, "panda_pinch_no_tendon": panda, "panda_pinch_two_cubes": panda,
    "fetch_pinch": fetch, "fetch_pinch_two_cubes": fetch, "fetch_ground_press": fetch, "fetch_limits": fetch,
    "stick_drag": stick, "branch_arm_two_cubes": branch_arm,
}
# Variants that add ONE static triangle mesh, so that the scene runs the TRI instance of its (NDOF, NR) cell: name -> (base scene,
# Scene.mesh). "far": the problem, its reference (shared) and the bounds are the base scene's. "ground": the plane under the cube
# is one large triangle -- the ground contacts come out of the triangle stage; the reference's problem is the same four corners,
# the bounds are measured for the variant itself (FAMILY "mesh_ground").
VARIANTS = {
    "slider_push_far_mesh": ("slider_push", "far"),                      # (0, 1, T)
    "branch_arm_two_cubes_far_mesh": ("branch_arm_two_cubes", "far"),    # (0, 2, T)
    "level_arm_three_cubes_far_mesh": ("level_arm_three_cubes", "far"),  # (0, 4, T)
    "panda_pinch_tendon_far_mesh": ("panda_pinch_tendon", "far"),        # (9, 1, T)
    "panda_pinch_two_cubes_far_mesh": ("panda_pinch_two_cubes", "far"),  # (9, 2, T)
    "fetch_ground_press_far_mesh": ("fetch_ground_press", "far"),        # (15, 1, T)
    "fetch_pinch_far_mesh": ("fetch_pinch", "far"),                      # (15, 2, T)
    "slider_push_on_mesh": ("slider_push", "ground"),                    # (0, 1, T)
    "level_arm_press_on_mesh": ("level_arm_press", "ground"),            # (0, 1, T)
}
CASES = list(SCENES) + list(VARIANTS)


def bounds_name(name):
    """the scene whose F32_ORACLE_ERROR / FAMILY entry a case's kernel bounds come from"""
    return VARIANTS[name][0] if name in VARIANTS and VARIANTS[name][1] == "far" else name


def make_scene(name, tmp_path) -> Scene:
    base, mesh = VARIANTS.get(name, (name, None))
    sc = SCENES[base](base)
    sc.name, sc.base, sc.mesh = name, base, mesh
    if mesh is not None:  # plain_step has no unrolled <7, 0, true, 1>: a 7-joint model with a mesh runs the generic instance
        sc.instance = (0 if sc.instance[0] == 7 else sc.instance[0], sc.instance[1], True)
    if sc.urdf is not None:
        p = os.path.join(str(tmp_path), f"{name}.urdf")
        with open(p, "w") as f:
            f.write(sc.urdf)
        sc.robot = parse_urdf(p)
        if base == "branch_arm_two_cubes":
            assert active_joint_names(sc.robot) == ["j1", "k1", "j2", "k2", "j3"]
    # the state the solvers get is float32: the reference starts from exactly that
    for k in ("q", "q_target", "pos", "force", "spin"):
        setattr(sc, k, getattr(sc, k).astype(np.float32).astype(np.float64))
    return sc


def scaled(sc: Scene, factor) -> Scene:
    """the scene with its swept parameter moved by `factor` (for q_target: the distance of the target from the state, of the
    joints in `swept_dofs` where the scene names them)"""
    out = copy.copy(sc)
    if sc.swept == "q_target":
        out.q_target = sc.q + factor * (sc.q_target - sc.q)
        if sc.swept_dofs is not None:
            keep = [k for k in range(sc.q.shape[1]) if k not in sc.swept_dofs]
            out.q_target[:, keep] = sc.q_target[:, keep]
    else:
        setattr(out, sc.swept, getattr(sc, sc.swept) * factor)
    return out


# ---- the model the solvers run ------------------------------------------------------------------------------------------
def _root_T(p):
    T = np.eye(4)
    T[:3, 3] = p
    return T


def compile_scene(sc: Scene, sweeps=None):
    sweeps = sc.sweeps if sweeps is None else sweeps
    rb = sc.robot
    rec = ArticulationRecord("robot", rb, initial_pose=geom.pose(list(sc.root_p)), link_shapes=dict((k, [v]) for k, v in sc.pads.items()),
                             link_gravity={n: False for n in rb.links}, drives=dict(sc.drives), build_mimic_joints=sc.mimic)
    b = SceneModelBuilder()
    b.set_articulation(rec)
    if sc.ground_mu is not None and sc.mesh != "ground":
        g = ground_record(0.0)
        g.shapes[0].static_friction = g.shapes[0].dynamic_friction = sc.ground_mu
        b.add_actor(g)
    if sc.mesh == "ground":  # one triangle at z = 0, normal +z, every cube's footprint more than 0.1 m inside its edges (asserted)
        V = np.array(MESH_GROUND, dtype=np.float64)
        for i in range(len(sc.frees)):
            for sx in (-1, 1):
                for sy in (-1, 1):
                    c = sc.pos[:, i, :2] + np.array([sx * sc.frees[i].half[0], sy * sc.frees[i].half[1]])
                    assert (c[:, 0] - V[0, 0]).min() > 0.1 and (c[:, 1] - V[0, 1]).min() > 0.1 and ((V[1, 0] + V[0, 1] - c.sum(1)) / np.sqrt(2)).min() > 0.1
        tri = ShapeRecord("trimesh", geom.pose(), vertices=V, triangles=np.array([[0, 1, 2]]), static_friction=sc.ground_mu, dynamic_friction=sc.ground_mu)
        b.add_actor(ActorRecord("ground", "static", [tri]))
    elif sc.mesh == "far":
        V = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0]], dtype=np.float64)
        b.add_actor(ActorRecord("far_mesh", "static", [ShapeRecord("trimesh", geom.pose(), vertices=V, triangles=np.array([[0, 1, 2]]))], initial_pose=geom.pose([6.0, 6.0, 6.0])))
    for i, fb in enumerate(sc.frees):
        b.add_actor(ActorRecord(fb.name, "dynamic", [_box(fb.half, mu=fb.mu, patch_radius=fb.patch_radius)], initial_pose=geom.pose(list(sc.pos[0, i])), disable_gravity=not fb.gravity))
    model = b.compile(position_iterations=sweeps, sleep_threshold=0.0)
    # the instance mssim_dispatch::plain_step picks, as rows_per_env (mssim_model_pack.h) computes it
    comps = model.n_dof + 6 * model.n_free
    nr = 1 if comps <= 16 else (2 if model.n_free <= 2 else 4)
    tri = bool((model.arrays["shape_type"] == SHAPE_TRIMESH).any())
    ndof = 0 if nr == 4 else (model.n_dof if model.n_dof in (9, 15) or (model.n_dof == 7 and nr == 1 and not tri) else 0)
    assert tri == (sc.mesh is not None) and (ndof, nr, tri) == sc.instance, (sc.name, ndof, nr, tri)
    return model


def run_solver(px, sc: Scene, model):
    """one substep of `px` from the scene's state -> dict(qd [N, n], v [N, nf, 6], by_pair: per env {(row a, row b): impulse},
    counts: per env {(row a, row b): points}, q [N, n] after the substep)"""
    import torch

    dev = px.device
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev)
    px.cuda_articulation_qpos.torch()[:] = t(sc.q)
    px.cuda_articulation_qvel.torch()[:] = 0.0
    px.cuda_articulation_target_qpos.torch()[:] = t(sc.q_target)
    rb = px.cuda_rigid_body_data.torch().reshape(model.n_rows, N, 13)
    force = px.cuda_rigid_body_force.torch().reshape(model.n_rows, N, 4)
    for i, fb in enumerate(sc.frees):
        r = model.row_of(fb.name)
        rb[r, :, :3] = t(sc.pos[:, i])
        rb[r, :, 3:7] = t([1.0, 0, 0, 0])
        rb[r, :, 7:10] = 0.0
        rb[r, :, 10:13] = t(sc.spin[:, i])
        force[r, :, :3] = t(sc.force[:, i])
    px.gpu_apply_all()
    px.gpu_apply_rigid_dynamic_force()
    px.step(1)
    px.gpu_fetch_all()
    rb = px.cuda_rigid_body_data.torch().reshape(model.n_rows, N, 13).cpu().double().numpy()
    v = np.stack([rb[model.row_of(fb.name), :, 7:13] for fb in sc.frees], axis=1) if sc.frees else np.zeros((N, 0, 6))
    if model.n_pair > 0:
        imp = px.read_internal("pair_impulse", 3 * model.n_pair).cpu().double().numpy().reshape(model.n_pair, 3, N)
        cnt = px.read_internal("contact_count", model.n_pair).cpu().numpy()
    rows, ps = model.arrays["shape_row"], model.arrays["pair_shape"]
    by_pair, counts = [dict() for _ in range(N)], [dict() for _ in range(N)]
    for e in range(N):
        for p in range(model.n_pair):
            if cnt[p, e] > 0:
                key = (int(rows[ps[p, 0]]), int(rows[ps[p, 1]]))
                by_pair[e][key] = by_pair[e].get(key, 0) + imp[p, :, e]
                counts[e][key] = counts[e].get(key, 0) + int(cnt[p, e])
    return dict(qd=px.cuda_articulation_qvel.torch().cpu().double().numpy().copy(), q=px.cuda_articulation_qpos.torch().cpu().double().numpy().copy(),
                v=v, by_pair=by_pair, counts=counts)


# ---- the reference ----------------------------------------------------------------------------------------------------
def _face_contacts(ca, ha, cb, hb, axis):
    """two axis-aligned boxes (centre, half sizes) touching on faces normal to `axis`, a on the + or - side of b: the corners of the
    overlap rectangle on the mid-plane of the two faces -> (points, unit normal from b towards a, gap)"""
    s = 1.0 if ca[axis] > cb[axis] else -1.0
    fa, fb = ca[axis] - s * ha[axis], cb[axis] + s * hb[axis]
    gap = s * (fa - fb)
    o = [k for k in range(3) if k != axis]
    lo = [max(ca[k] - ha[k], cb[k] - hb[k]) for k in o]
    hi = [min(ca[k] + ha[k], cb[k] + hb[k]) for k in o]
    assert all(h_ - l_ > 1e-3 for l_, h_ in zip(lo, hi)), "the faces do not overlap"
    pts = []
    for u in (lo[0], hi[0]):
        for w in (lo[1], hi[1]):
            p = np.zeros(3)
            p[axis], p[o[0]], p[o[1]] = 0.5 * (fa + fb), u, w
            pts.append(p)
    n = np.zeros(3)
    n[axis] = s
    return pts, n, gap


def with_shape_inertials(sc: Scene):
    """the robot the reference's dynamics see: the scene's, with every link of `shape_inertial` (no <inertial> in the URDF) given
    the inertial of its pad, a solid box of 1000 kg/m^3, in closed form: m = 8000 hx hy hz at the pad's centre, I = m / 3 diag(hy^2 +
    hz^2, ...) turned into the link frame"""
    if not sc.shape_inertial:
        return sc.robot
    rb = copy.copy(sc.robot)
    rb.links = dict(rb.links)
    for l in sc.shape_inertial:
        assert not rb.links[l].has_inertial, l
        s = sc.pads[l]
        hx, hy, hz = (float(x) for x in s.half_size)
        m = 1000.0 * 8 * hx * hy * hz
        R = geom.quat_to_mat(s.pose[3:])
        I = R @ np.diag([m / 3 * (hy * hy + hz * hz), m / 3 * (hx * hx + hz * hz), m / 3 * (hx * hx + hy * hy)]) @ R.T
        rb.links[l] = replace(rb.links[l], mass=m, com=np.array(s.pose[:3], dtype=np.float64), inertia=I, has_inertial=True)
    return rb


def problem(sc: Scene, env):
    """what env `env` hands the direct solver: -> dict(A, rhs, saturated, implicit = dt kd + dt^2 kp per joint, tendons, jac(link, x),
    bodies, contacts, limits, torsion, points {(a, b): count}, normal {(a, b): unit normal}) with sides as in `sc.pairs`"""
    rb = with_shape_inertials(sc)
    names = active_joint_names(rb)
    n = len(names)
    q, qt = sc.q[env], sc.q_target[env]
    root_T = _root_T(sc.root_p)
    off = {l: False for l in rb.links}
    M, c = mass_matrix_and_bias(rb, q, np.zeros(n), link_gravity=off, root_T=root_T)
    kp = np.array([sc.drives[j][0] for j in names])
    kd = np.array([sc.drives[j][1] for j in names])
    fmax = np.array([sc.drives[j][2] for j in names])
    tendons = []
    if sc.mimic:
        for j in rb.joints:
            if j.mimic is not None and j.type != "fixed":  # q_j = multiplier q_src + offset, stiffness 1e5, no damping
                cc = np.zeros(n)
                cc[names.index(j.name)], cc[names.index(j.mimic[0])] = 1.0, -j.mimic[1]
                tendons.append((cc, j.mimic[2], 1e5, 0.0))
    A, rhs, sat = indep_lcp.joint_space_system(M, c, q, np.zeros(n), DT, kp, kd, fmax, qt, tendons=tendons)
    T = urdf_link_poses(rb, q, root_T)
    boxes = {}
    for link, s in sc.pads.items():
        X = T[link] @ _T44(s.pose)
        assert np.abs(X[:3, :3] - np.eye(3)).max() < 1e-6 or np.abs(np.abs(X[:3, :3]).round() - np.abs(X[:3, :3])).max() < 1e-6, (link, X)
        boxes[link] = (X[:3, 3], np.abs(X[:3, :3]).round() @ np.asarray(s.half_size, dtype=np.float32).astype(np.float64))
    bodies = []
    for i, fb in enumerate(sc.frees):
        half = np.asarray(fb.half, dtype=np.float32).astype(np.float64)
        m = 1000.0 * 8 * half.prod()
        I = np.diag([m / 3 * (half[1] ** 2 + half[2] ** 2), m / 3 * (half[0] ** 2 + half[2] ** 2), m / 3 * (half[0] ** 2 + half[1] ** 2)])
        bodies.append(dict(m=m, I=I, x=sc.pos[env, i], v=np.zeros(3), w=sc.spin[env, i], f=sc.force[env, i], gravity=fb.gravity))
        boxes[i] = (sc.pos[env, i], half)
    mu_of = lambda s: sc.ground_mu if s == -1 else (sc.pads[s].static_friction if isinstance(s, str) else sc.frees[s].mu)
    contacts, torsion, points, normals = [], [], {}, {}
    for a, b, axis in sc.pairs:
        if b == -1:
            ca, ha = boxes[a]
            pts = [np.array([ca[0] + sx * ha[0], ca[1] + sy * ha[1], 0.0]) for sx in (-1, 1) for sy in (-1, 1)]
            nrm, gap = np.array([0, 0, 1.0]), ca[2] - ha[2]
        else:
            pts, nrm, gap = _face_contacts(*boxes[a], *boxes[b], axis)
        assert abs(gap) < 1e-7, (sc.name, a, b, gap)  # gap 0 up to the float32 rounding of the state
        mu = 0.5 * (mu_of(a) + mu_of(b))
        first = len(contacts)
        contacts += [(a, b, p, nrm, 0.0, mu) for p in pts]
        points[(a, b)] = len(pts)
        normals[(a, b)] = nrm
        r = max(sc.pads[s].patch_radius if isinstance(s, str) else (sc.frees[s].patch_radius if s >= 0 else 0.0) for s in (a, b))
        if r > 0:
            members = list(range(first, len(contacts)))
            torsion.append((a, b, nrm, mu * r, members))
    limits = []
    for k, jn in enumerate(names):
        lo, hi = rb.parent_joint[next(l for l in rb.link_order if l in rb.parent_joint and rb.parent_joint[l].name == jn)].limit
        lo, hi = float(np.float32(lo)), float(np.float32(hi))
        if np.isfinite(lo) or np.isfinite(hi):
            dlo, dhi = q[k] - lo, hi - q[k]
            assert min(dlo, dhi) >= 0
            limits.append((k, 1.0, dlo) if dlo <= dhi else (k, -1.0, dhi))

    def jac(link, x):
        return link_point_jacobian(rb, q, link, x, root_T)

    return dict(A=A, rhs=rhs, saturated=sat, implicit=DT * kd + DT * DT * kp, tendons=tendons, jac=jac, bodies=bodies, contacts=contacts,
                limits=limits, torsion=torsion, points=points, normal=normals)


def solve(pb, covering=None):
    """the direct solution of a problem: -> dict(qd [n], v [nf, 6], by_pair {(a, b): impulse on a}, points, normal, info of the LCP,
    saturated [n], contacts)"""
    n = len(pb["rhs"])
    u, imp, info = indep_lcp.solve_substep_generalized(pb["A"], pb["rhs"], pb["jac"], pb["bodies"], pb["contacts"], DT, limits=pb["limits"],
                                                       torsion=pb["torsion"], covering=covering)
    by_pair = {}
    for (a, b, *_), i in zip(pb["contacts"], imp):
        by_pair[(a, b)] = by_pair.get((a, b), 0) + i
    sliding = {}  # per pair and friction axis: every pushing point moves along it, so its friction is at the bound mu lambda_n
    for key in by_pair:
        idx = [k for k, c in enumerate(pb["contacts"]) if (c[0], c[1]) == key and info["lam"][k] > 1e-9]
        sliding[key] = tuple(bool(idx) and all(info["sigma"][2 * k + t] > 1e-7 for k in idx) for t in (0, 1))
    return dict(qd=u[:n], v=u[n:].reshape(len(pb["bodies"]), 6), by_pair=by_pair, points=pb["points"], normal=pb["normal"], sliding=sliding,
                info=info, saturated=pb["saturated"], contacts=pb["contacts"])


def reference(sc: Scene, env, covering=None):
    return solve(problem(sc, env), covering)


def _T44(pose7):
    T = np.eye(4)
    T[:3, :3] = geom.quat_to_mat(pose7[3:])
    T[:3, 3] = pose7[:3]
    return T


def compared_parts(sc: Scene, env, ref, key):
    """the directions along which the impulse of pair `key` is unique and compared: its normal; a friction axis if the pair slides
    along it (the impulse there is mu sum(lambda_n)) or if the scene says the whole impulse is unique in this env"""
    nrm = ref["normal"][key]
    return [nrm] + [t for t, slides in zip(indep_lcp.tangents(nrm), ref["sliding"][key]) if slides or sc.tangent_unique[env]]


def row_of_side(sc: Scene, model, side):
    return -1 if side == -1 else (model.row_of(side) if isinstance(side, str) else model.row_of(sc.frees[side].name))


def errors(sc: Scene, model, got, refs):
    """largest velocity error (joints, linear, angular alike) and impulse error over the envs; contact counts must equal the
    reference's point count per pair -> (err_v, err_i). Impulses: per pair the parts that are unique (compared_parts), and always
    the net impulse on every free body."""
    ev = ei = 0.0
    for e, ref in enumerate(refs):
        ev = max(ev, np.abs(got["qd"][e] - ref["qd"]).max(), np.abs(got["v"][e] - ref["v"]).max() if sc.frees else 0.0)
        want = {(row_of_side(sc, model, a), row_of_side(sc, model, b)): (w, ref["points"][(a, b)], compared_parts(sc, e, ref, (a, b))) for (a, b), w in ref["by_pair"].items()}
        assert len(got["by_pair"][e]) == len(want), (sc.name, e, got["counts"][e], want)
        net_got, net_want = {}, {}
        for (ra, rb_), (w, npts, parts) in want.items():
            # (the solver keys a pair by its shapes' order: the impulse on the first body; the other order is its negative)
            fwd = (ra, rb_) in got["by_pair"][e]
            key = (ra, rb_) if fwd else (rb_, ra)
            assert got["counts"][e][key] == npts, (sc.name, e, key, got["counts"][e], npts)
            g = got["by_pair"][e][key] if fwd else -got["by_pair"][e][key]
            ei = max(ei, max(abs((g - w) @ d) for d in parts))
            for row, sgn in ((ra, 1.0), (rb_, -1.0)):
                net_got[row] = net_got.get(row, 0) + sgn * g
                net_want[row] = net_want.get(row, 0) + sgn * w
        for fb in sc.frees:
            row = model.row_of(fb.name)
            ei = max(ei, np.abs(net_got[row] - net_want[row]).max())
    return float(ev), float(ei)
