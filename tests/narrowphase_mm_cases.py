"""Millimetre-scale rows for the narrowphase tests: a peg of PlugCharger's charger (a box of half size 8 x 0.75 x 3.2 mm)
against the walls of one slot of the receptacle, which leaves it 0.5 mm per side, under the usual contact offset of 20 mm --
forty times the clearance, so every wall of the slot is in contact range of the peg at once. One batch of class 'boxbox_mm'
for the machinery of tests/narrowphase_cases.py: the float64 reference (tests/narrowphase_reference.py), the oracles' hook
and `mssim_test_collide`, with the box-box bounds MEASURED_BOXBOX of that file (the float32 oracle's error on the metre-scale
table, times 4; nothing here is measured against the HIP kernels).

The receptacle stands at the origin, unrotated, as tests/test_plug_charger.py pins its boxes: every box spans x in
[-20, 0] mm (the mouth is the face x = 0), the +y slot is bounded by the outer block (y >= 8.25 mm), the filler
(y <= 5.75 mm) and the two plates (|z| >= 3.7 mm). The peg sits in it as at the goal pose: turned by pi about z, centred at
(-8, 7, 0) mm.

Cases: the centred peg against each of the four walls (0.5 mm gap, as shape A and as shape B); the peg moved until it touches
a wall (0 gap) and 0.2 mm into it; the peg pitched and yawed by 0.1 rad inside the slot, as a sagging charger holds it (its
ends then lie inside the plates or the side walls); and the peg edge-on at the slot's mouth: rolled and pitched so that one of
its long edges crosses the mouth edge of a plate or of the outer block at right angles, 0.3 mm away and 0.1 mm inside (the
separating axis is the cross product of the two edges: a one-point manifold)."""
import functools

import numpy as np

from tests import narrowphase_cases as nc
from tests.narrowphase_reference import BOX

PEG = [8e-3, 0.75e-3, 3.2e-3]
CLEAR = 5e-4
SLOT = [PEG[0], PEG[1] + CLEAR, PEG[2] + CLEAR]  # the slot's half size
REC = [1e-2, 5e-2, 5e-2]
GAP = 7e-3
Q_PI_Z = (0.0, 0.0, 0.0, 1.0)
PEG_P = np.array([-PEG[0], GAP, 0.0])


def walls():
    """name -> (centre, half size) of the four boxes around the +y slot, by the task's formulas (plug_charger.py
    `receptacle_boxes`, written out again here: the env is not imported)"""
    sy, sz = 0.5 * (REC[1] - SLOT[1] - GAP), 0.5 * (REC[2] - SLOT[2])
    dx, dy, dz = -REC[0], SLOT[1] + GAP + sy, SLOT[2] + sz
    return {
        "top plate": ([dx, 0, dz], [REC[0], REC[1], sz]),
        "bottom plate": ([dx, 0, -dz], [REC[0], REC[1], sz]),
        "outer block": ([dx, dy, 0], [REC[0], sy, REC[2]]),
        "filler": ([dx, 0, 0], [REC[0], GAP - SLOT[1], SLOT[2]]),
    }


# the direction from the slot's middle toward each wall
TOWARD = {"top plate": np.array([0, 0, 1.0]), "bottom plate": np.array([0, 0, -1.0]), "outer block": np.array([0, 1.0, 0]), "filler": np.array([0, -1.0, 0])}


def ref_quat(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw])


def _axis_q(axis, angle):
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * np.asarray(axis, np.float64)])


@functools.lru_cache(maxsize=None)
def mm_batch():
    b = nc.Batch("boxbox_mm")
    W = walls()
    for name, (c, h) in W.items():
        # centred: 0.5 mm from every wall; in either order of the pair
        b.add(f"centred, {name}", BOX, nc._pose(PEG_P, Q_PI_Z), PEG, BOX, nc._pose(c), h, tags=("clear",))
        b.add(f"centred, {name} as A", BOX, nc._pose(c), h, BOX, nc._pose(PEG_P, Q_PI_Z), PEG, tags=("clear",))
        # moved toward the wall: touching, and 0.2 mm inside (0.25 mm off centre along x as well, so that nothing is symmetric)
        for what, move in (("0 gap", CLEAR), ("0.2 mm penetration", CLEAR + 2e-4)):
            p = PEG_P + TOWARD[name] * move + [2.5e-4, 0, 0]
            b.add(f"{what}, {name}", BOX, nc._pose(p, Q_PI_Z), PEG, BOX, nc._pose(c), h, tags=(what,))
    # tilted by 0.1 rad inside the slot: pitched (about y) against the plates, yawed (about z) against the side walls
    for k, s in enumerate((1.0, -1.0)):
        for name in ("top plate", "bottom plate"):
            b.add(f"pitched {k}, {name}", BOX, nc._pose(PEG_P, ref_quat(_axis_q([0, 1, 0], 0.1 * s), Q_PI_Z)), PEG, BOX, nc._pose(W[name][0]), W[name][1], tags=("tilted",))
        for name in ("outer block", "filler"):
            b.add(f"yawed {k}, {name}", BOX, nc._pose(PEG_P, ref_quat(_axis_q([0, 0, 1], 0.1 * s), Q_PI_Z)), PEG, BOX, nc._pose(W[name][0]), W[name][1], tags=("tilted",))
    # pitched AND yawed, with a little roll: no axis of the peg stays aligned with the slot
    q = ref_quat(_axis_q([0, 1, 0], 0.1), ref_quat(_axis_q([0, 0, 1], -0.1), ref_quat(_axis_q([1, 0, 0], 0.03), Q_PI_Z)))
    for name, (c, h) in W.items():
        b.add(f"pitched, yawed and rolled, {name}", BOX, nc._pose(PEG_P, q), PEG, BOX, nc._pose(c), h, tags=("tilted",))
    # edge-on at the mouth. The wall's mouth edge runs along e_w through the point m; its two faces have outward normals n_1
    # (into the slot) and n_2 = +x (the mouth). The peg's long edge must run along cross(e_w, bis), bis = (n_1 + n_2) / sqrt 2,
    # with the peg's body on the far side of it: the peg is rolled so that one long edge looks along -bis and placed so that
    # this edge passes the mouth edge at the distance g along bis, crossing it 1 mm from the slot's middle.
    r = float(np.hypot(PEG[1], PEG[2]))  # from the peg's axis to a long edge
    for name, n1, m, e_w in (("bottom plate", np.array([0, 0, 1.0]), np.array([0, GAP + 1e-3, -SLOT[2]]), np.array([0, 1.0, 0])),
                            ("top plate", np.array([0, 0, -1.0]), np.array([0, GAP - 1e-3, SLOT[2]]), np.array([0, 1.0, 0])),
                            ("outer block", np.array([0, -1.0, 0]), np.array([0, GAP + SLOT[1], 1e-3]), np.array([0, 0, 1.0]))):
        bis = (n1 + np.array([1.0, 0, 0])) / np.sqrt(2)
        x_axis = np.cross(e_w, bis)          # the peg's long axis
        x_axis /= np.linalg.norm(x_axis)
        # the peg's frame: x along x_axis; the corner (0, -hy, -hz) / r of its cross section along -bis
        down = np.array([0.0, -PEG[1], -PEG[2]]) / r
        Rm = np.stack([x_axis, -bis, np.cross(x_axis, -bis)], 1) @ np.stack([[1.0, 0, 0], down, np.cross([1.0, 0, 0], down)], 1).T
        qm = _mat_q(Rm)
        for what, g in (("0.3 mm off", 3e-4), ("0.1 mm in", -1e-4)):
            centre = m + bis * (g + r)
            b.add(f"edge-on at the mouth, {name}, {what}", BOX, nc._pose(centre, qm), PEG, BOX, nc._pose(W[name][0]), W[name][1], tags=("edge",))
    return b.finish()


def _mat_q(R):
    """quaternion (wxyz) of a rotation matrix (the trace branch is enough: none of the rotations here is near a half turn)"""
    w = 0.5 * np.sqrt(max(1.0 + R[0, 0] + R[1, 1] + R[2, 2], 0.0))
    assert w > 0.2
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
