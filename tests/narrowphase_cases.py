"""Case tables for the narrowphase tests (tests/test_narrowphase.py on the CPU, tests/test_gpu_narrowphase.py on the GPU):
seeded generators and hand-written edge cases, one batch per class, in exactly the float32 numbers that every
implementation is given. Checked against tests/narrowphase_reference.py.

Classes:  'boxbox' (SAT + clipping), 'plane' (plane against every primitive), 'plane_hull', 'mpr' (single-point manifolds
of sphere, capsule, cylinder, hull and box against each other; box-box forced through the MPR is its own batch
'mpr_boxbox': only the forced path can run it).

A case carries tags: 'dyadic' (every number a small dyadic rational and every frame axis-aligned: float32 and float64
arithmetic are both exact, results must be bitwise those of the f64 oracle), 'far' (10 m from the origin: constants of
its own), 'tie' (a hull support tie on exact numbers: the contact point must be the f64 oracle's).

MEASURED_*: the largest error of the FLOAT32 ORACLE against the reference (for n and x of the exact classes: against the
f64 oracle) per class and quantity, times 4 -- the margin for the HIP build's approximate reciprocal and square root and
for FMA contraction that differs from the host's. Never measured against the HIP kernels. Produced by
    python -m tests.narrowphase_cases
which prints the raw maxima and the constants below.
"""
import ctypes as C
import functools

import numpy as np

from maniskill_amd.model import geom
from tests import narrowphase_reference as ref
from tests.narrowphase_reference import BOX, CAPSULE, CONVEX, CYLINDER, PLANE, SPHERE, Shape

OFFSET = 0.02  # the contact offset of every batch (mani_skill/utils/structs/types.py:40)
MARGIN = 4.0   # MEASURED = MARGIN x the float32 oracle's largest error

# ---- measured (see the module docstring); {quantity: bound}, lengths in metres
MEASURED_BOXBOX = dict(unit=2.13e-06, axis=5.62e-06, deficit=1.31e-07, depth=1.66e-06, surface=3.75e-07, outside=9.57e-07, n_vs_f64=3.93e-06, x_vs_f64=1.79e-06, sep_vs_f64=1.66e-06)
# (10 m from the origin. The zeros: the normal of these cases is an axis of an axis-aligned box, exact in any arithmetic)
MEASURED_BOXBOX_FAR = dict(unit=0.00e+00, axis=0.00e+00, deficit=0.00e+00, depth=4.10e-06, surface=6.07e-06, outside=3.93e-06, n_vs_f64=0.00e+00, x_vs_f64=3.81e-06, sep_vs_f64=4.10e-06)
MEASURED_PLANE = dict(n=2.25e-06, x=1.70e-06, sep=6.31e-07, n_vs_f64=2.15e-06, x_vs_f64=1.73e-06, sep_vs_f64=6.31e-07)
MEASURED_PLANE_HULL = dict(n=1.93e-06, x=3.49e-07, sep=6.89e-07, n_vs_f64=1.91e-06, x_vs_f64=4.77e-07, sep_vs_f64=6.85e-07)
# (sep, mid, g_deficit: the MPR stops MSSIM_MPR_TOLERANCE = 1e-5 short of the surface and takes its depth from the last portal,
# whose normal on a flat or sharp feature is ill-conditioned: the float32 oracle is this far from g(n). exact, sep_vs_f64: sharp)
MEASURED_MPR = dict(unit=4.91e-07, sep=8.15e-04, mid=2.71e-04, g_deficit=5.25e-04, exact=2.66e-05, sep_vs_f64=1.77e-05, tie_x=1.51e-08)
MEASURED_MPR_BOXBOX = dict(unit=4.66e-07, sep=3.97e-05, mid=1.65e-05, g_deficit=2.97e-05, exact=0.00e+00, sep_vs_f64=1.82e-05, tie_x=0.00e+00)
# the f64 oracle's own distance from the reference where the reference is exact (the reference's own error: it pins both)
F64_TOL = 1e-9

MPR_PERTURB = 2e-6       # the stability filter of the MPR classes (mpr_filter): a case is left out only if the F64 ORACLE ALONE
MPR_PERTURB_SEP = 5e-6   # flips its count or moves sep by more than this under four translations of shape A by MPR_PERTURB
MPR_FILTER_CAP = 0.03    # at most this share of a class may be left out


def _q(rpy):
    r, p, y = (0.5 * float(v) for v in rpy)
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy])


def _rand_q(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _pose(p, q=(1, 0, 0, 0)):
    return np.concatenate([np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)])


class Batch:
    """arrays of a batch of n pairs: type [n][2] int32, pose [n][2][7], param [n][2][4] float32, hulls [n][2] (float32 [k][3] or
    None), tags [n] (sets of str), names [n]"""

    def __init__(self, name):
        self.name, self.offset = name, OFFSET
        self._rows = []

    def add(self, name, ta, pa, prm_a, tb, pb, prm_b, va=None, vb=None, tags=()):
        f = lambda v, k: np.asarray(list(v) + [0.0] * (k - len(v)), dtype=np.float32)
        h = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
        self._rows.append((name, int(ta), f(pa, 7), f(prm_a, 4), int(tb), f(pb, 7), f(prm_b, 4), h(va), h(vb), frozenset(tags)))

    def finish(self):
        r = self._rows
        self.n = len(r)
        self.names = [x[0] for x in r]
        self.type = np.array([[x[1], x[4]] for x in r], dtype=np.int32)
        self.pose = np.array([[x[2], x[5]] for x in r], dtype=np.float32)
        self.param = np.array([[x[3], x[6]] for x in r], dtype=np.float32)
        self.hulls = [(x[7], x[8]) for x in r]
        self.tags = [x[9] for x in r]
        return self

    def shapes(self, i):
        return (Shape(self.type[i, 0], self.pose[i, 0], self.param[i, 0], self.hulls[i][0]),
                Shape(self.type[i, 1], self.pose[i, 1], self.param[i, 1], self.hulls[i][1]))

    def tagged(self, tag):
        return np.array([tag in t for t in self.tags])

    def moved(self, dp):
        """the same batch with shape A translated by dp ([3] or [n][3]; the perturbations of the MPR filter)"""
        b = Batch(self.name)
        b.n, b.names, b.type, b.param, b.hulls, b.tags = self.n, self.names, self.type, self.param, self.hulls, self.tags
        b.pose = self.pose.copy()
        b.pose[:, 0, :3] = (self.pose[:, 0, :3].astype(np.float64) + dp).astype(np.float32)
        return b

    def packed_hulls(self):
        """(hull [n][2][2] int32: first vertex, count; verts [m][3] float32) laid out as the model packer lays hulls out: every
        hull starts on a multiple of 8 vertices and is padded to a multiple of 8 with copies of its vertex 0"""
        hull = np.zeros((self.n, 2, 2), dtype=np.int32)
        chunks, seen, used = [], {}, 0
        for i, pair in enumerate(self.hulls):
            for k, v in enumerate(pair):
                if v is None:
                    continue
                if id(v) not in seen:
                    pad = (-len(v)) % 8
                    chunks.append(np.concatenate([v, np.repeat(v[:1], pad, axis=0)]))
                    seen[id(v)] = used
                    used += len(v) + pad
                hull[i, k] = (seen[id(v)], len(v))
        verts = np.concatenate(chunks) if chunks else np.zeros((8, 3), dtype=np.float32)
        return hull, np.ascontiguousarray(verts, dtype=np.float32)


# ------------------------------------------------------------------------------------------ the oracle's hook
def oracle_collide(lib, batch, force_mpr=False):
    """[n][20] float32 of the oracle's mssim_ref_test_collide: count | n | 4 x (x y z sep)"""
    fn = lib.lib.mssim_ref_test_collide
    fn.restype = C.c_int
    F = C.POINTER(C.c_float)
    out = np.zeros((batch.n, 20), dtype=np.float32)
    none = np.zeros(3, dtype=np.float32)
    for i in range(batch.n):
        va, vb = batch.hulls[i]
        fn(C.c_int(int(batch.type[i, 0])), batch.pose[i, 0].ctypes.data_as(F), batch.param[i, 0].ctypes.data_as(F),
           (none if va is None else va).ctypes.data_as(F), C.c_int(0 if va is None else len(va)),
           C.c_int(int(batch.type[i, 1])), batch.pose[i, 1].ctypes.data_as(F), batch.param[i, 1].ctypes.data_as(F),
           (none if vb is None else vb).ctypes.data_as(F), C.c_int(0 if vb is None else len(vb)),
           C.c_float(batch.offset), C.c_int(1 if force_mpr else 0), out[i].ctypes.data_as(F))
    return out


def split(out):
    """(count [n] int, normal [n][3], points [n][4][4]) as float64"""
    out = np.asarray(out, dtype=np.float64)
    return out[:, 0].astype(np.int64), out[:, 1:4], out[:, 4:20].reshape(-1, 4, 4)


# ------------------------------------------------------------------------------------------ box-box
TABLE = [1.0, 1.0, 0.5]   # half extents of the 2 x 2 x 1 m table, top face at z = 0
CUBE = [0.02, 0.02, 0.02]


def _lowest(R, h):
    return -float(np.abs(R[2, :]) @ np.asarray(h))


def _place(rng, A0, B0, target):
    """centre of A relative to B's, in a random direction d, at which the gap along d is `target` (both shapes given at the
    origin; the distance of the pair is at least that gap)"""
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    return d * (target + ref.support_value(A0, -d) + ref.support_value(B0, d))


def _boxbox_hand(b):
    d6 = 2.0 ** -6
    tb = _pose([0, 0, -0.25])
    # dyadic, axis-aligned: all four corners tie in depth, the faces of A and B tie as reference face
    for gi, g in enumerate((2.0 ** -10, -(2.0 ** -10), 0.0, 2.0 ** -7)):
        for xi, (x, y) in enumerate(((0.0, 0.0), (0.25, -0.125), (-0.375, 0.4375))):
            b.add(f"dyadic cube on table {gi}.{xi}", BOX, _pose([x, y, d6 + g]), [d6] * 3, BOX, tb, [0.5, 0.5, 0.25], tags=("dyadic",))
            b.add(f"dyadic table under cube {gi}.{xi}", BOX, tb, [0.5, 0.5, 0.25], BOX, _pose([x, y, d6 + g]), [d6] * 3, tags=("dyadic",))
        for xi, (x, y) in enumerate(((0.0, 0.0), (2.0 ** -8, 0.0), (2.0 ** -7, -(2.0 ** -8)), (-(2.0 ** -6), 2.0 ** -6))):
            b.add(f"dyadic cube on equal cube {gi}.{xi}", BOX, _pose([x, y, 2 * d6 + g]), [d6] * 3, BOX, _pose([0, 0, 0]), [d6] * 3, tags=("dyadic",))
            b.add(f"dyadic cube under equal cube {gi}.{xi}", BOX, _pose([0, 0, 0]), [d6] * 3, BOX, _pose([x, y, 2 * d6 + g]), [d6] * 3, tags=("dyadic",))
    tt = _pose([0, 0, -0.5])
    # equal cubes at yaw 45 degrees (and around it): the clipped octagon, 8 points cut to 4
    for k, yaw in enumerate((np.pi / 4, np.pi / 4 + 1e-3, np.pi / 4 - 0.02, 0.7, 3 * np.pi / 4)):
        # (never centred and flat at once: by symmetry two candidates of the 4-point reduction would span equal areas, and rounding
        # -- not the routine -- would choose between them)
        for j, (x, y, tilt) in enumerate(((0.002, 0.0005, 0), (0.001, -0.002, 0), (0, 0, 0.01), (0.003, 0.001, -0.02))):
            b.add(f"yaw45 {k}.{j}", BOX, _pose([x, y, 0.041], _q([tilt, 0.5 * tilt, yaw])), CUBE, BOX, _pose([0, 0, 0]), CUBE)
    # a cube overhanging a table edge and a table corner: overlap polygons of 3, 5 and 6 vertices
    for k, yaw in enumerate((0.0, 0.3, 0.8, 1.0, 1.3)):  # (not pi / 4 with the centre on the edge: two corners would lie ON a clip plane)
        for j, (x, y) in enumerate(((1.0, 0.2), (1.012, -0.3), (0.99, 0.5), (1.0, 1.0), (1.01, 0.995), (0.99, 1.012), (1.015, 1.015), (0.985, 0.99), (0.98, 0.98))):
            for t, tilt in enumerate((0.0, 0.004)):
                b.add(f"overhang {k}.{j}.{t}", BOX, _pose([x, y, 0.021], _q([tilt, -tilt, yaw])), CUBE, BOX, tt, TABLE)
    # crossed edges (closed form: edges at 90 degrees, 3 mm apart)
    h = 0.02 * np.sqrt(2)
    for k, g in enumerate((0.003, -0.002, 0.015)):
        b.add(f"crossed edges {k}", BOX, _pose([0, 0, 0], _q([np.pi / 4, 0, 0])), CUBE, BOX, _pose([0, 0, -2 * h - g], _q([0, np.pi / 4, 0])), CUBE, tags=("crossed",))
    # nearly parallel edges: cross-product axes of length ~1e-7 must be skipped
    for k, yaw in enumerate((1e-7, -2e-7, 5e-7)):
        b.add(f"nearly parallel {k}", BOX, _pose([0.004, -0.003, 0.041], _q([0, 0, yaw])), CUBE, BOX, _pose([0, 0, 0]), CUBE)
        b.add(f"nearly parallel tilted {k}", BOX, _pose([0.004, -0.003, 0.041], _q([yaw, 0, 0])), CUBE, BOX, _pose([0, 0, 0]), CUBE)
    # the gap just inside and just outside the contact offset
    for k, yaw in enumerate((0.0, 0.4)):
        b.add(f"inside offset {k}", BOX, _pose([0.1, 0.2, 0.02 + OFFSET - 1e-4], _q([0, 0, yaw])), CUBE, BOX, tt, TABLE)
        b.add(f"outside offset {k}", BOX, _pose([0.1, 0.2, 0.02 + OFFSET + 1e-4], _q([0, 0, yaw])), CUBE, BOX, tt, TABLE)
    # centres 1e-4 apart
    for k, (d, yaw) in enumerate((((0, 0, 1e-4), 0.0), ((6e-5, 0, 8e-5), 0.0), ((2e-5, -3e-5, 9e-5), 0.3), ((0, 0, -1e-4), 0.3))):
        b.add(f"centres 1e-4 apart {k}", BOX, _pose(d, _q([0, 0, yaw])), CUBE, BOX, _pose([0, 0, 0]), CUBE)
    # a 2 cm cube on the table 0.9 m off centre; the same pair 10 m from the origin
    for k, (yaw, tilt, g) in enumerate(((0.0, 0.0, 0.001), (0.4, 0.0, 0.001), (0.4, 0.01, -0.0005), (1.1, -0.02, 0.003))):
        R = Shape(BOX, _pose([0, 0, 0], _q([tilt, tilt, yaw])), [0.01] * 3).R
        z = g - _lowest(R, [0.01] * 3)
        b.add(f"small cube off centre {k}", BOX, _pose([0.9, -0.9, z], _q([tilt, tilt, yaw])), [0.01] * 3, BOX, tt, TABLE)
        far = np.array([10.0, -10.0, 10.0])
        b.add(f"small cube far {k}", BOX, _pose(far + [0.9, -0.9, z], _q([tilt, tilt, yaw])), [0.01] * 3, BOX, _pose(far + [0, 0, -0.5]), TABLE, tags=("far",))


def _boxbox_random(b, n_each):
    tt = _pose([0, 0, -0.5])
    rng = np.random.default_rng(20240611)
    for k in range(n_each):  # cube on table, tilt +/-0.05
        q = _q([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(-np.pi, np.pi)])
        R = Shape(BOX, _pose([0, 0, 0], q), CUBE).R
        g = rng.uniform(-0.004, 0.015)
        b.add(f"tilted cube {k}", BOX, _pose([rng.uniform(-0.9, 0.9), rng.uniform(-0.9, 0.9), g - _lowest(R, CUBE)], q), CUBE, BOX, tt, TABLE, tags=("random",))
    for k in range(n_each):  # boxes of any size in any orientation, the gap along the centre line drawn
        ha, hb = rng.uniform(0.01, 0.08, size=3), rng.uniform(0.01, 0.08, size=3)
        qa, qb, pb = _rand_q(rng), _rand_q(rng), rng.uniform(-0.5, 0.5, size=3)
        pa = pb + _place(rng, Shape(BOX, _pose([0, 0, 0], qa), ha), Shape(BOX, _pose([0, 0, 0], qb), hb), rng.uniform(-0.004, 0.006))
        b.add(f"any boxes {k}", BOX, _pose(pa, qa), ha, BOX, _pose(pb, qb), hb, tags=("random",))
    k = 0
    while k < n_each:  # flat stacks: a box on a box, yaw only
        ha, hb = rng.uniform(0.01, 0.05, size=3), rng.uniform(0.02, 0.1, size=3)
        x, y = rng.uniform(-1, 1, size=2) * (ha[:2] + hb[:2]) * 0.9
        g = rng.uniform(-0.004, 0.015)
        pa, pb = _pose([x, y, hb[2] + ha[2] + g], _q([0, 0, rng.uniform(-np.pi, np.pi)])), _pose([0, 0, 0], _q([0, 0, rng.uniform(-np.pi, np.pi)]))
        # All points of a flat contact are equally deep, so with more than 4 of them the reduction starts from whichever comes
        # first and, whenever its first edge is parallel to a side of the overlap polygon, meets two candidates of EQUAL area:
        # rounding decides, differently in float32 and float64. Point order can be pinned only where it is defined: flat
        # stacks keep the overlaps of up to 4 vertices; the reduction is exercised by the tilted families, where depth orders.
        A, B = Shape(BOX, pa, ha), Shape(BOX, pb, hb)
        if len(ref.overlap_polygon(B, 2, B.R[:, 2], A, 2, A.p - A.R[:, 2] * np.sign(A.R[2, 2]) * ha[2])) > 4:
            continue
        b.add(f"flat stack {k}", BOX, pa, ha, BOX, pb, hb, tags=("random",))
        k += 1


@functools.lru_cache(maxsize=None)
def boxbox_batch(n_each=800):
    b = Batch("boxbox")
    _boxbox_hand(b)
    _boxbox_random(b, n_each)
    return b.finish()


# ------------------------------------------------------------------------------------------ plane pairs
Q_X_TO_Y = (0.5, 0.5, 0.5, 0.5)       # x -> y, y -> z, z -> x: exact in float32 (a plane with normal +y, a shape with axis +y)
Q_GROUND = _q([0, -np.pi / 2, 0])     # the ground plane of the scenes: normal +z up to rounding
HULL_COUNTS = (4, 5, 8, 9, 16, 17, 40, 63, 64)


def _hull(rng, n, radius=0.04):
    """n points in convex position: on an ellipsoid"""
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * radius * rng.uniform(0.6, 1.0, size=3)).astype(np.float32)


def _cup(n=16, r=0.04, h=0.06):
    a = 2 * np.pi * np.arange(n) / n
    ring = np.stack([r * np.cos(a), r * np.sin(a), np.zeros(n)], axis=1)
    return np.concatenate([ring, ring * [1.2, 1.2, 0] + [0, 0, h]]).astype(np.float32)


def _rand_plane(rng):
    return _pose(rng.uniform(-0.5, 0.5, size=3), _rand_q(rng))


def _on_plane(rng, plane, B0, g):
    """centre of B at which its lowest point is `g` above the plane (B0: the shape at the origin)"""
    P = Shape(PLANE, plane, [0] * 4)
    npl = P.R[:, 0]
    side = np.cross(npl, rng.normal(size=3))
    return P.p + 0.3 * side + npl * (g + ref.support_value(B0, -npl))


def _prim(rng, t):
    if t == BOX:
        return list(rng.uniform(0.01, 0.06, size=3))
    if t == SPHERE:
        return [rng.uniform(0.01, 0.05)]
    return [rng.uniform(0.01, 0.03), rng.uniform(0.02, 0.06)]  # capsule, cylinder: radius, half length


@functools.lru_cache(maxsize=None)
def plane_batch(n_each=375):
    b = Batch("plane")
    rng = np.random.default_rng(20240612)
    py = _pose([0.1, -0.25, 0.3], Q_X_TO_Y)  # the plane y = -0.25
    # a capsule parallel to the plane: both ends tie exactly; a cylinder on its face: exactly no lowest rim point
    for k, g in enumerate((0.001, -0.002, OFFSET - 1e-4, OFFSET + 1e-4)):
        b.add(f"capsule parallel {k}", PLANE, py, [], CAPSULE, _pose([0.3, -0.25 + 0.02 + g, 0.1]), [0.02, 0.05])
        b.add(f"cylinder on its face {k}", PLANE, py, [], CYLINDER, _pose([0.3, -0.25 + 0.05 + g, 0.1], Q_X_TO_Y), [0.02, 0.05])
        b.add(f"box flat {k}", PLANE, py, [], BOX, _pose([0.3, -0.25 + 0.03 + g, 0.1]), [0.02, 0.03, 0.04])
        b.add(f"sphere {k}", PLANE, py, [], SPHERE, _pose([0.3, -0.25 + 0.03 + g, 0.1]), [0.03])
    for t in (BOX, SPHERE, CAPSULE, CYLINDER):
        for k in range(n_each):
            plane = _pose([0, 0, 0], Q_GROUND) if k % 3 == 0 else _rand_plane(rng)
            prm, q = _prim(rng, t), _rand_q(rng)
            if t == CYLINDER and k % 5 == 0:  # on its rim, nearly on its face
                Pn = Shape(PLANE, plane, [0] * 4)
                q = _tilted_axis_q(rng, Pn.R[:, 0], rng.uniform(0.002, 0.05))
            g = rng.choice([rng.uniform(-0.004, OFFSET - 1e-3), rng.uniform(OFFSET + 1e-3, 0.05)], p=[0.85, 0.15])
            pb = _on_plane(rng, plane, Shape(t, _pose([0, 0, 0], q), prm + [0] * (4 - len(prm))), g)
            b.add(f"plane {t} {k}", PLANE, plane, [], t, _pose(pb, q), prm)
    return b.finish()


def _tilted_axis_q(rng, axis, angle):
    """a frame whose x axis is `axis` tilted by `angle`"""
    t = np.cross(axis, rng.normal(size=3))
    t /= np.linalg.norm(t)
    x = np.cos(angle) * axis + np.sin(angle) * t
    y = np.cross(x, t)
    y /= np.linalg.norm(y)
    R = np.stack([x, y, np.cross(x, y)], axis=1)
    return np.asarray(geom.mat_to_quat(R), dtype=np.float64)


@functools.lru_cache(maxsize=None)
def plane_hull_batch(n_each=160):
    b = Batch("plane_hull")
    rng = np.random.default_rng(20240613)
    py = _pose([0.1, -0.25, 0.3], Q_X_TO_Y)
    cup = _cup()
    cube8 = (np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * 2.0 ** -6).astype(np.float32)
    # the cup rim flat on the plane (exact: all 16 rim vertices tie, the extent rule picks), and nearly flat
    for k, g in enumerate((0.0, 0.001, -0.002)):
        b.add(f"cup flat {k}", PLANE, py, [], CONVEX, _pose([0.3, -0.25 + g, 0.1], Q_X_TO_Y[:1] + (-0.5, -0.5, -0.5)), [], vb=cup)
        b.add(f"cube hull flat {k}", PLANE, py, [], CONVEX, _pose([0.3, -0.25 + 2.0 ** -6 + g, 0.1]), [], vb=cube8)
    for k in range(n_each):
        plane = _pose([0, 0, 0], Q_GROUND) if k % 3 == 0 else _rand_plane(rng)
        Pn = Shape(PLANE, plane, [0] * 4)
        # the cup's axis is its local z: a frame whose z is the plane normal, tilted a little
        qx = _tilted_axis_q(rng, Pn.R[:, 0], rng.uniform(0.0005, 0.01))
        q = geom.quat_mul(qx, np.array(Q_X_TO_Y))  # (z -> x first: the frame's z axis is where qx puts x)
        g = rng.uniform(-0.003, 0.012)
        pb = _on_plane(rng, plane, Shape(CONVEX, _pose([0, 0, 0], q), [0] * 4, cup), g)
        b.add(f"cup rim {k}", PLANE, plane, [], CONVEX, _pose(pb, q), [], vb=cup)
    for nv in HULL_COUNTS:
        for k in range(n_each // 2):
            v = _hull(rng, nv)
            plane = _pose([0, 0, 0], Q_GROUND) if k % 3 == 0 else _rand_plane(rng)
            q = _rand_q(rng)
            if k % 4 == 1:  # the deepest vertex is the last one
                Pn, S = Shape(PLANE, plane, [0] * 4), Shape(CONVEX, _pose([0, 0, 0], q), [0] * 4, v)
                low = int(np.argmin(S.world_verts() @ Pn.R[:, 0]))
                v = np.concatenate([np.delete(v, low, axis=0), v[low:low + 1]])
            g = rng.choice([rng.uniform(-0.004, OFFSET - 1e-3), rng.uniform(OFFSET + 1e-3, 0.05)], p=[0.9, 0.1])
            pb = _on_plane(rng, plane, Shape(CONVEX, _pose([0, 0, 0], q), [0] * 4, v), g)
            b.add(f"hull {nv} {k}" + (" deepest last" if k % 4 == 1 else ""), PLANE, plane, [], CONVEX, _pose(pb, q), [], vb=v)
    return b.finish()


# ------------------------------------------------------------------------------------------ single-point manifolds (MPR)
def _round_hull(rng, n):
    """n points on a sphere: the ray from the centre through a vertex lies in the normal cone of that vertex"""
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * rng.uniform(0.02, 0.05)).astype(np.float32)


def _mpr_shape(rng, t, nv=None):
    if t == CONVEX:
        return [], _round_hull(rng, nv or int(rng.choice(HULL_COUNTS)))
    return _prim(rng, t), None


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _aligned_dir(rng, t, verts):
    """a direction of the shape frame along which the ray from the centre meets the surface where that direction is a normal:
    a face of a box, a cap or the side of a capsule / cylinder, a vertex of a round hull, anywhere on a sphere"""
    if t == BOX:
        return np.eye(3)[rng.integers(3)] * rng.choice([-1.0, 1.0])
    if t in (CAPSULE, CYLINDER):
        if rng.random() < 0.4:
            return np.array([rng.choice([-1.0, 1.0]), 0.0, 0.0])
        a = rng.uniform(0, 2 * np.pi)
        return np.array([0.0, np.cos(a), np.sin(a)])
    if t == CONVEX:
        v = verts[rng.integers(len(verts))].astype(np.float64)
        return v / np.linalg.norm(v)
    return _unit(rng)


def _frame(rng, x):
    y = np.cross(x, _unit(rng))
    y /= np.linalg.norm(y)
    return np.stack([x, y, np.cross(x, y)], axis=1)


def _q_taking(rng, a, w, tilt):
    """a rotation taking the unit vector a to w (any spin about it), then tilted by the angle `tilt` about a random axis"""
    R = _frame(rng, w) @ _frame(rng, a).T
    k = _unit(rng)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(3) + np.sin(tilt) * K + (1 - np.cos(tilt)) * K @ K
    return np.asarray(geom.mat_to_quat(T @ R), dtype=np.float64)


def _mpr_targets(rng):
    """touching, separated inside the offset, penetrating, beyond the offset"""
    return rng.choice([rng.uniform(-1e-4, 1e-4), rng.uniform(0.002, OFFSET - 2e-3), rng.uniform(-0.004, -2e-4), rng.uniform(OFFSET + 5e-3, 0.06)], p=[0.2, 0.35, 0.35, 0.1])


def _mpr_add(b, rng, name, ta, tb, nva=None, nvb=None, tags=()):
    """A pair whose contact normal is (up to a tilt of at most 0.02 rad, none in half of the cases) the line of the two
    centres: the MPR's own assumption -- its depth is measured from the ray through the centres, and the F64 ORACLE ITSELF is
    off by millimetres and unstable on oblique pairs (a sphere beside the end of a capsule), which no check here could pin."""
    pa_, va = _mpr_shape(rng, ta, nva)
    pb_, vb = _mpr_shape(rng, tb, nvb)
    d, pb = _unit(rng), rng.uniform(-0.5, 0.5, size=3)
    tilt = 0.0 if rng.random() < 0.5 else rng.uniform(0, 0.02)
    qa = _q_taking(rng, _aligned_dir(rng, ta, va), -d, tilt)
    qb = _q_taking(rng, _aligned_dir(rng, tb, vb), d, 0.0)
    A0 = Shape(ta, _pose([0, 0, 0], qa), pa_ + [0] * (4 - len(pa_)), va)
    B0 = Shape(tb, _pose([0, 0, 0], qb), pb_ + [0] * (4 - len(pb_)), vb)
    target = _mpr_targets(rng)
    pa = pb + d * (target + ref.support_value(A0, -d) + ref.support_value(B0, d))
    b.add(f"{name} (gap {target:.4f} tilt {tilt:.3f})", ta, _pose(pa, qa), pa_, tb, _pose(pb, qb), pb_, va=va, vb=vb, tags=tags)


@functools.lru_cache(maxsize=None)
def mpr_batch(n_each=40):
    b = Batch("mpr")
    rng = np.random.default_rng(20240614)
    d6 = 2.0 ** -6
    cube8 = (np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * d6).astype(np.float32)
    # hull support ties on exact numbers: a box-corner hull probed along a face normal, the lowest index must win
    for k, g in enumerate((2.0 ** -10, -(2.0 ** -10), 2.0 ** -7)):
        for ax in range(3):
            for sg in (1.0, -1.0):
                p = np.zeros(3)
                p[ax] = sg * (d6 + 2.0 ** -5 + g)
                b.add(f"tie sphere over hull face {k}.{ax}.{sg}", SPHERE, _pose(p), [2.0 ** -5], CONVEX, _pose([0, 0, 0]), [], vb=cube8, tags=("tie",))
                b.add(f"tie hull face under sphere {k}.{ax}.{sg}", CONVEX, _pose([0, 0, 0]), [], SPHERE, _pose(p), [2.0 ** -5], va=cube8, tags=("tie",))
    types = (BOX, SPHERE, CAPSULE, CYLINDER, CONVEX)
    for ta in types:
        for tb in types:
            if ta == BOX and tb == BOX:
                continue
            for k in range(n_each):
                _mpr_add(b, rng, f"mpr {ta}-{tb} {k}", ta, tb)
    # every hull vertex count, as shape A and as shape B
    for nv in HULL_COUNTS:
        for k in range(6):
            other = types[k % 5]
            _mpr_add(b, rng, f"hull{nv} as A vs {other} {k}", CONVEX, other, nva=nv)
            _mpr_add(b, rng, f"hull{nv} as B vs {other} {k}", other, CONVEX, nvb=nv)
    return b.finish()


@functools.lru_cache(maxsize=None)
def mpr_boxbox_batch(n=300):
    b = Batch("mpr_boxbox")
    rng = np.random.default_rng(20240615)
    for k in range(n):
        _mpr_add(b, rng, f"forced box-box {k}", BOX, BOX)
    return b.finish()


def mpr_filter(lib64, batch, out64):
    """mask of the cases that stay: all but those on which the F64 ORACLE ALONE flips its count or moves sep by more than
    MPR_PERTURB_SEP under four translations of shape A by MPR_PERTURB: +/- along two directions at right angles to the f64
    oracle's normal (to the line of centres where it reports no contact), which leave the true gap unchanged to second
    order -- what moves is the oracle, not the answer"""
    c0, n0, p0 = split(out64)
    nn = np.where((c0 > 0)[:, None], n0, (batch.pose[:, 0, :3] - batch.pose[:, 1, :3]).astype(np.float64))
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    t1 = np.cross(nn, np.eye(3)[np.argmin(np.abs(nn), axis=1)])
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(nn, t1)
    keep = np.ones(batch.n, dtype=bool)
    for t in (t1, -t1, t2, -t2):
        c, _, p = split(oracle_collide(lib64, batch.moved(MPR_PERTURB * t), force_mpr=True))
        keep &= (c == c0) & ~((c0 > 0) & (np.abs(p[:, 0, 3] - p0[:, 0, 3]) > MPR_PERTURB_SEP))
    assert np.mean(~keep) <= MPR_FILTER_CAP, f"{batch.name}: the stability filter leaves out {np.mean(~keep):.1%} of the class"
    return keep


# ------------------------------------------------------------------------------------------ figures of merit
def _worst(fig, key, i, v, name):
    if v > fig[key][0]:
        fig[key] = (float(v), name)


def eval_boxbox(batch, out, out64, mask=None):
    """{quantity: (largest value, case)} of a box-box result against the reference and the f64 oracle; count and point order
    must equal the f64 oracle's on every case"""
    c, n, p = split(out)
    c64, n64, p64 = split(out64)
    fig = {k: (0.0, None) for k in MEASURED_BOXBOX}
    bad = [batch.names[i] for i in range(batch.n) if c[i] != c64[i] and (mask is None or mask[i])]
    assert not bad, f"{len(bad)} count mismatches against the f64 oracle: {bad[:8]}"
    for i in range(batch.n):
        if (mask is not None and not mask[i]) or c[i] == 0:
            continue
        A, B = batch.shapes(i)
        try:
            r = ref.check_box_box(A, B, batch.offset, int(c[i]), n[i], p[i])
        except AssertionError as e:
            raise AssertionError(f"{batch.names[i]}: {e}") from None
        for k in ("unit", "axis", "depth", "surface", "outside"):
            _worst(fig, k, i, r[k], batch.names[i])
        _worst(fig, "deficit", i, max(r["deficit"], 0.0), batch.names[i])
        _worst(fig, "n_vs_f64", i, np.max(np.abs(n[i] - n64[i])), batch.names[i])
        _worst(fig, "x_vs_f64", i, np.max(np.abs(p[i, :c[i], :3] - p64[i, :c[i], :3])), batch.names[i])
        _worst(fig, "sep_vs_f64", i, np.max(np.abs(p[i, :c[i], 3] - p64[i, :c[i], 3])), batch.names[i])
    return fig


def eval_plane(batch, out, out64):
    """against the closed form (count and order must be the closed form's and the f64 oracle's)"""
    c, n, p = split(out)
    c64, n64, p64 = split(out64)
    fig = {k: (0.0, None) for k in MEASURED_PLANE}
    for i in range(batch.n):
        A, B = batch.shapes(i)
        rc, rn, rp = ref.plane_manifold(A, B, batch.offset)
        assert c[i] == rc and c[i] == c64[i], f"{batch.names[i]}: count {c[i]}, closed form {rc}, f64 oracle {c64[i]}"
        if rc == 0:
            continue
        k = int(c[i])
        _worst(fig, "n", i, np.max(np.abs(n[i] - rn)), batch.names[i])
        _worst(fig, "x", i, np.max(np.abs(p[i, :k, :3] - rp[:, :3])), batch.names[i])
        _worst(fig, "sep", i, np.max(np.abs(p[i, :k, 3] - rp[:, 3])), batch.names[i])
        _worst(fig, "n_vs_f64", i, np.max(np.abs(n[i] - n64[i])), batch.names[i])
        _worst(fig, "x_vs_f64", i, np.max(np.abs(p[i, :k, :3] - p64[i, :k, :3])), batch.names[i])
        _worst(fig, "sep_vs_f64", i, np.max(np.abs(p[i, :k, 3] - p64[i, :k, 3])), batch.names[i])
    return fig


def eval_mpr(batch, out, out64, keep):
    """the value checks of a one-point manifold on the cases the stability filter keeps: (a) sep = g(n), (b) g(n) not below the
    f64 oracle's g, (c) |n| = 1 and n.x on the mid plane, (d) sep = the exact distance where one exists, (e) the f64 oracle's count"""
    c, n, p = split(out)
    c64, n64, p64 = split(out64)
    fig = {k: (0.0, None) for k in MEASURED_MPR}
    bad = [batch.names[i] for i in range(batch.n) if keep[i] and c[i] != c64[i]]
    assert not bad, f"{len(bad)} count mismatches against the f64 oracle: {bad[:8]}"
    for i in range(batch.n):
        if not keep[i] or c[i] == 0:
            continue
        A, B = batch.shapes(i)
        r = ref.check_point_manifold(A, B, batch.offset, n[i], p[i, 0, :3], p[i, 0, 3])
        g64 = ref.gap(A, B, n64[i] / np.linalg.norm(n64[i]))
        _worst(fig, "unit", i, r["unit"], batch.names[i])
        _worst(fig, "sep", i, r["sep"], batch.names[i])
        _worst(fig, "mid", i, r["mid"], batch.names[i])
        _worst(fig, "g_deficit", i, max(g64 - r["g"], 0.0), batch.names[i])
        ex = ref.exact_distance(A, B)
        if ex is not None:
            _worst(fig, "exact", i, abs(p[i, 0, 3] - ex), batch.names[i])
        _worst(fig, "sep_vs_f64", i, abs(p[i, 0, 3] - p64[i, 0, 3]), batch.names[i])
        if "tie" in batch.tags[i]:
            _worst(fig, "tie_x", i, np.max(np.abs(p[i, 0, :3] - p64[i, 0, :3])), batch.names[i])
    return fig


def within(fig, measured, what):
    over = {k: v for k, v in fig.items() if v[0] > measured[k]}
    assert not over, f"{what}: beyond the measured constants: " + ", ".join(f"{k} {v[0]:.3g} > {measured[k]:.3g} ({v[1]})" for k, v in over.items())


def bitwise_share(a, b):
    return float(np.mean(np.all(np.asarray(a).view(np.uint32) == np.asarray(b).view(np.uint32), axis=1)))


def measure():
    from tests import oracle_backend as ob

    l64, l32 = ob.load_oracle("f64"), ob.load_oracle("f32")
    res = {}
    bb = boxbox_batch()
    o64, o32 = oracle_collide(l64, bb), oracle_collide(l32, bb)
    far = bb.tagged("far")
    res["MEASURED_BOXBOX"] = eval_boxbox(bb, o32, o64, ~far)
    res["MEASURED_BOXBOX_FAR"] = eval_boxbox(bb, o32, o64, far)
    for name, b in (("MEASURED_PLANE", plane_batch()), ("MEASURED_PLANE_HULL", plane_hull_batch())):
        res[name] = eval_plane(b, oracle_collide(l32, b), oracle_collide(l64, b))
    for name, b in (("MEASURED_MPR", mpr_batch()), ("MEASURED_MPR_BOXBOX", mpr_boxbox_batch())):
        o64 = oracle_collide(l64, b, force_mpr=True)
        keep = mpr_filter(l64, b, o64)
        print(f"# {b.name}: {b.n} cases, the filter leaves out {np.sum(~keep)} ({np.mean(~keep):.2%})")
        res[name] = eval_mpr(b, oracle_collide(l32, b, force_mpr=True), o64, keep)
    for name, fig in res.items():
        for k, v in fig.items():
            print(f"#   {name}.{k}: f32 oracle max {v[0]:.3e} ({v[1]})")
    for name, fig in res.items():
        print(f"{name} = dict(" + ", ".join(f"{k}={MARGIN * v[0]:.2e}" for k, v in fig.items()) + ")")


if __name__ == "__main__":
    measure()
