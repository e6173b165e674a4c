"""Seeded case tables for the iterative-IK block (tests/ik_reference.py states what must come out), on the Panda: the
TCP link (10), whose path holds dofs 0-6, joint limits from the model's `dof_limit`. Env counts are those of
tests/action_cases.ENV_COUNTS (128, 1, 17, 67); the table of N envs is the first N rows of one seeded sequence per
(set, rows), so the first 17 envs of the 128-env table ARE the 17-env table.

  near  q0 = rest + 0.3 u, target = FK(clip(q0 + d u', limits -+ 0.05)) with d = 0.1 (even envs) / 0.5 (odd envs):
        every env converges in a few iterations;
  wide  q0 = rest + 1.0 u, d = 1.0: some targets are reached only at the iteration cap (joint limits, near-singular
        poses).
`nan=True` (the stand-alone form only) puts NaN into one position component of the LAST env's target.

Map form (`build_map`): per mode the action a controller would receive and the previous target pose.
  mode 1 (target-delta, normalised columns): the previous target is FK(q0) displaced by a seeded 1 cm / 0.02 rad, the
         columns are seeded uniform in [-1.3, 1.3] (so some are clipped), every 5th env commands zero;
  mode 0 (absolute pose, raw columns): position and XYZ Euler angles of the near set's target."""
import numpy as np

from tests import action_cases as ac
from tests import action_reference as ar
from tests import ik_reference as ik

SEED = 20261018
LINK = 10
ROWS = (3, 6)
SETS = {"near": (0.3, (0.1, 0.5)), "wide": (1.0, (1.0, 1.0))}
ENV_COUNTS = ac.ENV_COUNTS
MAX_N = 3072
K_FORMS = (1, 2, 5)  # tolerance = 0: exactly K iterations


def _fk_pose(A, q):
    pe, qe, _ = ar.link_fk_jacobian(A, q, LINK)
    return np.concatenate([pe, qe], 1)


def _sequence(A, rest, name, rows, count):
    spread, ds = SETS[name]
    lim = np.asarray(A["dof_limit"], dtype=np.float64)
    rest = np.asarray(rest, dtype=np.float64)
    n = len(rest)
    path = ar.path_dofs(A, LINK)
    rng = np.random.default_rng([SEED, sum(map(ord, name)), rows])
    u, u2 = rng.uniform(-1.0, 1.0, (count, n)), rng.uniform(-1.0, 1.0, (count, n))
    q0 = np.tile(rest, (count, 1))
    q0[:, path] = np.clip(rest[path] + spread * u[:, path], lim[path, 0], lim[path, 1])
    d = np.where(np.arange(count) % 2 == 0, ds[0], ds[1])[:, None]
    q1 = q0.copy()
    q1[:, path] = np.clip(q0[:, path] + d * u2[:, path], lim[path, 0] - 0.05, lim[path, 1] + 0.05)
    return q0.astype(np.float32), _fk_pose(A, q1).astype(np.float32)


_CACHE = {}


def build(A, rest, name, rows, N, nan=False):
    """-> dict q0 [N, n_dof] f32, target [N, 7] f32 (root frame), labels"""
    key = (name, rows, N > max(ENV_COUNTS))
    if key not in _CACHE:
        _CACHE[key] = _sequence(A, rest, name, rows, MAX_N if key[2] else max(ENV_COUNTS))
    q0, target = (x[:N].copy() for x in _CACHE[key])
    labels = [f"{name} rows={rows} N={N} env {e}" for e in range(N)]
    if nan:
        target[N - 1, 1] = np.nan
        labels[N - 1] += " NAN target"
    return dict(q0=q0, target=target, labels=labels, nan=nan)


def quat_to_euler_xyz(q):
    """angles a with Rx(a0) Ry(a1) Rz(a2) = R(q), q [N, 4] wxyz unit"""
    w, x, y, z = np.moveaxis(np.asarray(q, np.float64), -1, 0)
    r00, r01, r02 = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    r12, r22 = 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)
    return np.stack([np.arctan2(-r12, r22), np.arcsin(np.clip(r02, -1.0, 1.0)), np.arctan2(-r01, r00)], -1)


def build_map(A, rest, ikspec, N):
    """ikspec = (link, column0, rows, mode, low, high, rot_scale, flags) -> dict q0, prev_pose [N, 7] f32, columns
    [N, rows] f32 (the block's own columns; the caller places them at column0), labels"""
    link, c0, rows, mode = ikspec[:4]
    assert link == LINK
    near = build(A, rest, "near", rows, N)
    rng = np.random.default_rng([SEED, 77, rows, mode])
    r = rng.uniform(-1.0, 1.0, (max(ENV_COUNTS), 16))[:N]
    here = _fk_pose(A, near["q0"].astype(np.float64))
    if mode == 1:
        prev = here.copy()
        prev[:, :3] += 0.01 * r[:, :3]
        prev[:, 3:] = ar._qmul(ik.euler_xyz_quat(0.02 * r[:, 3:6]), here[:, 3:])
        cols = 1.3 * r[:, 6 : 6 + rows]
        cols[np.arange(N) % 5 == 4] = 0.0
    else:
        prev = here.copy()  # (overwritten by the absolute modes)
        t = near["target"].astype(np.float64)
        cols = np.concatenate([t[:, :3], quat_to_euler_xyz(ar._unit(t[:, 3:]))], 1)[:, :rows]
    return dict(q0=near["q0"], prev_pose=prev.astype(np.float32), columns=cols.astype(np.float32),
                labels=[f"map mode={mode} rows={rows} N={N} env {e}" for e in range(N)])


def panda_tables():
    """(model arrays, rest joint positions) of the Panda tabletop model, without an env"""
    from maniskill_amd.model.scenes import panda_tabletop_model

    A = panda_tabletop_model().arrays
    rest = np.array([0.0, np.pi / 8, 0.0, -np.pi * 5 / 8, 0.0, np.pi * 3 / 4, np.pi / 4, 0.04, 0.04])
    return A, rest


def compare(C, R, q, iters, band, what, measured=False):
    """q [N, n_dof] f32 / f64 and iters [N] of the code under test against the reference result R on the table C.
    Envs whose iteration count equals the reference's are held to `band` on q; the others (default settings only:
    at most 2 % of the table, and by no more than 1 iteration) to max|err| < 2e-5 at the returned q -- evaluated by the
    caller-supplied residual in R["residual"](q). NaN exactly where the reference says NaN. Returns the largest |dq|."""
    q = np.asarray(q, dtype=np.float64)
    N = len(q)
    nanref = np.isnan(R["q"])
    assert np.array_equal(np.isnan(q), nanref), f"{what}: NaN pattern differs from the reference's"
    ok = ~nanref.any(1)
    same = (np.asarray(iters) == R["iters"]) & ok
    diff = ok & ~same
    assert np.abs(np.asarray(iters)[diff] - R["iters"][diff]).max(initial=0) <= 1, f"{what}: iteration count off by more than 1"
    assert diff.sum() <= 0.02 * N, f"{what}: iteration count differs in {diff.sum()} of {N} envs"
    for e in np.flatnonzero(diff):
        res = R["residual"](e, q[e])
        assert res < 2e-5, f"{what}: {C['labels'][e]}: count {iters[e]} vs {R['iters'][e]}, residual {res:.3e}"
    dq = np.abs(q - R["q"]).max(1)
    worst = float(dq[same].max(initial=0.0))
    if not measured:
        bad = same & (dq > band)
        assert not bad.any(), f"{what}: {C['labels'][int(np.flatnonzero(bad)[0])]}: |dq| {dq[bad].max():.3e} > band {band:.3e}"
    return worst
