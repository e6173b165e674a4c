"""The float64 reference of the end-effector blocks with held joints (tests/held_ik_reference.py) and its cases on the
Fetch (tests/fetch_ik_cases.py), checked on the CPU before the HIP kernels are held to them
(tests/test_gpu_fetch_ee.py):

  1. the reference is pinned three ways: with no held joint it is tests/ik_reference.py (and, for the delta step,
     tests/action_reference.py) bit for bit on the Panda tables; with the held joints frozen at one set of values it
     equals tests/ik_reference.py run on the solved chain alone, rooted at the composed prefix; one planar case is
     computed by hand;
  2. the Fetch tables: *near* converges below the iteration cap in every env, the limits hold, held and off-path dofs
     come back as q0's bits, a NaN target or a NaN held position gives NaN on that env's solved dofs alone;
  3. the band: a float32 restatement of the kernel's formula (the held prefix composed once in float32, then the loop
     of tests/test_ik_reference.ik_f32 from that transform) against the reference, see MEASURED. Its iteration count
     differs from the reference's in at most 2 % of the envs of any table and by at most one iteration -- the allowance
     tests/ik_cases.compare gives.

MEASURED: the largest |q32 - q_ref|_inf of the restatement over the tables (N = 128, 1, 17, 67 and one of 1024 envs), per
(set, form, rows), recorded rounded up to two digits with `python -m tests.test_held_ik_reference`. The band used on
the GPU is 4 x the recorded value; the test asserts that the restatement stays within the recorded value and reaches at
least a fifth of it."""
import numpy as np
import pytest

import maniskill_amd  # noqa: F401  (installs the gymnasium stand-in where the real module is absent)
from tests import action_reference as ar
from tests import fetch_ik_cases as fc
from tests import held_ik_reference as hr
from tests import ik_cases as ic
from tests import ik_reference as ik
from tests.test_ik_reference import settings_of

FORMS = [("near", "default")] + [(s, f"K{k}") for s in ("near", "wide") for k in fc.K_FORMS]
EXTRA_N = fc.MAX_N
# largest |q32 - q_ref|_inf of the float32 restatement, per (set, form, rows); the band is 4 x this
MEASURED = {
    ("near", "default", 3): 1.2e-6, ("near", "default", 6): 4.2e-6,
    ("near", "K1", 3): 7.8e-7, ("near", "K1", 6): 2.3e-6,
    ("near", "K2", 3): 1.1e-6, ("near", "K2", 6): 2.5e-6,
    ("near", "K5", 3): 8.0e-7, ("near", "K5", 6): 3.4e-6,
    ("wide", "K1", 3): 1.4e-6, ("wide", "K1", 6): 2.2e-5,
    ("wide", "K2", 3): 1.9e-6, ("wide", "K2", 6): 2.7e-5,
    ("wide", "K5", 3): 2.1e-6, ("wide", "K5", 6): 3.9e-5,
}


def band(name, form, rows):
    return 4.0 * MEASURED[(name, form, rows)]


# ---------------------------------------------------------------- float32 restatement of the kernel's formula
def held_ik_f32(A, link, q0, target, rows, held, max_iters=60, damping=1e-3, max_step=0.3, tolerance=1e-5):
    """every operation rounded to float32, in the kernel's order: the held prefix composed once per env, then the loop
    over the solved chain from that transform -> (q [N, n_dof] f32, iters [N])"""
    f = np.float32
    path, sel, solved = hr.split_path(A, link, list(held))
    assert path[: len(held)] == list(held)
    unit = lambda fr: np.concatenate([fr[:3], fr[3:] / np.linalg.norm(fr[3:])]).astype(f)  # normalised in double, as the host does
    frame_of = {j: unit(np.asarray(A["dof_frame"][j], np.float64)) for j in path}
    axis_of = {j: np.asarray(A["dof_axis"][j], f) for j in path}
    rev_of = {j: int(A["dof_type"][j]) == 0 for j in path}
    tip = unit(np.asarray(A["link_frame"][link], np.float64))
    lim = np.asarray(A["dof_limit"], f)[solved]
    damping, max_step, tolerance = f(damping), f(max_step), f(tolerance)
    q0 = np.asarray(q0, f)
    N = len(q0)
    Q, T = q0[:, solved].copy(), np.asarray(target, f)
    iters, active = np.zeros(N, np.int64), np.ones(N, bool)
    conj = np.array([1, -1, -1, -1], f)

    def joint(j, p, r, qj):
        """one joint at positions qj [M, 1] on top of (p, r) -> (p, r, world axis, anchor)"""
        M = len(p)
        jp = p + ar._qrot(r, frame_of[j][:3])
        jq = ar._qmul(r, np.broadcast_to(frame_of[j][3:], (M, 4)))
        a = ar._qrot(jq, axis_of[j])
        if rev_of[j]:
            h = f(0.5) * qj
            return jp, ar._qmul(jq, np.concatenate([np.cos(h), np.sin(h) * axis_of[j]], 1)), a, jp
        return jp + a * qj, jq, a, jp

    with np.errstate(invalid="ignore", over="ignore"):
        P0, R0 = np.zeros((N, 3), f), np.tile(np.array([1, 0, 0, 0], f), (N, 1))
        for j in held:
            P0, R0, _, _ = joint(j, P0, R0, q0[:, j : j + 1])
        assert P0.dtype == f and R0.dtype == f
        for it in range(max_iters + 1):
            idx = np.flatnonzero(active)
            if idx.size == 0:
                break
            q, M = Q[idx], len(idx)
            p, r = P0[idx], R0[idx]
            ax, an = [], []
            for k, j in enumerate(solved):
                p, r, a, anc = joint(j, p, r, q[:, k : k + 1])
                ax.append(a)
                an.append(anc)
            pe = p + ar._qrot(r, tip[:3])
            err = T[idx, :3] - pe
            if rows == 6:
                qe = ar._qmul(r, np.broadcast_to(tip[3:], (M, 4)))
                d = ar._qmul(T[idx, 3:], qe * conj)
                d = np.where(d[:, :1] < 0, -d, d)
                nv = np.sqrt((d[:, 1:2] * d[:, 1:2] + d[:, 2:3] * d[:, 2:3]) + d[:, 3:4] * d[:, 3:4])
                ang = f(2) * np.arctan2(nv, d[:, :1])
                err = np.concatenate([err, d[:, 1:] / np.maximum(nv, f(1e-9)) * ang], 1)
            assert err.dtype == f and pe.dtype == f
            stop = (np.abs(err).max(1) < tolerance) | (it >= max_iters)
            active[idx[stop]] = False
            idx, err = idx[~stop], err[~stop]
            if idx.size == 0:
                continue
            M = len(idx)
            J = np.zeros((M, rows, len(solved)), f)
            G = np.zeros((M, rows, rows), f)
            G[:, np.arange(rows), np.arange(rows)] = damping
            for k, j in enumerate(solved):
                a, anc = ax[k][~stop], an[k][~stop]
                J[:, :3, k] = np.cross(a, pe[~stop] - anc) if rev_of[j] else a
                if rows == 6 and rev_of[j]:
                    J[:, 3:, k] = a
                G = G + J[:, :, None, k] * J[:, None, :, k]
            L = np.zeros((M, rows, rows), f)
            for i in range(rows):
                for jj in range(i + 1):
                    s = G[:, i, jj].copy()
                    for m in range(jj):
                        s = s - L[:, i, m] * L[:, jj, m]
                    L[:, i, jj] = np.sqrt(np.maximum(s, f(1e-20))) if i == jj else s / L[:, jj, jj]
            z, y = np.zeros((M, rows), f), np.zeros((M, rows), f)
            for i in range(rows):
                s = err[:, i].copy()
                for m in range(i):
                    s = s - L[:, i, m] * z[:, m]
                z[:, i] = s / L[:, i, i]
            for i in range(rows - 1, -1, -1):
                s = z[:, i].copy()
                for m in range(i + 1, rows):
                    s = s - L[:, m, i] * y[:, m]
                y[:, i] = s / L[:, i, i]
            step = np.zeros((M, len(solved)), f)
            for i in range(rows):
                step = step + J[:, i, :] * y[:, i : i + 1]
            big = np.abs(step).max(1)
            step = step * (max_step / np.maximum(big, max_step))[:, None]
            assert step.dtype == f and L.dtype == f
            Q[idx] = np.minimum(np.maximum(Q[idx] + step, lim[:, 0]), lim[:, 1])
            iters[idx] += 1
    out = q0.copy()
    out[:, solved] = Q
    return out, iters


_REF = {}


def reference(A, link, name, form, rows, N, nan=None):
    """the reference's result on a Fetch case table, computed once per table and shared (treat as read-only); carries
    "residual": (env, q [n_dof]) -> max|err| at q in float64"""
    key = (name, form, rows, N, nan)
    if key not in _REF:
        C = fc.build(A, link, name, rows, N, nan=nan)
        R = hr.solve(A, link, C["q0"], C["target"], rows, held=fc.HELD, **settings_of(form))
        T = C["target"].astype(np.float64)
        R["residual"] = lambda e, q: hr.residual(A, link, q, T[e], rows)
        _REF[key] = (C, R)
    return _REF[key]


def _measure(A, link, name, form, rows):
    worst, counts = 0.0, []
    for N in fc.ENV_COUNTS + (EXTRA_N,):
        C, R = reference(A, link, name, form, rows, N)
        q, iters = held_ik_f32(A, link, C["q0"], C["target"], rows, fc.HELD, **settings_of(form))
        worst = max(worst, ic.compare(C, R, q, iters, 0.0, f"restatement fetch {name} {form} rows={rows} N={N}", measured=True))
        counts.append(int((iters != R["iters"]).sum()))
    return worst, counts


@pytest.fixture(scope="module")
def fetch():
    return fc.fetch_tables()


# ---------------------------------------------------------------- 1. the reference, pinned
@pytest.mark.parametrize("rows", ic.ROWS)
@pytest.mark.parametrize("name", list(ic.SETS))
def test_no_held_joint_is_the_plain_reference_bit_for_bit(name, rows):
    A, rest = ic.panda_tables()
    for N in (17, 67):
        C = ic.build(A, rest, name, rows, N, nan=(N == 17))
        want = ik.solve(A, ic.LINK, C["q0"], C["target"], rows)
        got = hr.solve(A, ic.LINK, C["q0"], C["target"], rows, held=())
        for k in ("q", "iters", "err", "raw_step"):
            assert np.array_equal(got[k], want[k], equal_nan=True), (name, rows, N, k)
        assert got["path"] == want["path"] == got["solved"]
    # the map form of the iterative block and the delta step
    ikspec = (ic.LINK, 0, rows, 1, -0.1, 0.1, -0.1, 2)
    M = ic.build_map(A, rest, ikspec, 67)
    want, got = ik.apply(ikspec, A, M["q0"], M["prev_pose"], M["columns"]), hr.apply(ikspec, A, M["q0"], M["prev_pose"], M["columns"])
    assert np.array_equal(got["q"], want["q"]) and np.array_equal(got["pose"], want["pose"]) and np.array_equal(got["iters"], want["iters"])
    spec = ([-1] * 9, [0.0] * 9, [0.0] * 9, [4] * 7 + [0, 0], (ic.LINK, 0, rows, -0.1, 0.1, 0.1, 2))
    prev = np.zeros((67, 9))
    want = ar.apply_action(spec, A, M["q0"], prev, prev, M["columns"])
    got = hr.apply_action(spec, A, M["q0"], prev, prev, M["columns"])
    for k in ("tq", "tv", "wq", "wv", "kappa", "dq_inf", "kappa_j", "dq"):
        assert np.array_equal(got[k], want[k]), k
    assert got["ee_dofs"] == want["ee_dofs"]


@pytest.mark.parametrize("rows", fc.ROWS)
def test_frozen_held_joints_equal_the_plain_reference_on_the_rooted_chain(fetch, rows):
    A, link = fetch
    C = fc.build(A, link, "near", rows, 17)
    q_held = C["q0"][3, fc.HELD].astype(np.float64)  # one set of held positions for every env
    q0 = C["q0"].astype(np.float64)
    q0[:, fc.HELD] = q_held
    target = np.tile(C["target"][3].astype(np.float64), (17, 1))  # reachable at those held positions
    got = hr.solve(A, link, q0, target, rows, held=fc.HELD)
    B = hr.rooted_chain(A, link, fc.HELD, q_held)
    assert ar.path_dofs(B, link) == fc.SOLVED
    want = ik.solve(B, link, q0, target, rows)
    assert np.array_equal(got["iters"], want["iters"]) and (got["iters"] > 0).any() and (got["iters"] < 60).all()
    assert np.abs(got["q"] - want["q"]).max() <= 1e-9  # (the prefix enters through one composed frame there: another order of roundings)
    assert np.array_equal(got["q"][:, fc.HELD], q0[:, fc.HELD])
    # and the delta step: the solved joints' columns of the whole chain are the rooted chain's Jacobian
    flags = [0] * 15
    for j in fc.SOLVED:
        flags[j] = 4
    for j in fc.HELD:
        flags[j] = 64
    a = np.random.default_rng(5).uniform(-1, 1, (17, rows))
    prev = np.zeros((17, 15))
    ee = (link, 0, rows, -0.1, 0.1, 0.1, 2)
    got = hr.apply_action(([-1] * 15, [0.0] * 15, [0.0] * 15, flags, ee), A, q0, prev, prev, a)
    want = ar.apply_action(([-1] * 15, [0.0] * 15, [0.0] * 15, [f & 4 for f in flags], ee), B, q0, prev, prev, a)
    assert got["ee_dofs"] == want["ee_dofs"] == fc.SOLVED and np.abs(got["tq"] - want["tq"]).max() <= 1e-9
    # holding is not the same as solving over every path joint
    full = ar.apply_action(([-1] * 15, [0.0] * 15, [0.0] * 15, [4 if f else 0 for f in flags], ee), A, q0, prev, prev, a)
    assert np.abs(full["tq"][:, fc.SOLVED] - got["tq"][:, fc.SOLVED]).max() > 1e-3


def test_planar_case_computed_by_hand():
    """joint 0 (held): revolute about z at the origin, at pi / 2; joint 1 (solved): prismatic along its parent's x, which
    now points along the root's y; the link sits 0.5 further along. So pe = (0, 0.5 + q1, 0) and Js = (0, 1, 0)^T:
      delta step:  dq1 = a_y / (1 + 1e-9), whatever a_x and a_z are;
      iterative:   err = (0, e, 0), step = e / (1 + 1e-3): e shrinks by r = 1e-3 / 1.001 per iteration; from e0 = 0.2
                   that is 2.0e-4, then 2.0e-7 < 1e-5: two iterations, q1 = q1_0 + e0 (1 - r^2)."""
    ident = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    A = dict(dof_frame=np.array([ident, ident]), dof_axis=np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]), dof_type=np.array([0, 1]),
             dof_parent=np.array([-1, 0]), dof_limit=np.array([[-10.0, 10.0], [-10.0, 10.0]]), link_body=np.array([0, 1]),
             link_frame=np.array([ident, [0.5, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]]))
    q0 = np.array([[np.pi / 2, 0.1]])
    prev = np.zeros((1, 2))
    R = hr.apply_action(([-1, -1], [0.0, 0.0], [0.0, 0.0], [64, 4], (1, 0, 3, 0.0, 0.0, 0.0, 0)), A, q0, prev, prev, np.array([[0.3, 0.05, -0.2]]))
    assert R["ee_dofs"] == [1] and abs(R["tq"][0, 1] - (0.1 + 0.05 / (1 + 1e-9))) < 1e-15 and R["tq"][0, 0] == 0.0
    target = np.array([[0.0, 0.8, 0.0, 1.0, 0.0, 0.0, 0.0]])  # e0 = 0.8 - (0.5 + 0.1)
    S = hr.solve(A, 1, q0, target, 3, held=[0])
    r = 1e-3 / 1.001
    assert S["iters"][0] == 2 and abs(S["q"][0, 1] - (0.1 + 0.2 * (1 - r * r))) < 1e-13 and S["q"][0, 0] == np.pi / 2
    # without the bit joint 0 takes the column z x pe = (-0.6, 0, 0) and the x command turns it: dq0 = -0.6 a_x / (0.36 + 1e-9)
    F = ar.apply_action(([-1, -1], [0.0, 0.0], [0.0, 0.0], [4, 4], (1, 0, 3, 0.0, 0.0, 0.0, 0)), A, q0, prev, prev, np.array([[0.3, 0.05, -0.2]]))
    assert abs(F["tq"][0, 0] - (np.pi / 2 - 0.18 / (0.36 + 1e-9))) < 1e-12 and abs(F["tq"][0, 1] - R["tq"][0, 1]) < 1e-12


# ---------------------------------------------------------------- 2. the Fetch tables
@pytest.mark.parametrize("rows", fc.ROWS)
@pytest.mark.parametrize("name", list(fc.SETS))
def test_fetch_tables_are_sound(fetch, name, rows):
    A, link = fetch
    lim = np.asarray(A["dof_limit"], np.float64)
    off = [j for j in range(15) if j not in fc.SOLVED]
    for N in fc.ENV_COUNTS:
        C, R = reference(A, link, name, "default", rows, N)
        assert R["solved"] == fc.SOLVED and R["path"] == fc.PATH
        assert (R["q"][:, fc.SOLVED] >= lim[fc.SOLVED, 0]).all() and (R["q"][:, fc.SOLVED] <= lim[fc.SOLVED, 1]).all()
        assert np.array_equal(R["q"][:, off], C["q0"][:, off].astype(np.float64))
        assert np.abs(C["q0"][:, :2]).max() <= 1.0 and np.abs(C["q0"][:, 2]).max() <= np.pi + 1e-6
        assert (C["q0"][:, 3] >= lim[3, 0] - 1e-6).all() and (C["q0"][:, 3] <= lim[3, 1] + 1e-6).all()
        if name == "near":
            assert (R["iters"] < 60).all() and (R["err"] < 1e-5).all(), (N, R["iters"].max(), R["err"].max())
    big = fc.build(A, link, name, rows, 128)
    for N in (1, 17, 67):
        C = fc.build(A, link, name, rows, N)
        assert np.array_equal(C["q0"], big["q0"][:N]) and np.array_equal(C["target"], big["target"][:N])
    assert len(np.unique(big["q0"][:, 2])) == 128 and np.ptp(big["q0"][:, 0]) > 1.5 and np.ptp(big["q0"][:, 3]) > 0.2
    clean = reference(A, link, name, "default", rows, 17)[1]
    for nan in ("target", "held"):
        C, R = reference(A, link, name, "default", rows, 17, nan=nan)
        assert np.isnan(R["q"][16, fc.SOLVED]).all() and R["iters"][16] == 60
        keep = np.ones((17, 15), bool)
        keep[16, fc.SOLVED] = False
        assert np.array_equal(R["q"][keep], np.where(np.isnan(C["q0"]), np.nan, clean["q"])[keep], equal_nan=True)
        assert np.isfinite(R["q"][:16]).all()


# ---------------------------------------------------------------- 3. the band
@pytest.mark.parametrize("rows", fc.ROWS)
@pytest.mark.parametrize("name,form", FORMS)
def test_float32_restatement_stays_within_the_recorded_band(fetch, name, form, rows):
    A, link = fetch
    worst, counts = _measure(A, link, name, form, rows)  # (ic.compare asserts the 2 % / one-iteration allowance per table)
    rec = MEASURED[(name, form, rows)]
    print(f"fetch {name} {form} rows={rows}: largest |q32 - q_ref| {worst:.3e}, recorded {rec:.3e}, envs with another count {counts}")
    assert worst <= rec, (name, form, rows, worst)
    assert worst >= rec / 5.0, f"the band (4 x {rec:.3e}) is more than 20 x loose: the restatement reaches {worst:.3e}"
    if form != "default":
        assert counts == [0] * len(counts)


def test_restatement_with_no_held_joint_is_the_panda_restatement():
    from tests.test_ik_reference import ik_f32

    A, rest = ic.panda_tables()
    C = ic.build(A, rest, "wide", 6, 67)
    q, it = held_ik_f32(A, ic.LINK, C["q0"], C["target"], 6, [])
    q2, it2 = ik_f32(A, ic.LINK, C["q0"], C["target"], 6)
    assert np.array_equal(q, q2) and np.array_equal(it, it2)


if __name__ == "__main__":
    A, link = fc.fetch_tables()
    for (name, form) in FORMS:
        for rows in fc.ROWS:
            worst, counts = _measure(A, link, name, form, rows)
            print(f'    ("{name}", "{form}", {rows}): {worst:.3e},   # other count: {counts}')
