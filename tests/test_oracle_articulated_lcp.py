"""The solver's ARTICULATED contact rows against a direct solution of the same complementarity problem.

tests/test_oracle_lcp.py pins the iterative solver on free bodies only. Here the rows touch the articulation: contact rows whose
Jacobian has joint columns, W = A^-1 J^T with A = M + dt Kd + dt^2 Kp (+ tendon), the one-pass force-limit active set that
changes A, the joint-limit rows swept after the contacts, the torsional row bounded by mu r sum(lambda_n). The reference
(tests/indep_lcp.py::solve_substep_generalized) is Lemke's pivoting over generalized coordinates; M and the bias come from the
independent ABA alone (tests/indep_dynamics.py::mass_matrix_and_bias), the Jacobians from the URDF matrix-chain FK. The scenes
and bounds are in tests/articulated_lcp_cases.py; the HIP kernel runs the same scenes in tests/test_gpu_articulated_lcp.py.
"""
import numpy as np
import pytest

from maniskill_amd.model.scenes import PANDA_URDF
from maniskill_amd.model.urdf import parse_urdf
from tests import articulated_lcp_cases as cases
from tests import indep_lcp
from tests import oracle_backend as ob
from tests.articulated_lcp_cases import A_PAD, DT, G, H, KP, N
from tests.indep_dynamics import aba_forward_dynamics, link_point_jacobian, mass_matrix_and_bias, urdf_link_poses

NAMES = list(cases.SCENES)                                                     # every scene with a problem of its own
ON_MESH = [n for n, (b, m) in cases.VARIANTS.items() if m == "ground"]         # same problem, ground contacts out of the triangle stage


def check_complementarity(info):
    z, w = info["z"], info["w"]
    assert z.min() >= -1e-10 and w.min() >= -1e-9 and abs(z @ w) < 1e-9, (z.min(), w.min(), z @ w)


_REFS = {}


def references(sc):
    """the direct solution of every env of a scene, solved once per test session and left unchanged"""
    if sc.base not in _REFS:  # (a mesh variant shares its base scene's problem and entry)
        refs = [cases.reference(sc, e) for e in range(N)]
        for r in refs:
            check_complementarity(r["info"])
        _REFS[sc.base] = refs
    return _REFS[sc.base]


# ---- mass_matrix_and_bias, the Jacobian ---------------------------------------------------------------------------------
def test_mass_matrix_and_bias_reproduce_the_aba_on_random_panda_states():
    rb = parse_urdf(PANDA_URDF)
    rng = np.random.default_rng(3)
    lims = np.array([j.limit for j in rb.joints if j.type != "fixed"])
    for gravity_on in (True, False):
        lg = None if gravity_on else {l: False for l in rb.links}
        for _ in range(4):
            q = rng.uniform(lims[:, 0] * 0.9, lims[:, 1] * 0.9)
            qd, tau = rng.uniform(-1, 1, 9), rng.uniform(-5, 5, 9)
            M, c = mass_matrix_and_bias(rb, q, qd, link_gravity=lg)
            assert np.abs(M - M.T).max() < 1e-12 and np.linalg.eigvalsh(M).min() > 0
            qdd = aba_forward_dynamics(rb, q, qd, tau, link_gravity=lg)
            assert np.abs(M @ qdd + c - tau).max() < 1e-9
    M2, _ = mass_matrix_and_bias(rb, q, qd, armature=np.full(9, 0.1))
    assert np.allclose(M2 - mass_matrix_and_bias(rb, q, qd)[0], 0.1 * np.eye(9), atol=1e-12)


def test_point_jacobian_matches_central_differences_of_the_fk():
    rb = parse_urdf(PANDA_URDF)
    rng = np.random.default_rng(4)
    lims = np.array([j.limit for j in rb.joints if j.type != "fixed"])
    q = rng.uniform(lims[:, 0] * 0.9, lims[:, 1] * 0.9)
    local = np.array([0.01, -0.02, 0.045, 1.0])
    for link in ("panda_leftfinger", "panda_rightfinger", "panda_link4"):
        x = (urdf_link_poses(rb, q)[link] @ local)[:3]
        Jv, Jw = link_point_jacobian(rb, q, link, x)
        for k in range(9):
            d = np.zeros(9)
            d[k] = 1e-6
            Tp, Tm = urdf_link_poses(rb, q + d)[link], urdf_link_poses(rb, q - d)[link]
            assert np.abs(((Tp @ local)[:3] - (Tm @ local)[:3]) / 2e-6 - Jv[:, k]).max() < 1e-8
            S = (Tp[:3, :3] - Tm[:3, :3]) / 2e-6 @ urdf_link_poses(rb, q)[link][:3, :3].T  # Rdot R^T = [w]x
            assert np.abs(np.array([S[2, 1], S[0, 2], S[1, 0]]) - Jw[:, k]).max() < 1e-8


# ---- the generalized solver ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sliding", "sticking", "stack", "pinned", "slipping"])
def test_generalized_solver_equals_the_free_body_solver(name):
    from tests.test_oracle_lcp import scene

    recs, bodies, contacts, names = scene(name)
    v, imp = indep_lcp.solve_substep(bodies, contacts, DT)
    u, imp2, info = indep_lcp.solve_substep_generalized(np.zeros((0, 0)), np.zeros(0), None, bodies, contacts, DT)
    check_complementarity(info)
    assert np.abs(u.reshape(-1, 6) - v).max() < 1e-12 and np.abs(imp.sum(0) - imp2.sum(0)).max() < 1e-12


def test_slider_push_closed_form(tmp_path):
    """one scalar A, one mass, ground friction mu m g: the cube stays while KP t < mu m g, else both move with
    (KP t - mu m g) dt / (A + m); the pad face carries the rest"""
    sc = cases.make_scene("slider_push", tmp_path)
    m = 1000.0 * float(np.float32(0.04)) ** 3 * 8
    fric = 0.3 * m * G
    moved = []
    for e, r in enumerate(references(sc)):
        F = KP * sc.q_target[e, 0]
        v = max(0.0, (F - fric) * DT / (A_PAD + m))
        moved.append(v > 0)
        assert abs(r["qd"][0] - v) < 1e-10 and np.abs(r["v"][0] - [v, 0, 0, 0, 0, 0]).max() < 1e-10
        lam = F * DT - A_PAD * v
        assert np.abs(r["by_pair"][(0, "pad")] - [lam, 0, 0]).max() < 1e-10
        assert abs(r["by_pair"][(0, -1)][2] - m * G * DT) < 1e-10 and abs(r["by_pair"][(0, -1)][0] + min(lam, fric * DT)) < 1e-10
        assert min(abs(F / fric - 1), 1) > 0.1  # 10 % in force off the threshold
    assert moved == [False, False, True, True, True]


def test_slider_limit_closed_form(tmp_path):
    """the joint limit 0.2 mm ahead: the pad (and the cube it pushes) cannot exceed C / dt = 0.02 m/s in this substep"""
    sc = cases.make_scene("slider_limit", tmp_path)
    m = 1000.0 * float(np.float32(0.04)) ** 3 * 8
    fric = 0.3 * m * G
    C = float(np.float32(0.0002))
    limited = []
    for e, r in enumerate(references(sc)):
        F = KP * sc.q_target[e, 0]
        free = max(0.0, (F - fric) * DT / (A_PAD + m))
        v = min(free, C / DT)
        limited.append(free > C / DT)
        assert abs(r["qd"][0] - v) < 1e-10 and abs(r["v"][0][0] - v) < 1e-10
        lam = m * v + min(F, fric) * DT if v > 0 else F * DT  # what the cube needs: its momentum plus the ground's friction
        assert np.abs(r["by_pair"][(0, "pad")] - [lam, 0, 0]).max() < 1e-10
        F_limit = (C / DT) * (A_PAD + m) / DT + fric
        assert abs(F / F_limit - 1) > 0.1 and abs(F / fric - 1) > 0.1
    assert limited == [False, False, False, True, True]


@pytest.mark.parametrize("name", ["two_pad_hold", "two_pad_slip"])
def test_two_pad_closed_form(name, tmp_path):
    """each pad presses with KP t, or with fmax and without its implicit terms once the one-pass check saturates it; pads and cube
    move along x together; the cube is held iff mu (N_l + N_r) > m g, else it slips with g - mu (N_l + N_r) / m"""
    sc = cases.make_scene(name, tmp_path)
    m, mu = 1000.0 * float(np.float32(H)) ** 3 * 8, 0.3
    fmax = sc.drives["jl"][2]
    sats = []
    for e, r in enumerate(references(sc)):
        seen = KP * sc.q_target[e] * (1 - (A_PAD - 1.0) / A_PAD)  # the drive torque of the contact-free solution, what the one-pass check looks at
        sat = seen > fmax
        sats.append(list(sat))
        assert list(r["saturated"]) == list(sat) and np.all(np.abs(seen / fmax - 1) > 0.1)
        F = np.where(sat, fmax, KP * sc.q_target[e])
        A = np.where(sat, 1.0, A_PAD)
        v = DT * (F[0] - F[1]) / (A[0] + m + A[1])
        Nl, Nr = F[0] - A[0] * v / DT, F[1] + A[1] * v / DT
        assert Nl > 0 and Nr > 0 and abs(mu * (Nl + Nr) / (m * G) - 1) > 0.1
        vz = 0.0 if mu * (Nl + Nr) > m * G else -(G - mu * (Nl + Nr) / m) * DT
        assert (vz == 0.0) == (name == "two_pad_hold")
        assert np.abs(r["qd"] - [v, -v]).max() < 1e-10 and np.abs(r["v"][0] - [v, 0, vz, 0, 0, 0]).max() < 1e-10
        assert abs(r["by_pair"][(0, "padl")][0] - Nl * DT) < 1e-10 and abs(r["by_pair"][("padr", 0)][0] - Nr * DT) < 1e-10
    assert sats == [[False, False]] * 3 + [[True, False], [True, True]]


def test_turntable_twist_closed_form(tmp_path):
    """the relative spin stops while w0 / (1 / I + 1 / A) <= mu m g dt (r + 2 H) (the torsional row plus four corners * two axes
    * mu m g / 4 * H); beyond, everything is at its bound: the cube loses T / I, the table gains T / A"""
    sc = cases.make_scene("turntable_twist", tmp_path)
    h = float(np.float32(H))
    m, mu = 1000.0 * h**3 * 8, 0.3
    I, A = m * (2 * h) ** 2 / 6, 0.02 + DT * 1e2 + DT * DT * KP
    T = mu * m * G * DT * (0.1 + 2 * h)
    for e, r in enumerate(references(sc)):
        w0 = sc.spin[e, 0, 2]
        need = w0 / (1 / I + 1 / A)
        assert abs(need / T - 1) > 0.1
        wc, wt = (I * w0 / (I + A),) * 2 if need <= T else (w0 - T / I, T / A)
        assert np.abs(r["v"][0] - [0, 0, 0, 0, 0, wc]).max() < 1e-10 * max(1.0, w0) and abs(r["qd"][0] - wt) < 1e-10  # (relative: the spins are of order 10)
    assert [r["v"][0][5] - r["qd"][0] > 1e-9 for r in references(sc)] == [False, False, False, True, True]


def test_fetch_limits_rows_switch_on_one_after_the_other(tmp_path):
    """torso (dof 3), right finger (13), left finger (14), each 0.2 mm from a limit with its target beyond: a row pushes iff the
    joint's contact-free velocity (A^-1 rhs) exceeds C / dt, every such velocity is 10 % off that threshold, a pushing row leaves
    its joint at exactly C / dt towards the limit (A couples the three to other joints, the rest is Lemke's)"""
    sc = cases.make_scene("fetch_limits", tmp_path)
    dofs, sign = (cases.FETCH_TORSO, cases.FETCH_R, cases.FETCH_L), np.array([1.0, -1.0, 1.0])
    pushing = []
    for e, r in enumerate(references(sc)):
        pb = cases.problem(sc, e)
        free = np.linalg.solve(pb["A"], pb["rhs"])
        rows = {k: (s, C) for k, s, C in pb["limits"]}
        on = []
        for k, sg in zip(dofs, sign):
            s, C = rows[k]
            assert s == -sg and abs(C - 0.0002) < 2e-7, (k, s, C)  # (the row's sign is that of the limit's normal: away from it)
            assert abs(sg * free[k] / (C / DT) - 1) > 0.1, (e, k, free[k], C / DT)
            on.append(bool(sg * free[k] > C / DT))
            assert abs(r["qd"][k] - (sg * C / DT if on[-1] else free[k])) < (1e-10 if on[-1] else 1e-3), (e, k, r["qd"][k])
        lam = {pb["limits"][i][0]: x for i, x in enumerate(r["info"]["lam"][len(r["contacts"]):])}
        assert [bool(lam[k] > 1e-9) for k in dofs] == on and not any(x > 1e-9 for k, x in lam.items() if k not in dofs)
        pushing.append(on)
    assert pushing == [[False, False, False], [True, False, False], [True, True, False], [True, True, False], [True, True, True]]
    # the torso's drive is saturated in the last two envs (its row then holds a joint without implicit terms), no other drive is
    assert [[k for k in range(15) if r["saturated"][k]] for r in references(sc)] == [[], [], [], [cases.FETCH_TORSO], [cases.FETCH_TORSO]]


@pytest.mark.parametrize("name", NAMES)
def test_solution_does_not_depend_on_the_covering_vector(name, tmp_path):
    """a scene must have ONE velocity solution: Lemke started from other covering vectors ends in the same place. So must
    what is compared of the impulses: each pair's normal part and the net impulse on a body, and the whole pair impulse
    where the scene says it is unique"""
    sc = cases.make_scene(name, tmp_path)
    rng = np.random.default_rng(7)
    for e, r in enumerate(references(sc)):
        n = len(r["info"]["z"])
        for _ in range(2):
            other = cases.reference(sc, e, covering=rng.uniform(0.5, 2.0, n))
            check_complementarity(other["info"])
            assert np.abs(other["qd"] - r["qd"]).max() < 1e-9 and (not sc.frees or np.abs(other["v"] - r["v"]).max() < 1e-9), (name, e)
            for k, w in r["by_pair"].items():
                d = other["by_pair"][k] - w
                assert max(abs(d @ part) for part in cases.compared_parts(sc, e, r, k)) < 1e-9, (name, e, k, d)


def second_solution(info, objective):
    """another solution of the LCP with the SAME velocities and slacks that maximises objective . z, by linear programming over
    the multipliers the complementarity pattern leaves free (-> z, checked like every solution); None if the program fails"""
    from scipy.optimize import linprog

    z, w, M, n_un, n_fr = info["z"], info["w"], info["M"], info["n_un"], info["n_fr"]
    n, nv = len(z), n_un + 2 * n_fr
    sigma = z[nv:]
    lo_hi = [(0.0, None) if w[i] < 1e-10 else (0.0, 0.0) for i in range(nv)] + [(s_, s_) for s_ in sigma]
    at_bound = np.array([i for i in range(nv, n) if sigma[i - nv] > 1e-10], dtype=int)
    inside = np.array([i for i in range(nv, n) if sigma[i - nv] <= 1e-10], dtype=int)
    A_eq = np.vstack([M[:nv], M[at_bound]])
    b_eq = np.concatenate([M[:nv] @ z, np.zeros(len(at_bound))])
    for tol in (1e-10, 1e-9, 1e-8):  # (what the program returns counts only if it passes the same check as every solution)
        res = linprog(-np.asarray(objective), A_ub=-M[inside], b_ub=np.zeros(len(inside)), A_eq=A_eq, b_eq=b_eq, bounds=lo_hi, method="highs",
                      options=dict(primal_feasibility_tolerance=tol, dual_feasibility_tolerance=tol))
        if res.status != 0:
            continue
        z2 = np.maximum(res.x, 0.0)
        w2 = M @ z2 + info["q"]
        if w2.min() >= -1e-9 and abs(z2 @ w2) < 1e-9:
            return z2
    return None


@pytest.mark.parametrize("name", [n for n in NAMES if not all(cases.SCENES[n](n).tangent_unique)])
def test_a_held_bodys_pair_impulses_are_not_unique(name, tmp_path):
    """where a scene leaves a friction part of a pair impulse out of the comparison (Scene.tangent_unique False and the pair not
    sliding along that axis), that is needed: in every such env a second solution of the same LCP exists, with the same
    velocities, whose impulse along a left-out axis differs (constructed by a linear program, or reached by Lemke from another
    covering vector; checked for complementarity either way)"""
    sc = cases.make_scene(name, tmp_path)
    for e, r in enumerate(references(sc)):
        if sc.tangent_unique[e]:
            continue
        info, spread = r["info"], 0.0
        n_un, n_fr = info["n_un"], info["n_fr"]
        for key in r["by_pair"]:
            idx = [k for k, c in enumerate(r["contacts"]) if (c[0], c[1]) == key]
            for t in (0, 1):
                if r["sliding"][key][t]:
                    continue
                obj = np.zeros(len(info["z"]))
                for k in idx:
                    obj[n_un + 2 * k + t], obj[n_un + n_fr + 2 * k + t] = 1.0, -1.0
                z2 = second_solution(info, obj)
                if z2 is not None:
                    spread = max(spread, abs(obj @ (z2 - info["z"])))
        if spread < 1e-6:  # (the program is badly scaled with the Panda's two boxes; Lemke from other covering vectors reaches such solutions too)
            rng = np.random.default_rng(7)
            for _ in range(4):
                other = cases.reference(sc, e, covering=rng.uniform(0.5, 2.0, len(info["z"])))
                assert np.abs(other["qd"] - r["qd"]).max() < 1e-9 and np.abs(other["v"] - r["v"]).max() < 1e-9
                spread = max(spread, max(np.abs(other["by_pair"][k] - w).max() for k, w in r["by_pair"].items()))
        print(f"\nSECOND SOLUTION {name} env {e}: a left-out friction part moves by {spread:.3g} N s")
        assert spread > 1e-6, (name, e, spread)  # (solutions of one problem agree to 1e-9)


def pair_state(sc, r):
    """the active set, said in what is unique (the multipliers of coplanar points are not): per body pair pushing or not, per
    friction axis sliding or not (the LCP's slack sigma is the size of the relative velocity along a friction row); torsional rows
    turning or not; limit rows pushing or not; drives saturated or not"""
    info, out = r["info"], []
    nc = len(r["contacts"])
    lam, sigma = info["lam"], info["sigma"]
    for a, b, axis in sc.pairs:
        idx = [k for k, c in enumerate(r["contacts"]) if (c[0], c[1]) == (a, b)]
        out.append((a, b, bool(lam[idx].sum() > 1e-9)) + tuple(bool(max(sigma[2 * k + t] for k in idx) > 1e-7) for t in (0, 1)))
    out.append(tuple(bool(x > 1e-9) for x in lam[nc:]))          # limit rows
    out.append(tuple(bool(x > 1e-7) for x in sigma[2 * nc :]))   # torsional rows
    out.append(tuple(bool(x) for x in r["saturated"]))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_every_env_is_clear_of_its_thresholds(name, tmp_path):
    """the reference's active set -- which rows are at a bound, which drives are saturated -- does not change when the swept
    parameter moves by +-1 %, nor by +-10 % (the swept parameters are forces, or proportional to one); and the envs of a scene do
    not all take the same branch"""
    sc = cases.make_scene(name, tmp_path)
    states = [pair_state(sc, r) for r in references(sc)]
    for f in (0.99, 1.01, 0.9, 1.1):
        moved = cases.scaled(sc, f)
        for e in range(N):
            r = cases.reference(moved, e)
            check_complementarity(r["info"])
            assert pair_state(moved, r) == states[e], (name, e, f)
    assert len({repr(s) for s in states}) > 1, states


# ---- the oracle against the direct solution -----------------------------------------------------------------------------------
def alignment(sc):
    """of the scene's own links, in every env: each pad's box is axis-aligned in the world (its frame a signed permutation); two
    pads that hold the same free body along an axis face each other along that axis and nowhere else (their link frames differ
    along it alone, by the body's width plus the pads' own offsets); the Panda's and panda_stick's hand points down"""
    for e in range(N):
        T = urdf_link_poses(sc.robot, sc.q[e], cases._root_T(sc.root_p))
        for link, s in sc.pads.items():
            R = (T[link] @ cases._T44(s.pose))[:3, :3]
            assert np.abs(np.abs(R) - np.abs(R).round()).max() < 1e-6 and np.abs(np.abs(R).round().sum(0) - 1).max() == 0, (sc.name, link, R)
        if "panda_hand" in T:
            assert np.abs(T["panda_hand"][:3, :3] @ [0, 0, 1] - [0, 0, -1]).max() < 1e-6
        held = {}
        for a, b, axis in sc.pairs:
            for link, body in ((a, b), (b, a)):
                if isinstance(link, str) and not isinstance(body, str) and body >= 0:
                    held.setdefault((body, axis), []).append(link)
        for (body, axis), links in held.items():
            if len(links) == 2:
                pa, pb = (T[l] @ cases._T44(sc.pads[l].pose) for l in links)
                d = np.abs(pa[:3, 3] - pb[:3, 3])
                width = 2 * sc.frees[body].half[axis] + sum((np.abs(X[:3, :3]).round() @ sc.pads[l].half_size)[axis] for l, X in zip(links, (pa, pb)))
                want = np.zeros(3)
                want[axis] = width
                assert np.abs(d - want).max() < 1e-6, (sc.name, links, d, want)


def sweeps_have_exited(sc, precision):
    """the sweeps stopped at MSSIM_PGS_EXIT_TOLERANCE before the allowed count: twice as many change nothing"""
    a = cases.run_solver(ob.make_system(cases.compile_scene(sc), N, precision=precision), sc, cases.compile_scene(sc))
    b = cases.run_solver(ob.make_system(cases.compile_scene(sc, 2 * sc.sweeps), N, precision=precision), sc, cases.compile_scene(sc, 2 * sc.sweeps))
    return np.array_equal(a["qd"], b["qd"]) and np.array_equal(a["v"], b["v"])


@pytest.mark.parametrize("name", cases.CASES)
def test_f64_oracle_matches_direct_solution(name, tmp_path):
    """every scene and every mesh variant: contact counts equal to the reference's points per pair (four per face, also where the
    face lies on the one-triangle ground), velocities and impulses within the f64 bounds, the sweeps stopped by their tolerance"""
    sc = cases.make_scene(name, tmp_path)
    alignment(sc)
    model = cases.compile_scene(sc)
    px = ob.make_system(model, N, precision="f64")
    got = cases.run_solver(px, sc, model)
    assert px.overflow_count() == 0
    ev, ei = cases.errors(sc, model, got, references(sc))
    print(f"\nMEASURED_F64 {name}: velocity {ev:.3g} impulse {ei:.3g}")
    assert sweeps_have_exited(sc, "f64")
    # (TOL_F64's two exceptions are of the first ten scenes; a mesh variant is its base scene's problem and is held to that scene's
    # bound, slider_push's among them. No scene added since has an exception)
    tol_v, tol_i = cases.TOL_F64.get(sc.base, (cases.TOL_V_F64, cases.TOL_I_F64))
    assert ev < tol_v and ei < tol_i, (ev, ei)


@pytest.mark.parametrize("name", NAMES + ON_MESH)
def test_f32_oracle_matches_direct_solution(name, tmp_path):
    """the figures F32_ORACLE_ERROR holds are re-measured here: they must not have grown by more than a quarter (the kernel's
    bounds are 4 x the largest of a family; a figure that drifted would make them mean less)"""
    sc = cases.make_scene(name, tmp_path)
    model = cases.compile_scene(sc)
    px = ob.make_system(model, N, precision="f32")
    got = cases.run_solver(px, sc, model)
    assert px.overflow_count() == 0
    ev, ei = cases.errors(sc, model, got, references(sc))
    print(f"\nMEASURED_F32 {name}: velocity {ev:.3g} impulse {ei:.3g}")
    rec_v, rec_i = cases.F32_ORACLE_ERROR[name]
    assert ev <= 1.25 * rec_v and ei <= 1.25 * rec_i, (ev, ei)


# ---- references broken on purpose -------------------------------------------------------------------------------------------
# jacobian_sign flips the last joint's column where the pad's rows have one (branch_arm: the slide j3); else the last joint on the
# pad's path to the base with a column that counts: panda_stick's joint 6 (the push passes by joint 7's axis at 0.015 m), the
# Fetch's torso under the torso pad
FLIPPED_JOINT = {"stick_drag": 5, "fetch_ground_press": 3}
def broken_reference(sc, env, how):
    """the direct solution of a problem with one row type written wrongly"""
    pb = dict(cases.problem(sc, env))
    if how == "jacobian_sign":               # the sign of a link's Jacobian column (the last joint's, unless that one's is zero)
        jac = pb["jac"]
        flip = np.ones(len(pb["rhs"]))
        flip[FLIPPED_JOINT.get(sc.base, -1)] = -1.0
        pb["jac"] = lambda link, x: tuple(J * flip for J in jac(link, x))
    elif how == "tendon_diagonal_only":      # the tendon's off-diagonal dropped from A
        pb["A"] = pb["A"] - sum((DT * DT * k + DT * d) * (np.outer(cc, cc) - np.diag(cc * cc)) for cc, o_, k, d in pb["tendons"])
    elif how == "saturated_keeps_implicit":  # dt Kd + dt^2 Kp kept on a saturated joint
        pb["A"] = pb["A"] + np.diag(np.where(pb["saturated"], pb["implicit"], 0.0))
    elif how == "torsion_one_point":         # the torsional bound summed over one point instead of the patch
        pb["torsion"] = [(a, b, n, mur, members[:1]) for a, b, n, mur, members in pb["torsion"]]
    else:
        raise KeyError(how)
    return cases.solve(pb)


# which scene owns which row type: broken there, the reference must be more than ten of the KERNEL's bounds away from the oracle
BREAKS = [
    ("jacobian_sign", "level_arm_press"),
    ("jacobian_sign", "panda_pinch_tendon"),
    ("jacobian_sign", "fetch_pinch"),            # (the last joint: the left finger's own column)
    ("jacobian_sign", "fetch_ground_press"),
    ("jacobian_sign", "stick_drag"),
    ("jacobian_sign", "branch_arm_two_cubes"),
    ("jacobian_sign", "level_arm_press_on_mesh"),
    ("tendon_diagonal_only", "panda_pinch_tendon"),
    ("saturated_keeps_implicit", "two_pad_hold"),
    ("torsion_one_point", "turntable_twist"),
]


@pytest.mark.parametrize("how,name", BREAKS)
def test_a_broken_reference_is_noticed(how, name, tmp_path):
    sc = cases.make_scene(name, tmp_path)
    model = cases.compile_scene(sc)
    got = cases.run_solver(ob.make_system(model, N, precision="f64"), sc, model)
    ev, ei = cases.errors(sc, model, got, [broken_reference(sc, e, how) for e in range(N)])
    print(f"\nBROKEN {how} in {name}: velocity {ev:.3g} ({ev / cases.MEASURED_V[name]:.0f} bounds) impulse {ei:.3g} ({ei / cases.MEASURED_I[name]:.0f} bounds)")
    assert ev > 10 * cases.MEASURED_V[name], (ev, ei)
