"""An independent, DIRECT solution of the contact problem of one substep, to pin the oracle's (and the kernel's) iterative
solver -- the way tests/indep_dynamics.py pins the articulated dynamics with a different algorithm.

The product and the oracle run projected Gauss-Seidel sweeps over rows (normal + two friction rows per point, box
pyramid |lambda_t| <= mu lambda_n per tangent axis, speculative bias gap / dt). Here the same physical model is written as
one linear complementarity problem over free rigid bodies and solved by LEMKE's complementary pivoting (Cottle, Pang,
Stone, "The Linear Complementarity Problem", ch. 4.4): no sweeps, no iteration count, no warm start. Per tangent axis j
of a contact the friction impulse is beta_j+ - beta_j- with beta >= 0 and a slack sigma_j (Stewart & Trinkle 1996;
Anitescu & Potra 1997, written per axis so that the admissible set is the solver's box pyramid, not the diamond):

    w_n   = Jn v+ + gap / dt                     >= 0   _|_  lambda_n >= 0
    w_j+  =  (Jt_j v+) + sigma_j                 >= 0   _|_  beta_j+  >= 0
    w_j-  = -(Jt_j v+) + sigma_j                 >= 0   _|_  beta_j-  >= 0
    w_sj  = mu lambda_n - beta_j+ - beta_j-      >= 0   _|_  sigma_j  >= 0
    v+    = v* + M^-1 J^T lambda,     v* = v + dt (g + f / m)  (bodies start without spin in the scenes used: no gyroscopic term)

The multipliers of coplanar points are not unique (a box on four corners is statically indeterminate); what is unique, and
what the tests compare, are the bodies' velocities after the substep and the impulse each body pair exchanges.
"""
import numpy as np


def lemke(M, q, max_iter=2000, d=None):
    """w = M z + q >= 0, z >= 0, z.w = 0 by Lemke's algorithm with covering vector d > 0, 1 unless given (Cottle, Pang, Stone,
    algorithm 4.4.5). A problem with one solution has it whatever d is: two runs with different d are a uniqueness check."""
    n = len(q)
    if np.all(q >= 0):
        return np.zeros(n)
    d = np.ones(n) if d is None else np.asarray(d, dtype=np.float64)
    # tableau [I | -M | -d | q]: basis starts as w
    T = np.hstack([np.eye(n), -M, -d.reshape(-1, 1), q.reshape(-1, 1)]).astype(np.float64)
    basis = list(range(n))  # 0..n-1: w, n..2n-1: z, 2n: z0
    r = int(np.argmin(q / d))
    entering = 2 * n

    def pivot(row, col):
        T[row] /= T[row, col]
        for i in range(n):
            if i != row:
                T[i] -= T[i, col] * T[row]

    pivot(r, entering)
    leaving, basis[r] = basis[r], entering
    for _ in range(max_iter):
        entering = leaving + n if leaving < n else leaving - n  # the complement of what left
        col = T[:, entering]
        rows = np.where(col > 1e-12)[0]
        if len(rows) == 0:
            raise RuntimeError("Lemke: ray termination")
        ratios = T[rows, -1] / col[rows]
        best = ratios.min()
        ties = rows[ratios <= best + 1e-14 + 1e-12 * abs(best)]
        # if z0 can leave, let it (the solution is reached); other ties are broken lexicographically over the columns of the
        # basis inverse (the w block of the tableau): no cycling on the degenerate problems coplanar points make
        row = next((i for i in ties if basis[i] == 2 * n), None)
        if row is None:
            row = ties[0]
            if len(ties) > 1:
                cand = list(ties)
                for k in range(n):
                    vals = np.array([T[i, k] / col[i] for i in cand])
                    keep = vals <= vals.min() + 1e-14
                    cand = [i for i, kp in zip(cand, keep) if kp]
                    if len(cand) == 1:
                        break
                row = cand[0]
        pivot(row, entering)
        leaving, basis[row] = basis[row], entering
        if leaving == 2 * n:
            z = np.zeros(2 * n + 1)
            for i, b in enumerate(basis):
                z[b] = T[i, -1]
            return z[n : 2 * n]
    raise RuntimeError("Lemke: iteration limit")


def tangents(n):
    """the friction axes of a contact normal: the solver's documented convention (include/mssim.h: pyramid friction along
    t1 = normalize(n x e_x) -- n x e_y when n is within 54.7 degrees of e_x --, t2 = n x t1)"""
    n = np.asarray(n, dtype=np.float64)
    helper = np.array([1.0, 0, 0]) if abs(n[0]) < 0.57735 else np.array([0, 1.0, 0])
    t1 = np.cross(n, helper)
    t1 /= np.linalg.norm(t1)
    return t1, np.cross(n, t1)


def solve_substep(bodies, contacts, dt, gravity=(0, 0, -9.81)):
    """bodies: dicts(m, I = 3x3 world inertia about the centre of mass, x = centre of mass, v, w, f = external force, gravity: bool);
    contacts: (a, b, x, n, gap, mu): body indices (-1 = fixed), point, unit normal from b towards a, signed gap, friction.
    -> (v+ [nb, 6] lin | ang, impulses [nc, 3] world impulse on body a of each contact)"""
    nb, nc = len(bodies), len(contacts)
    g = np.asarray(gravity, dtype=np.float64)
    Minv = np.zeros((6 * nb, 6 * nb))
    vstar = np.zeros(6 * nb)
    for i, B in enumerate(bodies):
        Minv[6 * i : 6 * i + 3, 6 * i : 6 * i + 3] = np.eye(3) / B["m"]
        Minv[6 * i + 3 : 6 * i + 6, 6 * i + 3 : 6 * i + 6] = np.linalg.inv(B["I"])
        acc = (g if B.get("gravity", True) else 0 * g) + np.asarray(B.get("f", np.zeros(3))) / B["m"]
        vstar[6 * i : 6 * i + 3] = np.asarray(B["v"]) + dt * acc
        vstar[6 * i + 3 : 6 * i + 6] = np.asarray(B["w"])

    def row(a, b, x, d):
        J = np.zeros(6 * nb)
        for body, sgn in ((a, 1.0), (b, -1.0)):
            if body >= 0:
                J[6 * body : 6 * body + 3] = sgn * d
                J[6 * body + 3 : 6 * body + 6] = sgn * np.cross(np.asarray(x) - bodies[body]["x"], d)
        return J

    Jn = np.array([row(a, b, x, np.asarray(n, float)) for a, b, x, n, gap, mu in contacts])
    Jt = np.array([row(a, b, x, t) for a, b, x, n, gap, mu in contacts for t in tangents(n)])  # [2 nc]
    mu = np.array([c[5] for c in contacts])
    bias = np.array([c[4] for c in contacts]) / dt
    nt = 2 * nc
    # unknowns z = [lambda_n (nc) | beta+ (nt) | beta- (nt) | sigma (nt)]
    Ann, Ant, Att = Jn @ Minv @ Jn.T, Jn @ Minv @ Jt.T, Jt @ Minv @ Jt.T
    E = np.eye(nt)
    P = np.zeros((nt, nc))  # tangent row -> its contact
    for k in range(nt):
        P[k, k // 2] = 1.0
    Z = np.zeros
    M = np.block([
        [Ann, Ant, -Ant, Z((nc, nt))],
        [Ant.T, Att, -Att, E],
        [-Ant.T, -Att, Att, E],
        [P * mu[None, :], -E, -E, Z((nt, nt))],
    ])
    q = np.concatenate([Jn @ vstar + bias, Jt @ vstar, -(Jt @ vstar), np.zeros(nt)])
    z = lemke(M, q)
    lam_n, lam_t = z[:nc], z[nc : nc + nt] - z[nc + nt : nc + 2 * nt]
    v = vstar + Minv @ (Jn.T @ lam_n + Jt.T @ lam_t)
    imp = np.zeros((nc, 3))
    for k, (a, b, x, n, gap, mu_k) in enumerate(contacts):
        t1, t2 = tangents(n)
        imp[k] = lam_n[k] * np.asarray(n, float) + lam_t[2 * k] * t1 + lam_t[2 * k + 1] * t2
    return v.reshape(nb, 6), imp


# --------------------------------------------------------------------------------------------------------------------
# One fixed-base articulation plus free bodies (restated here and not taken from the oracle).
#
# The velocity vector is u = [qd | 6 per free body]. The drives and the tendon are integrated implicitly, so the joint block
# of the "mass" the constraint impulses act on is A = M + dt Kd + dt^2 Kp + w c c^T, and the free velocity of the joints is
# A^-1 rhs. On top of the contact rows above there are unilateral joint-limit rows +-e_j with bias C / dt, and per patch one
# torsional row -- relative spin about the patch normal -- written like a tangent axis (beta+, beta-, sigma) whose bound is
# mu_t r times the SUM of the patch's normal multipliers.


def joint_space_system(M, c, q, qd, dt, kp, kd, fmax, q_target, qd_target=None, qf=None, tendons=()):
    """A qd* = rhs of the implicit drive integration with the one-pass force limit.
    A = M + dt Kd + dt^2 Kp + sum w cc cc^T (w = dt^2 k + dt d per tendon (cc, offset, k, d): the constraint cc.q = offset),
    rhs = M qd + dt (Kp (q_t - q) + Kd qd_t + tau_tendon - c + qf). Solved once; a joint whose implicit drive torque
    kp (q_t - q - dt qd*) + kd (qd_t - qd*) exceeds fmax in size gets the constant +-fmax instead and loses dt kd + dt^2 kp;
    the caller solves again. -> (A, rhs, saturated [n] bool)"""
    q, qd, kp, kd, fmax, q_target = (np.asarray(a, dtype=np.float64) for a in (q, qd, kp, kd, fmax, q_target))
    n = len(q)
    qd_target = np.zeros(n) if qd_target is None else np.asarray(qd_target, dtype=np.float64)
    qf = np.zeros(n) if qf is None else np.asarray(qf, dtype=np.float64)
    base, tau_t = np.array(M, dtype=np.float64), np.zeros(n)
    for cc, offset, k, d in tendons:
        cc = np.asarray(cc, dtype=np.float64)
        base += (dt * dt * k + dt * d) * np.outer(cc, cc)
        tau_t -= k * (cc @ q - offset) * cc
    implicit = dt * kd + dt * dt * kp
    free_rhs = M @ qd + dt * (tau_t - np.asarray(c) + qf)
    A = base + np.diag(implicit)
    rhs = free_rhs + dt * (kp * (q_target - q) + kd * qd_target)
    v = np.linalg.solve(A, rhs)
    drive = kp * (q_target - q - dt * v) + kd * (qd_target - v)
    sat = np.abs(drive) > fmax
    A = base + np.diag(np.where(sat, 0.0, implicit))
    rhs = np.where(sat, free_rhs + dt * np.sign(drive) * np.where(sat, fmax, 0.0), rhs)
    return A, rhs, sat


def solve_substep_generalized(A, rhs, link_jacobian, bodies, contacts, dt, limits=(), torsion=(), gravity=(0, 0, -9.81), covering=None):
    """A, rhs: the joint-space system (joint_space_system); link_jacobian(link, x) -> (Jv, Jw) [3, n] each of the point x on `link`;
    bodies: as in solve_substep; contacts: (a, b, x, n, gap, mu) where a side is a free-body index, -1 (fixed) or a link name;
    limits: (joint, side = +-1, C >= 0): the row side * qd_j + C / dt >= 0;
    torsion: (a, b, n, mu_t * r, [contact indices of the patch]): |torque about n| <= mu_t r sum lambda_n over those contacts.
    -> (u+ [n + 6 nb], world impulse on side a per contact [nc, 3], info: z, w of the LCP, lam: the unilateral rows' multipliers,
    sigma: per friction row the size of the relative velocity along it, M, q: the LCP itself, n_un, n_fr: its unilateral and friction row counts)"""
    A = np.asarray(A, dtype=np.float64)
    nq, nb, nc = A.shape[0], len(bodies), len(contacts)
    nu = nq + 6 * nb
    g = np.asarray(gravity, dtype=np.float64)
    Minv = np.zeros((nu, nu))
    ustar = np.zeros(nu)
    if nq:
        Minv[:nq, :nq] = np.linalg.inv(A)
        ustar[:nq] = Minv[:nq, :nq] @ np.asarray(rhs, dtype=np.float64)
    for i, B in enumerate(bodies):
        o = nq + 6 * i
        Minv[o : o + 3, o : o + 3] = np.eye(3) / B["m"]
        Minv[o + 3 : o + 6, o + 3 : o + 6] = np.linalg.inv(B["I"])
        acc = (g if B.get("gravity", True) else 0 * g) + np.asarray(B.get("f", np.zeros(3))) / B["m"]
        ustar[o : o + 3] = np.asarray(B["v"]) + dt * acc
        ustar[o + 3 : o + 6] = np.asarray(B["w"])

    def row(a, b, x, lin, ang):
        """relative velocity (a minus b) of the point x along `lin`, plus relative angular velocity along `ang`"""
        J = np.zeros(nu)
        for side, sgn in ((a, 1.0), (b, -1.0)):
            if isinstance(side, str):
                Jv, Jw = link_jacobian(side, x)
                J[:nq] += sgn * (lin @ Jv + ang @ Jw)
            elif side >= 0:
                o = nq + 6 * side
                J[o : o + 3] += sgn * lin
                J[o + 3 : o + 6] += sgn * (np.cross(np.asarray(x) - bodies[side]["x"], lin) + ang)
        return J

    zero3 = np.zeros(3)
    Ju = [row(a, b, x, np.asarray(n, float), zero3) for a, b, x, n, gap, mu in contacts]
    bu = [gap / dt for a, b, x, n, gap, mu in contacts]
    for j, side, C in limits:
        e = np.zeros(nu)
        e[j] = side
        Ju.append(e)
        bu.append(C / dt)
    Jf = [row(a, b, x, t, zero3) for a, b, x, n, gap, mu in contacts for t in tangents(n)]
    for a, b, n, mur, members in torsion:
        Jf.append(row(a, b, zero3, zero3, np.asarray(n, float)))
    n_un, n_fr = len(Ju), len(Jf)
    Ju, Jf, bu = np.array(Ju).reshape(n_un, nu), np.array(Jf).reshape(n_fr, nu), np.array(bu)
    bound = np.zeros((n_fr, n_un))  # friction row -> what its bound sums, with the coefficient
    for k, c in enumerate(contacts):
        bound[2 * k, k] = bound[2 * k + 1, k] = c[5]
    for t, (a, b, n, mur, members) in enumerate(torsion):
        bound[2 * nc + t, list(members)] = mur
    # unknowns z = [lambda (n_un) | beta+ (n_fr) | beta- (n_fr) | sigma (n_fr)]
    Auu, Auf, Aff = Ju @ Minv @ Ju.T, Ju @ Minv @ Jf.T, Jf @ Minv @ Jf.T
    E, Z = np.eye(n_fr), np.zeros
    Mlcp = np.block([
        [Auu, Auf, -Auf, Z((n_un, n_fr))],
        [Auf.T, Aff, -Aff, E],
        [-Auf.T, -Aff, Aff, E],
        [bound, -E, -E, Z((n_fr, n_fr))],
    ])
    qlcp = np.concatenate([Ju @ ustar + bu, Jf @ ustar, -(Jf @ ustar), np.zeros(n_fr)])
    # Coplanar points make the problem degenerate and a pivot on rounding noise can end in a vector that is no solution: a
    # result is taken only if it IS one (the checks below), else the pivoting starts again from another covering vector
    rng = np.random.default_rng(len(qlcp))
    z = None
    for d in [covering] + [rng.uniform(0.5, 2.0, len(qlcp)) for _ in range(8)]:
        try:
            cand = lemke(Mlcp, qlcp, max_iter=20000, d=d)
        except RuntimeError:
            continue
        w = Mlcp @ cand + qlcp
        if cand.min() >= -1e-10 and w.min() >= -1e-9 and abs(cand @ w) < 1e-9:
            z = np.maximum(cand, 0.0)
            break
    if z is None:
        raise RuntimeError("Lemke: no covering vector led to a solution")
    lam, lam_f = z[:n_un], z[n_un : n_un + n_fr] - z[n_un + n_fr : n_un + 2 * n_fr]
    u = ustar + Minv @ (Ju.T @ lam + Jf.T @ lam_f)
    imp = np.zeros((nc, 3))
    for k, (a, b, x, n, gap, mu_k) in enumerate(contacts):
        t1, t2 = tangents(n)
        imp[k] = lam[k] * np.asarray(n, float) + lam_f[2 * k] * t1 + lam_f[2 * k + 1] * t2
    sigma = z[n_un + 2 * n_fr :]  # per friction row: the size of the relative velocity along it (0: sticking)
    return u, imp, dict(z=z, w=Mlcp @ z + qlcp, lam=lam, sigma=sigma, M=Mlcp, q=qlcp, n_un=n_un, n_fr=n_fr)
