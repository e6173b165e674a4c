"""The float64 action-map reference (tests/action_reference.py) and its cases (tests/action_cases.py), checked on the
CPU before the HIP kernels are held to them (tests/test_gpu_action_map.py):

  * the reference's own FK / Jacobian against the f64 oracle's `link_jacobian` for every Panda link under tilted,
    displaced roots. Derived tolerance: the oracle's output is rounded to float32 and its entries are below 2 in
    magnitude -> half an ulp of 2 = 1.2e-7, 2e-7 absolute;
  * the torch controllers (`agent.set_action` on the f32 oracle backend: the path MS_FUSED=0 takes) against the
    reference on every finite case, joint-space entries within the derived band (action_reference.joint_bound),
    end-effector entries within the band below;
  * the conditions of the case set: at most 1 % of the envs of a case table fall outside the tight end-effector
    comparison, and every kind of case is present.

End-effector band:  (K kappa_2(G) + K2 kappa_2(J)) 2^-23 |dq_ref|_inf + 4 * 2^-23 |q|,  G = J J^T + 1e-9 I.  (K, K2) is
four times the pair that just covers a float32 numpy restatement of the kernel's formula (3 x 3 adjugate, 6 x 6
unpivoted Cholesky, the Gram matrix summed joint by joint) fed with the Jacobian of the f32 oracle's FK, over the finite
cases in the tight comparison of the committed tables (N = 128, 1, 17, 67) and of one table of 3072 envs more per map.
Measured with `python -m tests.test_action_reference`:
  pd_ee_delta_pos (3 rows), 2036 cases, kappa_2(G) 1.68 .. 2.6e3, kappa_2(J) 1.3 .. 51: largest
    err / (2^-23 kappa_2(G) |dq|) = 4.47 -- in the best-conditioned quarter; 0.91 in the worst: the FK's rounding scales
    with kappa_2(J), so K alone would be 20 x loose where it matters -- and err / (2^-23 kappa_2(J) |dq|) = 12.1.
    Recorded pair (2.93, 2.0): the restatement reaches 1.00 of it (best-conditioned quarter 1.00, worst 0.295), i.e.
    0.25 / 0.074 of the band. No env above the kappa cap in any table.
  pd_ee_delta_pose (6 rows), 2378 cases, kappa_2(G) 64 .. 8.1e3, kappa_2(J) 8 .. 90: largest
    err / (2^-23 kappa_2(G) |dq|) = 0.436 (worst-conditioned quarter; 0.228 in the best). Recorded pair (0.437, 0): no
    second term needed, 0.13 / 0.25 of the band in the best / worst quarter. Above the kappa cap: 3 of 128, 0 of 1, 17
    and 67, 99 of 3072 envs, all of them in the uniform-within-limits pose set, which is outside the tight comparison
    with 6 rows as a whole.
  The cases that command the smallest normal float32 move the joints by ~1e-38: below float32's underflow threshold no
  relative band holds; they are kept out of the measurement and held by the band's absolute term.
The test asserts that the restatement stays within the recorded pair, so the band cannot drift from what it was derived
from, and holds the torch path to the full band."""
import numpy as np
import pytest
import torch

import maniskill_amd  # noqa: F401  (installs the gymnasium stand-in where the real module is absent)
from maniskill_amd.model.scenes import panda_tabletop_model
from tests import action_cases as ac
from tests import action_reference as ref
from tests import oracle_backend as ob

# (K, K2) that just cover the float32 restatement's error (see above), per number of rows; the band uses 4 x that
MEASURED = {3: (2.93, 2.0), 6: (0.437, 0.0)}
K = {rows: (4.0 * k, 4.0 * k2) for rows, (k, k2) in MEASURED.items()}
EXTRA_N = 3072
UNDERFLOW = 1e-30


def band_k(spec):
    return K[spec[4][2]] if spec[4] is not None else (0.0, 0.0)


def _make(name, N, precision="f32"):
    import gymnasium as gym

    import maniskill_amd.envs  # noqa: F401

    backend = ob.register(precision, f"oracle_{precision}_env")
    env_id, kw = ac.env_spec(name)
    env = gym.make(env_id, num_envs=N, sim_backend=backend, **kw)
    env.reset(seed=0)
    return env


def _quat_random(rng, N):
    q = rng.normal(size=(N, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def test_reference_jacobian_matches_f64_oracle_under_tilted_roots():
    model = panda_tabletop_model()
    N = 48
    px = ob.make_system(model, N, precision="f64")
    rng = np.random.default_rng(11)
    lim = model.arrays["dof_limit"].astype(np.float64)
    q = (lim[:, 0] + (lim[:, 1] - lim[:, 0]) * rng.uniform(size=(N, model.n_dof))).astype(np.float32)
    root = np.concatenate([rng.uniform(-1, 1, (N, 3)), _quat_random(rng, N)], 1).astype(np.float32)
    root[0] = [0, 0, 0, 1, 0, 0, 0]
    px.cuda_articulation_qpos.torch()[:] = torch.from_numpy(q)
    px.cuda_rigid_body_data.torch()[:N, :7] = torch.from_numpy(root)
    px.gpu_apply_all()
    px.gpu_update_articulation_kinematics()
    for link in range(model.n_link):
        J = ref.link_fk_jacobian(model.arrays, q.astype(np.float64), link)[2]
        got = px.link_jacobian(link).double().numpy()
        assert np.abs(J).max() < 2.0
        err = np.abs(got - J).max()
        assert err <= 2e-7, (model.link_names[link], err)


# ---------------------------------------------------------------- float32 restatement of the end-effector block
def _ee_f32(J, cmd):
    """J [N, rows, k] f32 (columns = joints on the path, root side first), cmd [N, rows] f32 -> dq [N, k] f32, every
    operation rounded to float32, in the kernel's order"""
    f = np.float32
    N, rows, k = J.shape
    G = np.zeros((N, rows, rows), f)
    G[:, np.arange(rows), np.arange(rows)] = f(1e-9)
    for j in range(k):
        G = (G + (J[:, :, None, j] * J[:, None, :, j]).astype(f)).astype(f)
    y = np.zeros((N, rows), f)
    if rows == 3:
        xx, yy, zz, xy, xz, yz = G[:, 0, 0], G[:, 1, 1], G[:, 2, 2], G[:, 0, 1], G[:, 0, 2], G[:, 1, 2]
        c = [(yy * zz - yz * yz).astype(f), (xz * yz - xy * zz).astype(f), (xy * yz - xz * yy).astype(f),
             (xx * zz - xz * xz).astype(f), (xy * xz - xx * yz).astype(f), (xx * yy - xy * xy).astype(f)]  # adjugate: xx xy xz yy yz zz
        det = ((xx * c[0]).astype(f) + (xy * c[1]).astype(f) + (xz * c[2]).astype(f)).astype(f)
        inv = [(ci / det).astype(f) for ci in c]
        a = cmd
        y[:, 0] = inv[0] * a[:, 0] + inv[1] * a[:, 1] + inv[2] * a[:, 2]
        y[:, 1] = inv[1] * a[:, 0] + inv[3] * a[:, 1] + inv[4] * a[:, 2]
        y[:, 2] = inv[2] * a[:, 0] + inv[4] * a[:, 1] + inv[5] * a[:, 2]
    else:
        L = np.zeros((N, 6, 6), f)
        for r in range(6):
            for q in range(r + 1):
                s = G[:, r, q].copy()
                for m in range(q):
                    s = (s - (L[:, r, m] * L[:, q, m]).astype(f)).astype(f)
                L[:, r, q] = np.sqrt(np.maximum(s, f(1e-20))).astype(f) if r == q else (s / L[:, q, q]).astype(f)
        z = np.zeros((N, 6), f)
        for r in range(6):
            s = cmd[:, r].copy()
            for m in range(r):
                s = (s - (L[:, r, m] * z[:, m]).astype(f)).astype(f)
            z[:, r] = (s / L[:, r, r]).astype(f)
        for r in range(5, -1, -1):
            s = z[:, r].copy()
            for m in range(r + 1, 6):
                s = (s - (L[:, m, r] * y[:, m]).astype(f)).astype(f)
            y[:, r] = (s / L[:, r, r]).astype(f)
    dq = np.zeros((N, k), f)
    for r in range(rows):
        dq = (dq + (J[:, r, :] * y[:, r : r + 1]).astype(f)).astype(f)
    return dq


def _restatement_ratios(name, N):
    """|dq32 - dq_ref|_inf / (2^-23 |dq_ref|_inf) per env of the table (name, N) -> (that, kappa_2(G), kappa_2(J), tight)"""
    env = _make(name, N, "f32")
    base = env.unwrapped
    spec = base.agent.controller.fused_action_spec()
    A, lim, rest, root0 = ac.tables(base)
    C = ac.build(name, spec, lim, rest, root0, N)
    ac.write_state(base, C)
    R = ac.reference(spec, A, C)
    link, rows = spec[4][0], spec[4][2]
    path = ref.path_dofs(A, link)
    J = base.scene.px.link_jacobian(link).numpy()[:, :rows][:, :, path]
    e = spec[4]
    cmd = ref.ee_command((link, e[1], rows, float(np.float32(e[3])), float(np.float32(e[4])), float(np.float32(e[5])), e[6]), C["action"].astype(np.float64)).astype(np.float32)
    dq32 = _ee_f32(J, cmd).astype(np.float64)
    dq_ref = R["dq"]
    env.close()
    # (a relative band describes float32 above its underflow threshold only: the cases that command the smallest normal
    # float32 move the joints by ~1e-38 and are held by the band's absolute term, 4 * 2^-23 |q|, alone)
    moving = R["dq_inf"] > UNDERFLOW
    assert not (np.abs(dq32[~moving]) > 2 * UNDERFLOW).any()
    e = np.zeros(N)
    e[moving] = np.abs(dq32 - dq_ref).max(1)[moving] / (ref.EPS32 * R["dq_inf"])[moving]
    return e, R["kappa"], R["kappa_j"], ac.tight(spec, C, R) & moving


EE_MAPS = ["panda:pd_ee_delta_pos", "panda:pd_ee_delta_pose"]


def _measure(name):
    out = [_restatement_ratios(name, N) for N in ac.ENV_COUNTS + (EXTRA_N,)]
    e, kg, kj, tight = (np.concatenate([o[i] for o in out]) for i in range(4))
    return e[tight], kg[tight], kj[tight]


def _quarters(kg):
    order = np.argsort(kg)
    q = len(order) // 4
    return (order[:q], "best-conditioned quarter"), (order[-q:], "worst-conditioned quarter")


@pytest.mark.parametrize("name", EE_MAPS)
def test_float32_restatement_stays_within_the_recorded_band(name):
    rows = 6 if name.endswith("pose") else 3
    e, kg, kj = _measure(name)
    assert len(e) > 2000
    k, k2 = MEASURED[rows]
    share = e / (k * kg + k2 * kj)
    assert share.max() <= 1.0, (name, share.max())
    # the band (4 x the recorded pair) is nowhere more than 20 x loose: in the best- and the worst-conditioned quarter
    # of the cases the restatement's largest error is between 0.05 and 0.25 of it
    for part, what in _quarters(kg):
        assert 0.05 <= share[part].max() / 4.0 <= 0.25, (name, what, share[part].max() / 4.0)


@pytest.mark.parametrize("N", ac.ENV_COUNTS)
@pytest.mark.parametrize("name", list(ac.MAPS))
def test_torch_controllers_match_reference(name, N):
    env = _make(name, N, "f32")
    base = env.unwrapped
    spec = base.agent.controller.fused_action_spec()
    assert spec is not None
    A, lim, rest, root0 = ac.tables(base)
    C = ac.build(name, spec, lim, rest, root0, N)
    ac.write_state(base, C)
    R = ac.reference(spec, A, C)
    base.agent.set_action(torch.from_numpy(C["action"]))
    px = base.scene.px
    tq, tv = px.cuda_articulation_target_qpos.torch().numpy().copy(), px.cuda_articulation_target_qvel.torch().numpy().copy()
    env.close()
    ac.compare(spec, C, R, tq, tv, band_k(spec), f"torch path {name} N={N}")
    ac.twins_agree(spec, C, R, tq, band_k(spec), f"torch path {name} N={N}")


@pytest.mark.parametrize("name", list(ac.MAPS) + list(ac.HAND_MAPS))
def test_case_tables_hold_their_conditions(name):
    env = _make(name, 4, "f32")
    base = env.unwrapped
    spec = ac.HAND_MAPS[name] if name in ac.HAND_MAPS else base.agent.controller.fused_action_spec()
    A, lim, rest, root0 = ac.tables(base)
    assert len(spec[0]) == base.scene.model.n_dof
    env.close()
    for N in ac.ENV_COUNTS:
        C = ac.build(name, spec, lim, rest, root0, N)
        C2 = ac.build(name, spec, lim, rest, root0, N)
        assert all(np.array_equal(C[k], C2[k], equal_nan=True) for k in ("qpos", "root", "action")), "cases are not deterministic"
        assert len(C["labels"]) == N and np.isfinite(C["action"]).all()
        R = ac.reference(spec, A, C)
        assert np.isfinite(R["tq"]).all() and np.isfinite(R["tv"]).all()
        if spec[4] is not None:
            rows = spec[4][2]
            for ps in ac.POSE_SETS:
                sel = C["pose_set"] == ps
                if not sel.any() or (rows == 6 and ps == "uniform"):
                    continue
                out = (R["kappa"][sel] > ref.KAPPA_CAP).mean()
                assert out <= 0.01, (name, N, ps, out)
            assert (~ac.tight(spec, C, R)).mean() <= (0.30 if rows == 6 else 0.01)
        # twins: same joints and action, another root pose
        i = np.arange(N)
        k = i - i % 3
        assert np.array_equal(C["qpos"], C["qpos"][k]) and np.array_equal(C["action"], C["action"][k])
        if N >= 3:
            assert not np.array_equal(C["root"][1], C["root"][0]) and abs(C["root"][2, 3]) < 0.9999
        NF = ac.build(name, spec, lim, rest, root0, N, nonfinite=True)
        assert np.isnan(NF["action"][N - 1]).any() and np.isfinite(NF["action"][: N - 1]).all()
    # N = 128: every value, every arm pose set, every rotation, every yaw is there, in every column
    C = ac.build(name, spec, lim, rest, root0, 128)
    a = C["action"].astype(np.float64)
    normalised = [c for c in range(a.shape[1]) if c not in {spec[0][j] for j in range(len(spec[0])) if not (spec[3][j] & 2)}]
    if spec[4] is None:
        for c in normalised:
            for v in (-1.0, 1.0, 1.5, -1.5, 1e6, -1e6, float(np.float32(1 + 1e-3)), float(np.float32(1 - 1e-3)), ac.TINY):
                assert (a[:, c] == v).any(), (name, c, v)
            assert (np.signbit(a[:, c]) & (a[:, c] == 0)).any()
    else:
        nr = np.linalg.norm(a[:, spec[4][1] + 3 : spec[4][1] + 6], axis=1) if spec[4][2] == 6 else None
        assert (a[:, spec[4][1] : spec[4][1] + 3] == 0).all(1).any() and (np.abs(a[:, spec[4][1] : spec[4][1] + 3]) >= 1).all(1).any()
        if nr is not None:
            assert (nr == 0).any() and (nr == 1).any() and ((nr > 1) & (nr < 1.002)).any() and ((nr < 1) & (nr > 0.998)).any() and (nr > 9.99).any()
    assert set(C["pose_set"]) == set(ac.POSE_SETS)
    if name.startswith("fetch"):
        yaw = C["qpos"][:, 2].astype(np.float64)
        for v in (0.0, 100.0, -100.0, float(np.float32(np.pi)), float(np.float32(np.pi / 2)), float(np.float32(-np.pi / 2))):
            assert (yaw == v).any(), v
        f = a[:, spec[0][0]]
        assert (f == 0).any() and (f == 1.5).any()


if __name__ == "__main__":
    for name in EE_MAPS:
        rows = 6 if name.endswith("pose") else 3
        e, kg, kj = _measure(name)
        k, k2 = MEASURED[rows]
        share = e / (k * kg + k2 * kj)
        print(f"{name}: {len(e)} cases in the tight comparison, kappa_2(G) {kg.min():.3g} .. {kg.max():.3g}, kappa_2(J) {kj.min():.3g} .. {kj.max():.3g}; "
              f"largest err / (2^-23 kappa_2(G) |dq|) {(e / kg).max():.4g}, / (2^-23 kappa_2(J) |dq|) {(e / kj).max():.4g}; "
              f"share of the recorded band (K, K2) = {MEASURED[rows]}: {share.max():.3f}, " + ", ".join(f"{what} {share[part].max():.3f}" for part, what in _quarters(kg)))
        for N in ac.ENV_COUNTS + (EXTRA_N,):
            _, g, _, t = _restatement_ratios(name, N)
            print(f"   N={N}: kappa_2(G) above the cap in {(g > ref.KAPPA_CAP).sum()} envs of {N}")
