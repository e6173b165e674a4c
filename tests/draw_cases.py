"""Scripted tcp positions for the DrawTriangle epilogue, one script per env index (the table repeats over the batch): what
the stick's tip does at each of STEPS control steps, written straight into the tcp link's pose row (nothing is stepped) and
driven through the stand-alone launch form, step by step. Shared by tests/test_draw_triangle.py (the torch path on the
oracle backend) and tests/test_gpu_draw_triangle.py (k_task_draw), both against tests/draw_reference.py.

Margins. Positions are float32 (about 1e-7 m at these magnitudes, and the float32 squared distance at 25 mm is good to about
3e-9 m), so a case meant to lie on one side of the z threshold or of THRESHOLD sits EDGE = 1e-5 m from it; `check_margins`
asserts, from the float32 inputs and in float64, that NO step of NO script comes closer than EDGE / 2 to either decision.

Observation tolerance. qpos, qvel, the two poses and goal_pos are copies: bit-exact. `vertices` and `tcp_to_verts_pos`
are float32 here where the reference implementation keeps float64 corners; the torch path's own difference to the float64
statement (corners from the goal's pose row in float64), measured on the CPU over 128, 67, 17 and 1 envs at seed 7 after two seeded random steps
(tests/test_draw_triangle.py::test_torch_path_matches_reference prints it and asserts that the band still bounds it):

    vertices          max |torch f32 - f64| = 4.13e-8 m
    tcp_to_verts_pos  max |torch f32 - f64| = 4.51e-8 m

MEASURED is that band, 4.6e-8; the native epilogue's two blocks are held to 4 x MEASURED = 1.84e-7, the project's rule, and
are bit for bit the torch path's (the same float32 subtraction)."""
import numpy as np
import torch

from tests import draw_reference as ref

f32 = np.float32
ENV_ID = "DrawTriangle-v1"
OBS_EXTRA = 35
EDGE = 1e-5
MEASURED = 4.6e-8
STEPS = ref.MAX_DOTS + 3  # a whole table and three calls after it
HIGH = 0.1  # a raised tip
NAN_CASE = 5
LABELS = ["never touches", "z just below the threshold, on a corner", "z just above the threshold", "just inside THRESHOLD", "just outside THRESHOLD",
          "nan tcp", "between two reference points", "outline completed at step 299", "outline with one stray dot", "corner dot, then nothing"]
# the full tables are compared after these steps (success and the counter after every step)
TABLE_STEPS = (0, 1, 2, 150, 151, 298, 299, 300, 301, 302)


def tolerance():
    return 4 * MEASURED


def make_env(N, backend, seed=7, **kw):
    import maniskill_amd.envs  # noqa: F401  (registers the task; installs the gymnasium stand-in when gymnasium is absent)
    import gymnasium as gym

    env = gym.make(ENV_ID, num_envs=N, sim_backend=backend, **kw)
    env.reset(seed=seed)
    return env


def _outline(verts, s):
    """the point at arc length s (metres, from corner 0 along edge 0, 1, 2) of the outline"""
    s = s % (3 * ref.EDGE)
    i = int(s // ref.EDGE)
    t = (s - i * ref.EDGE) / ref.EDGE
    return verts[i] * (1 - t) + verts[(i + 1) % 3] * t


def script(case, verts, tris):
    """[STEPS, 3] float64 tcp positions of one env; verts [3, 2] and tris [153, 2] are the env's own (float32 values)"""
    verts, tris = np.asarray(verts, np.float64), np.asarray(tris, np.float64)
    centre = verts.mean(0)
    out_of = lambda p: (p - centre) / np.linalg.norm(p - centre)  # (unit vector away from the centre)
    P = np.zeros((STEPS, 3))
    P[:, :2] = centre
    P[:, 2] = HIGH
    low = 0.024
    if case == 1:
        P[0] = [*verts[0], ref.Z_THRESH - EDGE]
    elif case == 2:
        P[0] = [*verts[0], ref.Z_THRESH + EDGE]
    elif case in (3, 4):  # beyond corner 0, away from the centre: corner 0 is the nearest reference point by far
        d = ref.THRESHOLD + (-EDGE if case == 3 else EDGE)
        P[0] = [*(tris[0] + d * out_of(tris[0])), low]
    elif case == NAN_CASE:
        P[:] = np.nan
    elif case == 6:
        P[0] = [*(0.5 * (tris[10] + tris[11])), low]
    elif case in (7, 8):
        # dots 0..286 run at half the reference points' spacing h from 10 h past corner 0 to 10 h short of it (29.4 mm): every
        # reference point but corner 0 itself gets a dot within 8 h = 23.5 mm, and every dot-to-point distance is
        # h sqrt(m^2 + n^2 - m n) for integers m, n -- 24.96 or 25.13 mm at the closest to THRESHOLD. Dots 287..298 stay
        # raised; dot 299 on corner 0 completes the outline. Then three calls past the table, low and far away
        h = ref.EDGE / 102
        for k in range(287):
            P[k] = [*_outline(verts, (10 + k) * h), low]
        if case == 8:  # 30 mm off the middle of edge 1, outwards
            mid = 0.5 * (verts[1] + verts[2])
            P[150] = [*(mid + 0.030 * out_of(mid)), low]
        P[ref.MAX_DOTS - 1] = [*verts[0], low]
        P[ref.MAX_DOTS:] = [*(centre + 0.2 * out_of(verts[0])), low]
    elif case == 9:
        P[0] = [*verts[0], low]
        P[ref.MAX_DOTS:] = [*(centre + 0.2 * out_of(verts[0])), low]
    return P


def build_scripts(vertices, triangles):
    """env e takes script e mod len(LABELS), built on ITS triangle; the NaN script goes to env NAN_CASE alone (its repeats
    never touch). -> (P [STEPS, N, 3] float32, labels)"""
    N = len(vertices)
    P, labels = np.zeros((STEPS, N, 3), dtype=f32), []
    for e in range(N):
        case = e % len(LABELS)
        if case == NAN_CASE and e != NAN_CASE:
            case = 0
        labels.append(LABELS[case])
        P[:, e] = script(case, vertices[e, :, :2], triangles[e]).astype(f32)
    return P, labels


def check_margins(P, triangles):
    """no step of no script lies closer than EDGE / 2 to the z threshold or to THRESHOLD from any reference point"""
    for t in range(len(P)):
        ok = ~np.isnan(P[t]).any(1)
        dz, dd = ref.margins(P[t][ok], triangles[ok])
        assert np.abs(dz).min() >= EDGE / 2, (t, np.abs(dz).min())
        low = dz < 0
        if low.any():
            assert np.abs(dd[low]).min() >= EDGE / 2, (t, np.abs(dd[low]).min())


def reference_run(P, triangles, table_steps=TABLE_STEPS):
    """the float64 reference over the scripts -> (success [STEPS, N], draw_step [STEPS, N], {step: copy of the tables})"""
    N = P.shape[1]
    st = ref.new_state(N)
    succ, cnt, tables = [], [], {}
    for t in range(len(P)):
        ref.append(st, P[t], triangles)
        succ.append(ref.success(st))
        cnt.append(st["draw_step"].copy())
        if t in table_steps:
            tables[t] = {k: v.copy() for k, v in st.items()}
    return np.array(succ), np.array(cnt), tables


def expected_story(succ, labels):
    """what the scripts are for, stated on the reference's own answers: who succeeds when"""
    last = ref.MAX_DOTS - 1
    for e, label in enumerate(labels):
        if label == "outline completed at step 299":
            assert not succ[:last, e].any() and succ[last:, e].all(), label  # (the calls after step 299 change nothing)
        else:
            assert not succ[:, e].any(), label


def check_tables(got, want, what):
    """the dot tables against the reference's: dot_near, ref_hit and the counter equal on every env, dots bit-exact"""
    assert np.array_equal(got["draw_step"].astype(np.int64), want["draw_step"]), (what, "draw_step")
    assert np.array_equal(got["dot_near"], want["dot_near"]), (what, "dot_near", np.argwhere(got["dot_near"] != want["dot_near"])[:4])
    assert np.array_equal(got["ref_hit"].astype(bool), want["ref_hit"]), (what, "ref_hit", np.argwhere(got["ref_hit"].astype(bool) != want["ref_hit"])[:4])
    assert got["dots"].dtype == f32 and np.array_equal(got["dots"].view(np.uint32), want["dots"].astype(f32).view(np.uint32)), (what, "dots")


def check_obs(got, qpos, qvel, tcp_pose, goal_pose, vertices, what):
    """one observation [N, 2 n + 35] f32 against the float64 statement on the float32 inputs: the copies bit for bit (a NaN
    matches a NaN), tcp_to_verts_pos the float32 difference bit for bit and, like vertices, within the tolerance of float64.
    -> max |got - f64| over the two blocks"""
    n = qpos.shape[1]
    want = ref.observation(qpos, qvel, tcp_pose, goal_pose, vertices)
    assert got.dtype == f32 and got.shape == want.shape, (what, got.shape, want.shape)
    w32 = want.astype(f32)
    w32[:, 2 * n + 14:2 * n + 23] = (np.asarray(vertices, f32).reshape(-1, 3, 3) - np.asarray(tcp_pose, f32)[:, None, :3]).reshape(-1, 9)
    same = (got.view(np.uint32) == w32.view(np.uint32)) | (np.isnan(got) & np.isnan(w32))
    assert same.all(), (what, "obs", np.argwhere(~same)[:4])
    blocks = np.r_[2 * n + 14:2 * n + 23, 2 * n + 26:2 * n + 35]
    d = np.abs(got[:, blocks].astype(np.float64) - want[:, blocks])
    return float(np.nanmax(d)) if d.size else 0.0


# ---- the env's buffers ----------------------------------------------------------------------------------------------------
def snapshot(base):
    """what the epilogue reads, as numpy float32"""
    px, N = base.scene.px, base.num_envs
    return dict(rigid=px.cuda_rigid_body_data.torch().cpu().numpy().reshape(-1, N, 13).copy(), qpos=px.cuda_articulation_qpos.torch().cpu().numpy().copy(),
                qvel=px.cuda_articulation_qvel.torch().cpu().numpy().copy(), vertices=base.vertices.cpu().numpy().copy(), triangles=base.triangles.cpu().numpy().copy())


def tcp_rows(base):
    """the tcp link's pose rows [N, 13] of the user-visible buffer, a view: what a script step is written into"""
    N, row = base.num_envs, int(base.agent.tcp._body_row)
    return base.scene.px.cuda_rigid_body_data.torch()[row * N:(row + 1) * N]


def env_tables(base):
    return dict(dots=base.dots.cpu().numpy().copy(), dot_near=base.dot_near.cpu().numpy().copy(), ref_hit=base.ref_hit.cpu().numpy().copy(),
                draw_step=base.draw_step.cpu().numpy().copy())


def obs_inputs(S, base):
    """(qpos, qvel, tcp_pose, goal_pose, vertices) of snapshot S for `check_obs`"""
    return S["qpos"], S["qvel"], S["rigid"][int(base.agent.tcp._body_row), :, :7], S["rigid"][int(base.goal_tri._body_row), :, :7], S["vertices"]
