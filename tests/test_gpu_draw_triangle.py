"""DrawTriangle-v1 on the HIP backend: the native epilogue k_task_draw against the float64 reference (tests/draw_reference.py)
over the scripts of tests/draw_cases.py, step by step through the stand-alone launch form (k_task_draw<false>), then once
through the form that first copies the state out (k_task_draw<true>; the task never runs at the control-step kernel's tail), at
env counts 128 and the ragged 1, 17, 67; the refusals; every env.step against the torch path (MS_FUSED=0) on the same state with
a partial reset on the way; the same seed twice; and a scripted episode that draws.

`success`, `dot_near`, `ref_hit` and the counters equal the reference's on every env, none left out; `dots` and the copied
observation floats are bit-exact, `tcp_to_verts_pos` is the float32 difference bit for bit, and it and `vertices` lie within
4 x the torch path's measured difference to float64 corners (tests/draw_cases.py: 4 x 4.6e-8 = 1.84e-7). Every written buffer
carries 8 guard rows on either side that must stay as they were."""
import numpy as np
import pytest
import torch

from tests import draw_cases as dc
from tests import draw_reference as ref

pytestmark = pytest.mark.gpu
BACKEND = "physx_cuda"
GUARD = 8
FILL = {torch.float32: -77.0, torch.uint8: 0xAB, torch.int8: 0x5A, torch.int32: -7777, torch.bool: True}
# the robot of PushT's start: the stick's tip 24 mm above the table, 4 mm above the canvas
LOW_QPOS = np.array([0.662, 0.212, 0.086, -2.685, -0.115, 2.898, 1.673])


class Guarded:
    """a tensor of N rows with GUARD rows before and after it, filled with a value the kernel never writes"""

    def __init__(self, N, tail, dtype, dev, init):
        self.N, self.fill = N, FILL[dtype]
        self.all = torch.full((N + 2 * GUARD,) + tail, self.fill, dtype=dtype, device=dev)
        self.t = self.all[GUARD:GUARD + N]
        if init is not None:
            self.t[:] = init

    def intact(self):
        return bool((self.all[:GUARD] == self.fill).all()) and bool((self.all[GUARD + self.N:] == self.fill).all())


def _buffers(base, N):
    dev, D = base.device, 2 * base.agent.robot.max_dof + dc.OBS_EXTRA
    return dict(obs=Guarded(N, (D,), torch.float32, dev, None), reward=Guarded(N, (), torch.float32, dev, None), flags=Guarded(N, (1,), torch.uint8, dev, None),
                dots=Guarded(N, (ref.MAX_DOTS, 2), torch.float32, dev, 0.0), dot_near=Guarded(N, (ref.MAX_DOTS,), torch.int8, dev, -1),
                ref_hit=Guarded(N, (ref.N_REF,), torch.bool, dev, False), draw_step=Guarded(N, (), torch.int32, dev, 0))


def _task(base, G, update=1):
    from maniskill_amd import native

    return native.DrawTask(tcp_row=int(base.agent.tcp._body_row), goal_row=int(base.goal_tri._body_row), vertices=base.vertices.data_ptr(),
                           triangles=base.triangles.data_ptr(), dots=G["dots"].t.data_ptr(), dot_near=G["dot_near"].t.data_ptr(), ref_hit=G["ref_hit"].t.data_ptr(),
                           draw_step=G["draw_step"].t.data_ptr(), max_dots=ref.MAX_DOTS, n_ref=ref.N_REF, z_thresh=base.z_thresh, near_thresh2=base.near_thresh2,
                           update=update, reward_scale=1.0)


def _call(base, G, task):
    base.scene.px.task_draw_outputs(task, G["obs"].t, G["reward"].t, G["flags"].t)


def _tables(G):
    return {k: G[k].t.cpu().numpy().copy() for k in ("dots", "dot_near", "ref_hit", "draw_step")}


def _outputs_ok(G, what):
    for k, g in G.items():
        assert g.intact(), (what, k, "guard rows written")
    fl = G["flags"].t.cpu().numpy()
    assert ((fl == 0) | (fl == 1)).all(), what
    assert np.array_equal(G["reward"].t.cpu().numpy(), fl[:, 0].astype(np.float32)), (what, "reward = success")
    return fl[:, 0].astype(bool)


@pytest.mark.parametrize("N", [128, 1, 17, 67])
def test_epilogue_runs_the_scripts_as_the_reference(N, monkeypatch):
    monkeypatch.setenv("MS_FUSED", "1")
    env = dc.make_env(N, BACKEND)
    base = env.unwrapped
    px = base.scene.px
    base.scene._gpu_fetch_all()
    S = dc.snapshot(base)
    P, labels = dc.build_scripts(S["vertices"], S["triangles"])
    dc.check_margins(P, S["triangles"])
    succ, cnt, tables = dc.reference_run(P, S["triangles"])
    dc.expected_story(succ, labels)
    if N >= 17:
        assert set(labels) == set(dc.LABELS)
    # ---- the stand-alone form, step by step
    G = _buffers(base, N)
    task = _task(base, G)
    rows, Pd = dc.tcp_rows(base), torch.from_numpy(P).to(base.device)
    got_succ, got_cnt, worst = [], [], 0.0
    for t in range(dc.STEPS):
        rows[:, :3] = Pd[t]
        _call(base, G, task)
        got_succ.append(G["flags"].t[:, 0].clone())
        got_cnt.append(G["draw_step"].t.clone())
        if t in tables:
            torch.cuda.synchronize()
            _outputs_ok(G, f"N={N} step {t}")
            dc.check_tables(_tables(G), tables[t], f"k_task_draw<false> N={N} step {t}")
            St = dc.snapshot(base)
            worst = max(worst, dc.check_obs(G["obs"].t.cpu().numpy(), *dc.obs_inputs(St, base), f"N={N} step {t}"))
    torch.cuda.synchronize()
    got_succ, got_cnt = torch.stack(got_succ).cpu().numpy().astype(bool), torch.stack(got_cnt).cpu().numpy()
    bad = np.argwhere(got_succ != succ)
    assert bad.size == 0, ("success", [(int(t), labels[e]) for t, e in bad[:6]])
    assert np.array_equal(got_cnt, cnt) and got_cnt.max() == ref.MAX_DOTS, "the counter stops at the table's end"
    print(f"DrawTriangle N={N} stand-alone: max |kernel - f64| over vertices / tcp_to_verts_pos {worst:.3e} (tolerance {dc.tolerance():.3e})")
    assert worst <= dc.tolerance()
    if N > dc.NAN_CASE:  # the NaN tcp drew nothing, succeeded never, and its neighbours are the reference's
        e = dc.NAN_CASE
        assert labels[e] == "nan tcp" and not got_succ[:, e].any() and bool((G["dot_near"].t[e] == -1).all()) and not bool(G["ref_hit"].t[e].any())
    # a reset's outputs (update = 0) read the tables and write none of them
    before = _tables(G)
    _call(base, G, _task(base, G, update=0))
    torch.cuda.synchronize()
    assert np.array_equal(_outputs_ok(G, "update=0"), succ[-1])
    after = _tables(G)
    assert all(np.array_equal(before[k], after[k]) for k in before)

    # ---- the copy-out form: the robot's joints put the tip near the canvas in some envs and above it in others; the launch
    # refills the stale buffers, appends one dot and evaluates. The reference runs on what the launch copied out, and the
    # stand-alone form on those buffers gives the same bits.
    g = np.random.RandomState(11)
    q = LOW_QPOS + g.normal(0, 0.02, (N, 7))
    q[::2, 1] -= 0.05  # (every other arm a little more upright: its tip some 2 cm higher)
    base.agent.robot.set_qpos(torch.from_numpy(q.astype(np.float32)).to(base.device))
    base.scene._gpu_apply_all()
    px.gpu_update_articulation_kinematics()
    px.cuda_rigid_body_data.torch()[:] = 5.0  # (stale: the launch has to refill the buffers)
    t0 = px.tail_step_count()
    px.defer_fetch_all()
    G1 = _buffers(base, N)
    _call(base, G1, _task(base, G1))
    torch.cuda.synchronize()
    assert px.tail_step_count() == t0
    s1 = _outputs_ok(G1, f"N={N} copy-out")
    S1 = dc.snapshot(base)
    assert not np.any(S1["rigid"][int(base.agent.tcp._body_row), :, :3] == 5.0), "the copy-out did not run"
    tcp = S1["rigid"][int(base.agent.tcp._body_row), :, :3]
    st = ref.append(ref.new_state(N), tcp, S1["triangles"])
    dz, dd = ref.margins(tcp, S1["triangles"])
    clear = (np.abs(dz) > 1e-6) & ((dz > 0) | (np.abs(dd).min(1) > 1e-6))
    assert clear.all(), "the seeded joints leave no env on a decision's edge: every env is judged"
    T1 = _tables(G1)
    for k in ("dot_near", "ref_hit", "draw_step"):
        assert np.array_equal(T1[k][clear].astype(st[k].dtype), st[k][clear]), k
    assert np.array_equal(T1["dots"][clear].view(np.uint32), st["dots"][clear].astype(np.float32).view(np.uint32))
    assert np.array_equal(s1[clear], ref.success(st)[clear])
    d = dc.check_obs(G1["obs"].t.cpu().numpy(), *dc.obs_inputs(S1, base), f"N={N} copy-out")
    assert d <= dc.tolerance()
    drawn = st["dot_near"][:, 0] > -1
    if N >= 17:
        assert drawn.any() and (~drawn).any(), "the copy-out batch has tips on both sides of the z threshold"
    G2 = _buffers(base, N)
    _call(base, G2, _task(base, G2))
    torch.cuda.synchronize()
    _outputs_ok(G2, f"N={N} stand-alone after the copy-out")
    for k in G1:
        a, b = G1[k].t.cpu().numpy(), G2[k].t.cpu().numpy()
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (k, "differs between the two launch forms")
    assert px.overflow_count() == 0
    env.close()


def test_refusals_launch_nothing(monkeypatch):
    from maniskill_amd import native

    monkeypatch.setenv("MS_FUSED", "1")
    env = dc.make_env(4, BACKEND)
    base = env.unwrapped
    px = base.scene.px
    G = _buffers(base, 4)
    args = (G["obs"].t, G["reward"].t, G["flags"].t)

    def task(**kw):
        t = _task(base, G)
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    for row in (-1, base.scene.model.n_rows):
        with pytest.raises(native.NativeError, match=r"\(1\).*body row out of range"):
            px.task_draw_outputs(task(tcp_row=row), *args)
    for kw in (dict(dots=None), dict(dot_near=None), dict(ref_hit=None), dict(draw_step=None), dict(vertices=None), dict(triangles=None), dict(max_dots=0),
               dict(max_dots=298), dict(n_ref=0), dict(dot_near=G["dot_near"].t.data_ptr() + 1)):
        with pytest.raises(native.NativeError, match=r"\(3\).*task_draw_outputs"):
            px.task_draw_outputs(task(**kw), *args)
    torch.cuda.synchronize()
    for k in ("obs", "reward", "flags"):
        assert bool((G[k].all == G[k].fill).all()), k
    assert bool((G["draw_step"].t == 0).all()) and bool((G["dot_near"].t == -1).all())
    env.close()


# ---------------------------------------------------------------------------------------------------------------------
ENV_N, ENV_STEPS, RESET_AT = 64, 25, 10
RESET_IDX = (1, 5, 40, ENV_N - 1)
TABLES = ("dots", "dot_near", "ref_hit", "draw_step")


def _actions(N, steps):
    """uniform random joint-delta actions; the shoulder and elbow columns are folded to one sign so that the arms come down
    to the canvas within the run"""
    g = torch.Generator().manual_seed(3)
    acts = [2 * torch.rand(N, 7, generator=g) - 1 for _ in range(steps)]
    for a in acts:
        a[:, 1] = a[:, 1].abs()
        a[:, 3] = a[:, 3].abs()
    return acts


def _env_tables(base):
    return {k: getattr(base, k).cpu().clone() for k in TABLES}


def _rollout(monkeypatch, fused, N=ENV_N, steps=ENV_STEPS, reset_at=RESET_AT, compare=False, reset_idx=None, reset_seed=None, **kw):
    """a seeded run with a partial reset after step `reset_at`. -> per step (obs, reward, terminated, truncated, elapsed,
    success, tables). compare: after every native step the tables are put back, the torch path appends its dot and computes
    its outputs on the very same state, and the two must be equal"""
    import maniskill_amd.envs  # noqa: F401
    import gymnasium as gym

    acts = _actions(N, steps)
    monkeypatch.setenv("MS_FUSED", fused)
    env = gym.make(dc.ENV_ID, num_envs=N, sim_backend=BACKEND, **kw)
    base = env.unwrapped
    assert base._use_fused_callers == (fused == "1")
    obs, info = env.reset(seed=5)
    if fused == "1":
        assert base._fused_ok() and base._fused_action_ready(acts[0].cuda()), "native action map / epilogue not in use"
    px = base.scene.px
    tail0 = px.tail_step_count()
    px.overflow_count()
    z = torch.zeros(N)
    traj = [(obs.cpu().clone(), z, z.bool(), z.bool(), info["elapsed_steps"].cpu().clone(), info["success"].cpu().clone(), _env_tables(base))]

    def same_state(o, s, before):
        after = _env_tables(base)
        if before is not None:
            for k in TABLES:
                getattr(base, k).copy_(before[k].to(base.device))
            base._append_dot()
        mine = _env_tables(base)
        for k in TABLES:
            assert torch.equal(mine[k], after[k]), (k, "the torch path's table differs on the same state")
        ti = base.get_info()
        to = base.get_obs(ti)
        assert torch.equal(to.cpu().view(torch.int32), o.cpu().view(torch.int32)), float((to.cpu() - o.cpu()).abs().max())
        assert torch.equal(ti["success"].cpu(), s.cpu())

    if compare:
        same_state(obs, info["success"], None)
    for i, a in enumerate(acts):
        before = _env_tables(base)
        obs, rew, term, trunc, info = env.step(a.cuda())
        if compare:
            same_state(obs, info["success"], before)
        traj.append((obs.cpu().clone(), rew.cpu().clone().float(), term.cpu().clone(), trunc.cpu().clone(), info["elapsed_steps"].cpu().clone(),
                     info["success"].cpu().clone(), _env_tables(base)))
        if i + 1 == reset_at:
            assert max(RESET_IDX) < N or reset_idx is not None, "a partial reset names envs of this batch only"
            obs, info = env.reset(seed=reset_seed, options=dict(env_idx=torch.tensor(RESET_IDX if reset_idx is None else reset_idx, device=base.device)))
            if compare:
                same_state(obs, info["success"], None)
            traj.append((obs.cpu().clone(), z, z.bool(), z.bool(), info["elapsed_steps"].cpu().clone(), info["success"].cpu().clone(), _env_tables(base)))
    tail, overflow = px.tail_step_count() - tail0, px.overflow_count()
    model = base.scene.model
    env.close()
    return traj, tail, overflow, (int(model.n_dof), int(model.n_free))


def test_env_with_epilogue_matches_torch_path(monkeypatch):
    """64 envs, 25 random-action control steps, a partial reset after the 10th: env.step with the native epilogue (the plain
    one-row control step k_solve16<7, 0, false, 1> + k_task_draw<true>, two launches) against what the MS_FUSED=0 step
    computes on that very state (`_append_dot` on the tables as they were before the step, get_info, get_obs): the dot tables
    equal, observations bit for bit, success equal. The separate MS_FUSED=0 run is compared where two runs can be (the
    physics of the two differ in the last bits, tests/test_gpu_place_tool.py explains why): the step counters, `truncated`
    and the dot counters at every step."""
    fused, tail, overflow, (n_dof, n_free) = _rollout(monkeypatch, "1", compare=True)
    plain, tail_t, _, _ = _rollout(monkeypatch, "0")
    assert tail == 0 and tail_t == 0, "DrawTriangle never takes the control-step kernel's tail"
    assert overflow == 0 and (n_dof, n_free) == (7, 0)
    assert len(fused) == len(plain) == ENV_STEPS + 2
    want = torch.zeros(ENV_N, dtype=torch.int64)
    for step, (a, b) in enumerate(zip(fused, plain)):
        if step == RESET_AT + 1:
            want[list(RESET_IDX)] = 0  # (the reset envs' counters are at zero, the others untouched)
        elif step > 0:
            want += 1
        for run in (a, b):
            assert torch.equal(run[4].long(), want) and torch.equal(run[6]["draw_step"].long(), want), step
            assert run[3].dtype == torch.bool and not run[3].any(), step
            assert torch.equal(run[2], run[5]), step
            assert torch.equal(run[1] != 0, run[5]), (step, "the sparse reward is success")
    drawn = int((fused[-1][6]["dot_near"] > -1).sum()), int((plain[-1][6]["dot_near"] > -1).sum())
    print(f"DrawTriangle-v1 rollout: dots drawn by the end, native / MS_FUSED=0: {drawn}; obs after the first step "
          f"{float((fused[1][0] - plain[1][0]).abs().max()):.3e}")
    assert drawn[0] > 0 and drawn[1] > 0, "no arm reached the canvas: the comparison saw empty tables only"
    assert torch.allclose(fused[1][0], plain[1][0], atol=1e-5)


def test_truncation_at_the_time_limit(monkeypatch):
    traj, tail, _, _ = _rollout(monkeypatch, "1", N=2, steps=6, reset_at=-1, max_episode_steps=5)
    plain, _, _, _ = _rollout(monkeypatch, "0", N=2, steps=6, reset_at=-1, max_episode_steps=5)
    assert all(torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]) for a, b in zip(traj, plain))
    assert not traj[4][3].any() and traj[5][3].all() and traj[6][3].all() and tail == 0


def test_same_seed_same_episode(monkeypatch):
    a, _, overflow_a, _ = _rollout(monkeypatch, "1", N=32, steps=20, reset_idx=(1, 5, 31), reset_seed=9)  # (an unseeded reset draws from the ambient stream)
    b, _, overflow_b, _ = _rollout(monkeypatch, "1", N=32, steps=20, reset_idx=(1, 5, 31), reset_seed=9)
    assert overflow_a == 0 and overflow_b == 0
    for step, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x[0].view(torch.int32), y[0].view(torch.int32)), step
        assert torch.equal(x[5], y[5]) and all(torch.equal(x[6][k], y[6][k]) for k in TABLES), step


def test_a_scripted_episode_draws_under_the_tip(monkeypatch):
    """pd_ee_delta_pos: the stick comes down, then moves along +y with a light downward command (on the float32 oracle this script draws 48 dots per env). Every env draws, and every
    drawn dot lies within BRUSH_RADIUS + 5 mm of the tcp's xy at its step"""
    import maniskill_amd.envs  # noqa: F401
    import gymnasium as gym

    monkeypatch.setenv("MS_FUSED", "1")
    N, steps = 4, 60
    env = gym.make(dc.ENV_ID, num_envs=N, sim_backend=BACKEND, control_mode="pd_ee_delta_pos")
    base = env.unwrapped
    env.reset(seed=2)
    base.scene.px.overflow_count()
    tcp = []
    for t in range(steps):
        a = torch.zeros(N, 3, device=base.device)
        if t < 12:
            a[:, 2] = -0.5  # (a target 5 cm below the tip at every step: the tip reaches the canvas within 6 steps)
        else:
            a[:, 1], a[:, 2] = 0.05, -0.2
        env.step(a)
        tcp.append(base.agent.tcp.pose.p.cpu().clone())
    tcp = torch.stack(tcp, 1)  # [N, steps, 3]
    near, dots = base.dot_near.cpu()[:, :steps], base.dots.cpu()[:, :steps]
    drawn = near > -1
    print(f"scripted episode: dots drawn per env {drawn.sum(1).tolist()}, lowest tip {float(tcp[..., 2].min()):.4f} m")
    assert torch.all(base.draw_step.cpu() == steps) and torch.all(drawn.sum(1) >= 1)
    assert torch.equal(drawn, tcp[..., 2] < base.z_thresh)
    off = torch.linalg.norm(dots - tcp[..., :2], dim=-1)
    assert float(off[drawn].max()) <= ref.BRUSH_RADIUS + 0.005
    assert base.scene.px.overflow_count() == 0
    env.close()
