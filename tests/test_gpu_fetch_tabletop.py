"""The table-top tasks with the Fetch on the HIP backend: dispatch (the native epilogue, no tail, the two-row 15-dof plain
step), the six robot-dependent epilogues against the float64 reference (tests/fetch_task_reference.py) on constructed states
in their two launch forms (k_task_*<false>, and k_task_*<true>, which first copies the state out) at env counts 128 and the
ragged 1, 17, 67, every env.step against the torch path on the same state, the robot profile being inert for a Panda, and
the three cameras of a camera obs mode.

Constructed states (tests/fetch_task_cases.py): the object is teleported between the Fetch's fingers and squeezed in the
even envs, the gripper stays open in the odd ones; the body that makes the robot's is_static matter comes to the object in
two envs of three; the joint velocities are overwritten from a table that puts both thresholds of Fetch.is_static on both
sides, the signed comparison included; nothing is stepped after that. Flags equal the reference's, observation entries
are bit-exact, rewards agree within 4 x MEASURED_TORCH[task], the torch path's own largest difference from the reference on
the same states, as measured on an MI355X (each test prints both figures). Output tensors carry 8 guard rows that must stay
as they were."""
import numpy as np
import pytest
import torch

from tests import fetch_task_cases as fc
from tests import fetch_task_reference as fr

pytestmark = pytest.mark.gpu
BACKEND = "physx_cuda"
GUARD = 8

# max |torch f32 path - f64 reference| of the dense reward over the constructed states of every N, both forms, measured on
# an MI355X and rounded up (measured: 1.890e-7, 2.772e-7, 4.685e-7, 1.198e-7, 9.133e-7, 2.658e-7). The kernels' own figures
# on the same states: pick 2.4e-7, stack 2.8e-7, poke 4.8e-7 (its metrics included), lift 1.2e-7, place 9.2e-7, tool 2.4e-7; over
# the env rollouts the epilogues differ from the torch path on the same state by at most 2.4e-7 (rewards) and 1.2e-7 (info floats)
MEASURED_TORCH = dict(pick=1.9e-7, stack=2.8e-7, poke=4.7e-7, lift=1.2e-7, place=9.2e-7, tool=2.7e-7)
# PushCube and PullCube read nothing of the robot but its tcp: the figures of their own epilogue tests
# (tests/task_cases.py, tests/roll_pull_cases.py)
MEASURED_TORCH.update(push=1.3e-7, pull=7.2e-8)


def tolerance(task):
    return 4 * MEASURED_TORCH[task]


def _alloc(task, base, N):
    D = 2 * base.agent.robot.max_dof + fc.OBS_EXTRA[task]
    dev = base.device
    out = dict(obs=torch.full((N + GUARD, D), -77.0, device=dev), reward=torch.full((N + GUARD,), -77.0, device=dev),
               flags=torch.full((N + GUARD, len(fc.FLAG_NAMES[task])), 0xAB, dtype=torch.uint8, device=dev))
    if task in fc.N_METRICS:
        out["metrics"] = torch.full((N + GUARD, fc.N_METRICS[task]), -77.0, device=dev)
    return out


def _call(task, base, P, out):
    px = base.scene.px
    fn = dict(pick=px.task_pick_outputs, stack=px.task_stack_outputs, poke=px.task_poke_outputs, lift=px.task_liftpeg_outputs,
              place=px.task_place_outputs, tool=px.task_pulltool_outputs)[task]
    extra = (out["metrics"],) if task in fc.N_METRICS else ()
    fn(fc.native_task(task, P), out["obs"], out["reward"], out["flags"], *extra)
    torch.cuda.synchronize()


def _read(task, out, N):
    for k, t in out.items():
        assert bool((t[N:] == (0xAB if t.dtype == torch.uint8 else -77.0)).all()), (task, k, "guard rows written")
    fl = out["flags"][:N].cpu().numpy()
    assert ((fl == 0) | (fl == 1)).all()
    got = dict(obs=out["obs"][:N].cpu().numpy(), reward=out["reward"][:N].cpu().numpy(),
               flags={name: fl[:, i].astype(bool) for i, name in enumerate(fc.FLAG_NAMES[task])})
    if "metrics" in out:
        got["metrics"] = out["metrics"][:N].cpu().numpy()
    return got


def _same(task, a, b, what):
    for k in ("obs", "reward") + (("metrics",) if "metrics" in a else ()):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (what, k)
    for name in fc.FLAG_NAMES[task]:
        assert np.array_equal(a["flags"][name], b["flags"][name]), (what, name)


def run_forms(task, N, tol):
    """-> (torch path's, standalone kernel's, copy-out kernel's) largest reward difference from the reference"""
    env = fc.make_env(task, N, BACKEND, reward_mode="dense")
    base = env.unwrapped
    px = base.scene.px
    assert base._use_fused_callers and base._fused_ok()
    closed = np.arange(N) % 2 == 0
    fc.squeeze(env, task, closed)
    fc.arrange(task, base, np.arange(N) % 3 != 2)
    fc.set_fetch_profile(px)
    S = fc.snapshot(base)
    P = fc.params(task, base)
    S["qvel"], labels, static = fc.qvel_batch(N)
    what = f"{task} N={N}"
    # the standalone form, and the torch path, on the buffers as written
    base.scene._gpu_fetch_all()
    fc.write_buffers(base, S)
    R = fr.evaluate(task, S, P)
    g = R["flags"][fr.GRASP_FLAG[task]]
    assert np.array_equal(g, closed), (what, "the squeeze", g.tolist())
    if N >= 4:
        assert min(int(g.sum()), int((~g).sum())) >= N // 4
    if "fetch_static" in R["flags"]:
        assert np.array_equal(R["flags"]["fetch_static"], static)
    if N >= 67 and task in ("pick", "poke"):
        placed = R["flags"]["is_obj_placed" if task == "pick" else "is_cube_placed"]
        assert R["flags"]["success"].any() and (placed & ~static).any() and (~placed & static).any()
    if N >= 67 and task == "place":
        on = R["flags"]["is_obj_on_bin"]
        assert (on & g & static).any() and (on & g & ~static).any()
    assert all(d.all() for d in R["decided"].values()) and R["reward_decided"].all(), (what, "a case inside a predicate's band")
    d_torch = fc.compare(task, fc.torch_outputs(task, base), R, labels, np.inf, what + " torch path")
    out = _alloc(task, base, N)
    t0 = px.tail_step_count()
    _call(task, base, P, out)
    got = _read(task, out, N)
    d_alone = fc.compare(task, got, R, labels, np.inf, what + " standalone")
    if task == "poke":
        d_alone = max(d_alone, float(np.abs(got["metrics"] - R["metrics"]).max()))
    # the copy-out form: the states applied to the simulation, the copy-out owed to the call; then the standalone form on
    # the buffers that launch filled: the same outputs bit for bit
    base.scene._gpu_apply_all()
    px.gpu_update_articulation_kinematics()
    stale = {**S, "rigid": np.full_like(S["rigid"], 5.0), "qvel": np.full_like(S["qvel"], 7.0)}
    fc.write_buffers(base, stale)
    px.defer_fetch_all()
    out = _alloc(task, base, N)
    _call(task, base, P, out)
    got1 = _read(task, out, N)
    S1 = fc.snapshot(base)
    assert not np.array_equal(S1["rigid"], stale["rigid"]) and np.array_equal(S1["qvel"], S["qvel"]), "the copy-out did not run"
    R1 = fr.evaluate(task, S1, P)
    assert all(d.all() for d in R1["decided"].values())
    d_copy = fc.compare(task, got1, R1, labels, np.inf, what + " copy-out")
    out = _alloc(task, base, N)
    _call(task, base, P, out)
    _same(task, got1, _read(task, out, N), what + ": the copy-out form against the standalone form")
    assert px.tail_step_count() == t0 and px.overflow_count() == 0
    print(f"{what}: max |reward - f64 reference|: torch path {d_torch:.3e}, k_task<false> {d_alone:.3e}, k_task<true> {d_copy:.3e} (tolerance {tol:.3e})")
    fc.compare(task, got, R, labels, tol, what + " standalone")
    fc.compare(task, got1, R1, labels, tol, what + " copy-out")
    if task == "poke":
        assert float(np.abs(got["metrics"] - R["metrics"]).max()) <= tol
    env.close()
    return d_torch, d_alone, d_copy


@pytest.mark.parametrize("N", [128, 1, 17, 67])
@pytest.mark.parametrize("task", fc.GATED)
def test_epilogue_forms_match_reference(task, N, monkeypatch):
    monkeypatch.setenv("MS_FUSED", "1")
    run_forms(task, N, tolerance(task))


@pytest.mark.parametrize("task", list(fc.ALL_ENV_IDS))
def test_dispatch(task, monkeypatch):
    """obs_mode="state", the default control mode: the native action map and epilogue are in use, no control step takes the
    kernel's tail, and the model resolves to the two-row plain step k_solve16<15, 0, false, 2>. The handle has no entry
    point that names its instance: `fc.plain_instance` restates mssim_dispatch::plain_step / rows_per_env in Python (as
    tests/test_gpu_place_tool.py and tests/test_gpu_poke_lift.py do), so this pins the model's shape, not the host's pick;
    a model without an instance is refused by mssim_create. A profile that somebody removed from the handle is set again
    before the next epilogue launch."""
    monkeypatch.setenv("MS_FUSED", "1")
    N = 17
    env = fc.make_env(task, N, BACKEND, obs_mode="state")
    base = env.unwrapped
    px = base.scene.px
    assert base._use_fused_callers and base._fused_ok()
    model = base.scene.model
    assert (int(model.n_dof), int(model.n_free)) == (15, fc.N_FREE[task]) and fc.plain_instance(model) == (15, 2)
    g = torch.Generator().manual_seed(0)
    for _ in range(3):
        a = (2 * torch.rand(N, 13, generator=g) - 1).cuda()
        assert base._fused_action_ready(a)
        obs, rew, *_ = env.step(a)
    assert obs.shape == (N, 30 + fc.OBS_EXTRA[task]) and torch.isfinite(obs).all() and torch.isfinite(rew).all()
    assert px.tail_step_count() == 0
    if task in ("pick", "poke", "place"):
        assert px.task_robot == (((0, 3, 0.05), (3, 10, 0.2)), True, 15)
        px.set_task_robot(None)
        env.step(a)
        assert px.task_robot == (((0, 3, 0.05), (3, 10, 0.2)), True, 15)
    else:
        assert px.task_robot is None
    assert px.overflow_count() == 0
    env.close()


# ---------------------------------------------------------------------------------------------------------------------
ENV_N, ENV_STEPS, RESET_AT = 32, 25, 12
RESET_IDX = (1, 5, ENV_N - 1)


def _keep(d):
    return {k: v.cpu().clone() for k, v in d.items() if isinstance(v, torch.Tensor)}


def _torch_path(base, action):
    """what the env's step computes with MS_FUSED=0, on the state the env is in: get_info, get_obs, get_reward"""
    info = base.get_info()
    obs = base.get_obs(info)
    rew = base.get_reward(obs=obs, action=action, info=info) if action is not None else torch.zeros(base.num_envs)
    return obs.cpu().clone(), rew.cpu().clone(), _keep(info)


def run_rollout(task, tol):
    """25 random-action control steps with a partial reset after the 12th: every output of env.step on the native path
    against the torch path on that very state. -> the largest reward / info float difference"""
    g = torch.Generator().manual_seed(3)
    acts = [2 * torch.rand(ENV_N, 13, generator=g) - 1 for _ in range(ENV_STEPS)]
    env = fc.make_env(task, ENV_N, BACKEND, seed=5, reward_mode="dense")
    base = env.unwrapped
    px = base.scene.px
    assert base._use_fused_callers and base._fused_ok() and base._fused_action_ready(acts[0].cuda()), "native action map / epilogue not in use"
    obs, rinfo = env.reset(seed=5)
    z = torch.zeros(ENV_N)
    pairs = [((obs.cpu().clone(), z, _keep(rinfo)), _torch_path(base, None), True)]
    for i, a in enumerate(acts):
        obs, rew, term, trunc, info = env.step(a.cuda())
        assert torch.equal(term.cpu(), info["success"].cpu()) and not trunc.any()
        pairs.append(((obs.cpu().clone(), rew.cpu().clone(), _keep(info)), _torch_path(base, a.cuda()), False))
        if i + 1 == RESET_AT:
            obs, rinfo = env.reset(options=dict(env_idx=torch.tensor(RESET_IDX, device=base.device)))
            pairs.append(((obs.cpu().clone(), z, _keep(rinfo)), _torch_path(base, None), True))
    assert px.tail_step_count() == 0 and px.overflow_count() == 0
    env.close()
    d_rew = d_inf = 0.0
    for step, ((o1, r1, i1), (o2, r2, i2), is_reset) in enumerate(pairs):
        assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)), (task, step, float((o1 - o2).abs().max()))
        assert list(i1.keys()) == list(i2.keys()), (task, step)
        for k in i1:
            assert i1[k].shape == i2[k].shape and i1[k].dtype == i2[k].dtype, (task, step, k)
            if i1[k].dtype.is_floating_point:
                d_inf = max(d_inf, float((i1[k] - i2[k]).abs().max()))
            else:
                assert torch.equal(i1[k], i2[k]), (task, step, k)
        if not is_reset:
            d_rew = max(d_rew, float((r1 - r2).abs().max()))
    print(f"{fc.ALL_ENV_IDS[task]} with the Fetch: max |epilogue - torch path on the same state| reward {d_rew:.3e}, info floats {d_inf:.3e} (tolerance {tol:.3e})")
    assert d_rew <= tol and d_inf <= tol
    return d_rew, d_inf


@pytest.mark.parametrize("task", list(fc.ALL_ENV_IDS))
def test_env_step_matches_torch_path(task, monkeypatch):
    monkeypatch.setenv("MS_FUSED", "1")
    run_rollout(task, tolerance(task))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id", ["PickCube-v1", "PlaceSphere-v1"])
def test_profile_is_inert_for_a_panda(env_id, monkeypatch):
    """64 Panda envs, 10 steps, then the goal / the bin brought to the object so that the robot's is_static is read: with no
    profile set (PickCube: the epilogue at the control-step kernel's tail) against the Panda's rules set as a profile (every
    epilogue a launch of its own, through the profile's code): bit-identical"""
    import gymnasium as gym

    from maniskill_amd.utils.structs.pose import Pose

    monkeypatch.setenv("MS_FUSED", "1")
    N, STEPS = 64, 10
    g = torch.Generator().manual_seed(1)
    acts = [(2 * torch.rand(N, 8, generator=g) - 1) for _ in range(STEPS)]
    runs = []
    for profile in (False, True):
        env = gym.make(env_id, num_envs=N, sim_backend=BACKEND, reward_mode="dense")
        base = env.unwrapped
        px = base.scene.px
        obs, info = env.reset(seed=2)
        assert base._fused_ok() and px.task_robot is None
        if profile:
            px.set_task_robot(ranges=[(0, 7, 0.2)], signed_compare=False, pick_norm_dofs=7)
        out = [(obs.cpu().clone(), torch.zeros(N), _keep(info))]
        for a in acts:
            obs, rew, term, trunc, info = env.step(a.cuda())
            out.append((obs.cpu().clone(), rew.cpu().clone(), _keep(info)))
        tails = px.tail_step_count()
        assert tails == (0 if profile or env_id != "PickCube-v1" else STEPS)
        if env_id == "PickCube-v1":
            base.goal_site.set_pose(Pose.create_from_pq(base.cube.pose.p))
        else:
            base.bin.set_pose(Pose.create_from_pq(base.obj.pose.p - torch.tensor([0.0, 0.0, base.radius + base.block_half_size[0]], device=base.device)))
        base.scene._gpu_apply_all()
        base.scene._gpu_fetch_all()
        obs, rew, info = base._fused_step_outputs(None, advance=False)
        read = info["is_obj_placed"] if env_id == "PickCube-v1" else info["is_obj_on_bin"]
        assert read.all(), "the state in which the reward reads the robot's velocities"
        out.append((obs.cpu().clone(), rew.cpu().clone(), _keep(info)))
        runs.append(out)
        env.close()
    for step, ((o1, r1, i1), (o2, r2, i2)) in enumerate(zip(*runs)):
        assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)) and torch.equal(r1.view(torch.int32), r2.view(torch.int32)), (env_id, step)
        assert i1.keys() == i2.keys() and all(torch.equal(i1[k], i2[k]) for k in i1), (env_id, step)


def test_profile_refusals():
    from maniskill_amd import native

    env = fc.make_env("pick", 2, BACKEND)
    px = env.unwrapped.scene.px
    for bad in (dict(ranges=[(0, 16, 0.2)]), dict(ranges=[(14, 2, 0.2)]), dict(ranges=[(-1, 2, 0.2)]), dict(ranges=[(0, 3, float("nan"))]),
                dict(ranges=[(0, 3, 0.05)], pick_norm_dofs=16)):
        with pytest.raises(native.NativeError, match=r"\(3\).*set_task_robot"):
            px.set_task_robot(**bad)
    px.set_task_robot(None)
    assert px.task_robot is None
    env.close()


def test_cameras_of_a_camera_obs_mode():
    """a table-top task with the Fetch has three cameras: the task's own and the robot's two"""
    env = fc.make_env("pick", 2, BACKEND, obs_mode="depth+segmentation")
    base = env.unwrapped
    obs, _ = env.reset(seed=0)
    data = obs["sensor_data"]
    assert set(data) == {"base_camera", "fetch_head", "fetch_hand"}
    for uid in data:
        assert set(data[uid]) == {"depth", "segmentation"} and data[uid]["depth"].shape == (2, 128, 128, 1)
    link_ids = {int(l._per_scene_id) for l in base.agent.robot.links}
    for e in range(2):
        seen = set(np.unique(data["base_camera"]["segmentation"][e].cpu().numpy()).tolist())
        assert seen & link_ids, "base_camera sees the Fetch"
        assert int(base.cube._per_scene_id) in seen
    env.close()
