"""The native action map of the HIP library against the float64 reference (tests/action_reference.py), case by case
(tests/action_cases.py: the case of env i sits in env i), at env counts 128 and the ragged 1, 17, 67, in its forms:

  1. stand-alone: `set_action_map / set_ee_action_map`, `apply_action`, targets read back; nothing is stepped. The
     only form that sees NaN / +-inf (last env of the batch): its outputs equal the reference's, NaN where it says NaN,
     and no other env notices;
  2. head of the control step: `step_action(a, 1)` -- joint-space maps run at the head of k_solve16, end-effector maps
     as apply_action + step -- targets read after the launch, reference evaluated at the pre-step joint positions;
  3. owed form: `env.step` of PickCube and PushT, where the action map, the substeps, the copy-out and the task
     epilogue are one launch: targets bit-identical to form 2.

Every form: targets the map does not write (dofs without a column, the other buffer of a dof) keep the previous
pattern bit for bit; the action is a slice of a larger tensor with NaN in front of and behind it; the visible target
buffers and the simulation's own copy agree. Joint-space entries are held to the derived band, end-effector entries to
the band measured on the CPU (tests/test_action_reference.py K), twins under another root pose to the same band.
One launch per form and case batch; nothing is stepped from a non-finite target."""
import numpy as np
import pytest
import torch

import maniskill_amd  # noqa: F401
from maniskill_amd.native import NativeError
from tests import action_cases as ac
from tests.test_action_reference import band_k

pytestmark = pytest.mark.gpu
BACKEND = "physx_cuda"
GUARD = 5


def _make(env_id, N, **kw):
    import gymnasium as gym

    import maniskill_amd.envs  # noqa: F401

    env = gym.make(env_id, num_envs=N, sim_backend=BACKEND, **kw)
    env.reset(seed=0)
    return env


def _spec(name, base):
    spec = ac.HAND_MAPS[name] if name in ac.HAND_MAPS else base.agent.controller.fused_action_spec()
    assert spec is not None, name
    return spec


def _guarded(action, device):
    """the action as rows GUARD .. GUARD + N of a tensor that is NaN everywhere else"""
    N, adim = action.shape
    big = torch.full((N + 2 * GUARD, adim), float("nan"), dtype=torch.float32, device=device)
    big[GUARD : GUARD + N] = torch.from_numpy(action).to(device)
    a = big[GUARD : GUARD + N]
    assert a.is_contiguous()
    return a


def _targets(px, what):
    """visible target buffers after the launch; the simulation's own copy (fetched) must be the same bits"""
    torch.cuda.synchronize()
    tq, tv = px.cuda_articulation_target_qpos.torch().cpu().numpy().copy(), px.cuda_articulation_target_qvel.torch().cpu().numpy().copy()
    px.gpu_fetch_articulation_target_qpos()
    px.gpu_fetch_articulation_target_qvel()
    torch.cuda.synchronize()
    for got, t in ((tq, px.cuda_articulation_target_qpos), (tv, px.cuda_articulation_target_qvel)):
        assert np.array_equal(got.view(np.int32), t.torch().cpu().numpy().view(np.int32)), f"{what}: visible targets differ from the simulation's"
    return tq, tv


def _check(name, spec, A, C, tq, tv, what):
    R = ac.reference(spec, A, C)
    worst = ac.compare(spec, C, R, tq, tv, band_k(spec), what)
    ac.twins_agree(spec, C, R, tq, band_k(spec), what)
    print(f"{what}: largest error / bound {worst:.3f}")
    return R


@pytest.mark.parametrize("N", ac.ENV_COUNTS)
@pytest.mark.parametrize("name", list(ac.MAPS) + list(ac.HAND_MAPS))
def test_action_map_matches_reference(name, N):
    env_id, kw = ac.env_spec(name)
    env = _make(env_id, N, **kw)
    base = env.unwrapped
    px = base.scene.px
    spec = _spec(name, base)
    A, lim, rest, root0 = ac.tables(base)
    px.set_action_map(*spec[:4])
    px.set_ee_action_map(spec[4])

    # ---- form 1: stand-alone, with the non-finite env
    C = ac.build(name, spec, lim, rest, root0, N, nonfinite=True)
    ac.write_state(base, C)
    px.apply_action(_guarded(C["action"], base.device))
    tq1, tv1 = _targets(px, f"stand-alone {name} N={N}")
    _check(name, spec, A, C, tq1, tv1, f"stand-alone {name} N={N}")

    # ---- an action that does not cover every mapped column: refused, nothing written
    ac.write_state(base, C)
    short = _guarded(C["action"][:, : ac.action_dim(spec) - 1], base.device)
    for call in (lambda: px.apply_action(short), lambda: px.step_action(short, 1), lambda: px.step_action(short, 1, defer=True)):
        with pytest.raises(NativeError, match="columns"):
            call()
    tq, tv = _targets(px, f"short action {name} N={N}")
    assert np.array_equal(tq.view(np.int32), C["prev_tq"].view(np.int32)) and np.array_equal(tv.view(np.int32), C["prev_tv"].view(np.int32))

    # ---- form 2: head of the control step, finite actions
    F = ac.build(name, spec, lim, rest, root0, N)
    ac.write_state(base, F)
    px.step_action(_guarded(F["action"], base.device), 1)
    tq2, tv2 = _targets(px, f"step head {name} N={N}")
    _check(name, spec, A, F, tq2, tv2, f"step head {name} N={N}")
    px.gpu_fetch_all()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(px.cuda_articulation_qpos.torch()).all()) and bool(torch.isfinite(px.cuda_articulation_qvel.torch()).all())
    env.close()


@pytest.mark.parametrize("N", ac.ENV_COUNTS)
@pytest.mark.parametrize("env_id", ["PickCube-v1", "PushT-v1"])
def test_owed_form_writes_the_targets_of_the_step_head(env_id, N):
    name = "panda:pd_joint_delta_pos" if env_id == "PickCube-v1" else "panda_stick:pd_joint_delta_pos"
    env = _make(env_id, N)
    base = env.unwrapped
    px = base.scene.px
    spec = _spec(name, base)
    A, lim, rest, root0 = ac.tables(base)
    F = ac.build(name, spec, lim, rest, root0, N)
    action = _guarded(F["action"], base.device)
    assert base._fused_action_ready(action) and base._fused_ok(), "the env does not take the one-launch step"
    ac.write_state(base, F)
    px.step_action(action, 1)
    tq2, tv2 = _targets(px, f"step head {env_id} N={N}")
    _check(name, spec, A, F, tq2, tv2, f"step head {env_id} N={N}")
    env.reset(seed=0)
    ac.write_state(base, F)
    t0 = px.tail_step_count()
    env.step(action)
    assert px.tail_step_count() == t0 + 1, "the step did not run as one launch with the action map at its head"
    tq3, tv3 = _targets(px, f"owed form {env_id} N={N}")
    assert np.array_equal(tq2.view(np.int32), tq3.view(np.int32)) and np.array_equal(tv2.view(np.int32), tv3.view(np.int32))
    env.close()
