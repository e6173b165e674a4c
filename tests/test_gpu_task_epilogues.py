"""The five task epilogues of the HIP library against the float64 reference (tests/task_reference.py), case by case
(tests/task_cases.py), in their three launch forms: the standalone kernel (k_task_*<false>), the kernel that first copies
the state out (k_task_*<true>) and the tail of the control-step kernel (k_solve16<.., TASK>), at env counts 128 and the
ragged 1, 17, 67. Flags must equal the reference's wherever its predicate is decided, PushT's count must lie in the
reference's interval, copied / single-subtraction observation entries are bit-exact, rewards (and Peg's hole pose) agree
within 4 x the difference measured between the torch path and the reference on the CPU (tests/task_cases.py MEASURED).

One env per (task, N), used in this order: reset state -> standalone (free batch, nothing grasped) -> scripted grasp in
every env -> constructed states set through the actors (goal / box / cube B brought to the held object, releases, arm
motion) -> ONE fused control step, the tail form -> scripted grasp again -> standalone (grasped batch, several task
structs alternating on one handle, min_force at a measured force x (1 +- 1e-3)) -> copy-out form -> containment. Every
form asserts from the reference's flags which tiers it reached. Nothing is stepped after the case tables (which hold
unphysical states) were applied to the simulation.

What a form cannot reach: the copy-out form recomputes the link rows from qpos, so the cases that write the tcp or a
finger row (PushCube's `near`, the finger angles) exist in the standalone form only; PushCube's `near` tier is reached in
the tail form by moving the hand to the table."""
import numpy as np
import pytest
import torch

from tests import task_cases as tc
from tests import task_reference as ref
from tests.task_cases import MEASURED, assert_expect, compare, gpu_tolerance

pytestmark = pytest.mark.gpu
BACKEND = "physx_cuda"
TASKS = ["pick", "push", "peg", "stack", "pusht"]
GUARD = 8
NORMALIZED = dict(pick=0.2, push=1.0 / 3.0, peg=0.1, stack=0.125)
POSE_TOL = 4 * MEASURED["peg_pose"]


def _alloc(task, base, N):
    D = 2 * base.agent.robot.max_dof + tc.OBS_EXTRA[task]
    dev = base.device
    out = dict(obs=torch.full((N + GUARD, D), -77.0, device=dev), reward=torch.full((N + GUARD,), -77.0, device=dev),
               flags=torch.full((N + GUARD, tc.N_FLAGS[task]), 0xAB, dtype=torch.uint8, device=dev))
    if task in ("peg", "pusht"):
        out["extra"] = torch.full((N + GUARD, 3 if task == "peg" else 1), -77.0, device=dev)
    return out


def _call(task, base, struct, out):
    px = base.scene.px
    if task == "peg":
        px.task_peg_outputs(struct, out["obs"], out["reward"], out["flags"], out["extra"])
    elif task == "pusht":
        px.task_pusht_outputs(struct, out["obs"], out["reward"], out["flags"], out["extra"])
    else:
        getattr(px, f"task_{task}_outputs")(struct, out["obs"], out["reward"], out["flags"])
    torch.cuda.synchronize()


def _read(task, out, N):
    """-> the `got` dict of compare(); asserts that nothing behind row N was written"""
    for k, t in out.items():
        g = t[N:]
        assert bool((g == (0xAB if t.dtype == torch.uint8 else -77.0)).all()), (task, k, "guard rows written")
    fl = out["flags"][:N].cpu().numpy()
    assert ((fl == 0) | (fl == 1)).all()
    got = dict(obs=out["obs"][:N].cpu().numpy(), reward=out["reward"][:N].cpu().numpy(),
               flags={name: fl[:, i].astype(bool) for i, name in enumerate(tc.FLAG_NAMES[task])})
    if task == "peg":
        got["head_at_hole"] = out["extra"][:N].cpu().numpy()
    if task == "pusht":
        got["count"] = out["extra"][:N, 0].cpu().numpy()
    return got


def _standalone(task, base, S, P, labels, what):
    N = base.num_envs
    base.scene._gpu_fetch_all()  # (nothing owed to the next native call: the launch is k_task_*<false>)
    tc.write_buffers(base, S)
    keep = []
    out = _alloc(task, base, N)
    _call(task, base, tc.native_task(task, base, P, keep), out)
    got = _read(task, out, N)
    R = ref.TASKS[task](S, P)
    compare(task, got, R, labels, gpu_tolerance(task, P), POSE_TOL, what=what)
    return got, R


def _tail_params(task, base):
    P = tc.params(task, base)
    if base._reward_mode == "normalized_dense":
        if task == "pusht":
            P["reward_div"] = 3.0
        else:
            P["reward_scale"] = float(np.float32(NORMALIZED[task]))
    return P


def _tail_step(task, env, action, what):
    """one env.step as ONE launch with the epilogue at the control-step kernel's tail; the reference on the post-step
    buffers and impulses. elapsed_steps one below / at the time limit in alternating envs."""
    base = env.unwrapped
    N = base.num_envs
    assert base._fused_ok() and base._time_limit is not None
    limit = int(base._time_limit)
    es = torch.full((N,), limit - 2, dtype=base._elapsed_steps.dtype, device=base.device)
    es[1::2] = limit - 1
    base._elapsed_steps[:] = es
    t0 = base.scene.px.tail_step_count()
    obs, rew, term, trunc, info = env.step(action)
    torch.cuda.synchronize()
    assert base.scene.px.tail_step_count() == t0 + 1, (what, "the step did not take the fused tail")
    S = tc.snapshot(base)
    P = _tail_params(task, base)
    R = ref.TASKS[task](S, P)
    got = dict(obs=obs.cpu().numpy(), reward=rew.cpu().numpy(), flags={k: info[k].cpu().numpy().astype(bool) for k in tc.FLAG_NAMES[task]})
    if task == "peg":
        got["head_at_hole"] = info["peg_head_pos_at_hole"].cpu().numpy()
    if task == "pusht":
        got["count"] = base._fused_intersection.cpu().numpy()
    labels = ["after one step"] * N
    compare(task, got, R, labels, gpu_tolerance(task, P), POSE_TOL, what=what)
    new, truncated = ref.time_limit(es.cpu().numpy(), limit)
    assert np.array_equal(info["elapsed_steps"].cpu().numpy(), new) and np.array_equal(trunc.cpu().numpy(), truncated), what
    assert truncated[1::2].all() and not truncated[0::2].any()
    assert np.array_equal(term.cpu().numpy(), got["flags"]["success"]), what
    return R


def _copy_out(task, base, S, P, labels, what):
    """the case states applied to the simulation, the copy-out owed to the task call: k_task_*<true>"""
    N = base.num_envs
    px = base.scene.px
    base.scene._gpu_fetch_all()
    tc.write_buffers(base, S)
    base.scene._gpu_apply_all()
    px.gpu_update_articulation_kinematics()
    stale = {**S, "rigid": np.full_like(S["rigid"], 5.0)}
    tc.write_buffers(base, stale)  # (the launch has to refill the buffers)
    t0 = px.tail_step_count()
    px.defer_fetch_all()
    keep = []
    out = _alloc(task, base, N)
    _call(task, base, tc.native_task(task, base, P, keep), out)
    assert px.tail_step_count() == t0
    got = _read(task, out, N)
    S1 = tc.snapshot(base)
    assert not np.array_equal(S1["rigid"], stale["rigid"]), "the copy-out did not run"
    R = ref.TASKS[task](S1, P)
    compare(task, got, R, labels, gpu_tolerance(task, P), POSE_TOL, what=what)
    return R


def _containment(task, base, S, P, what):
    """one poisoned env (PushT: |q_w| > 1, acos -> NaN; the others: a NaN object position): its neighbours' outputs do not
    change by a bit and it does not succeed"""
    N = base.num_envs
    if N < 3:
        return
    k = N // 2
    outs = []
    for poison in (False, True):
        S2 = {a: (b.copy() if isinstance(b, np.ndarray) else b) for a, b in S.items()}
        if poison:
            if task == "pusht":
                S2["rigid"][P["tee_row"], k, 3] = 1.5
            else:
                S2["rigid"][P[{"pick": "obj_row", "push": "obj_row", "peg": "peg_row", "stack": "cubeA_row"}[task]], k, 0] = np.nan
        base.scene._gpu_fetch_all()
        tc.write_buffers(base, S2)
        keep = []
        out = _alloc(task, base, N)
        _call(task, base, tc.native_task(task, base, P, keep), out)
        outs.append({a: b.cpu().numpy() for a, b in out.items()})
    others = np.arange(N + GUARD) != k
    for a in outs[0]:
        assert np.array_equal(outs[0][a][others].view(np.uint8), outs[1][a][others].view(np.uint8)), (what, a, "a neighbour of the poisoned env changed")
    assert outs[1]["flags"][k, 0] == 0, (what, "the poisoned env succeeded")


def _coverage(task, R, grasped_batch, fingers=True, near=True):
    """the case table reaches what it claims (from the reference's flags): every combination of the flags the reward reads,
    within the grasped or the ungrasped half that the batch is"""
    F = R["flags"]
    combos = lambda sel, *names: [bool((sel & np.logical_and.reduce([F[n] == v for n, v in zip(names, vals)])).any())
                                  for vals in np.ndindex(*(2,) * len(names))]
    if task == "pick":
        g = F["is_grasped"]
        assert g.any() == grasped_batch
        assert all(combos(g if grasped_batch else ~g, "is_obj_placed", "is_robot_static")), (task, "placed x static")
    if task == "push":
        assert all(combos(np.ones_like(F["low"]), *(("reached",) if near else ()), "inside", "low")), (task, "near x inside x low")
    if task == "stack":
        g = F["is_cubeA_grasped"]
        sel = g if grasped_batch else ~g
        assert all(combos(sel, "is_cubeA_on_cubeB", "static_lin", "static_ang")), (task, "on x linear x angular")
        assert not (F["success"] & g).any() and (not fingers or (F["success"] & ~g).any())
    if task == "peg":
        g = F["is_grasped"]
        sel = g if grasped_batch else ~g
        assert (sel & F["success"]).any()
        for a, b, c in ((False, True, True), (True, False, True), (True, True, False)):
            assert (sel & (F["deep"] == a) & (F["in_y"] == b) & (F["in_z"] == c)).any()
        assert all(combos(sel & ~F["success"], "head_aligned", "body_aligned")[1:]), (task, "head x body alignment")
    if task == "pusht":
        full = R["count_min"] >= 0.9 * R["area"]
        assert F["success"].any() and (R["count_max"] == 0).any() and ((R["count_min"] > 0) & ~full).any()
    if grasped_batch and fingers and task in ("pick", "stack", "peg"):
        assert (F["left"] & ~F["right"]).any() and (~F["left"] & F["right"]).any(), "envs where only one finger qualifies"


def _tail_coverage(task, R):
    """the tiers the ONE fused step reached, from the reference's flags on the post-step state"""
    F = R["flags"]
    if task == "pick":
        g = F["is_grasped"]
        need = dict(grasped_placed=g & F["is_obj_placed"], grasped_unplaced=g & ~F["is_obj_placed"], released=~g, success=F["success"],
                    placed_moving=F["is_obj_placed"] & ~F["is_robot_static"])
    elif task == "stack":
        g, on = F["is_cubeA_grasped"], F["is_cubeA_on_cubeB"]
        need = dict(on_grasped=on & g, on_released=on & ~g, off_grasped=~on & g, off_released=~on & ~g)
    elif task == "peg":
        g = F["is_grasped"]
        al = F["head_aligned"] & F["body_aligned"]
        need = dict(success=F["success"], grasped_aligned=g & al & ~F["success"], grasped_off_axis=g & ~al, released=~g)
    elif task == "push":
        need = dict(near_inside=F["reached"] & F["inside"], near_outside=F["reached"] & ~F["inside"], far_inside=~F["reached"] & F["inside"],
                    far_outside=~F["reached"] & ~F["inside"], success=F["success"])
    else:
        need = dict(success=F["success"], no_success=~F["success"])
    got = {k: int(v.sum()) for k, v in need.items()}
    print(f"tail {task}: {got}")
    assert all(got.values()), (task, "tiers not reached in the tail form", got)


def _force_threshold(task, base, S, P, labels, R0, tag):
    """min_force at a measured finger force x (1 -+ 1e-3): the weaker finger of a grasped env decides `grasped` alone"""
    g = R0["flags"]["is_cubeA_grasped" if task == "stack" else "is_grasped"]
    lf, rf = R0["forces"]
    done = 0
    for weaker, force in ((lf < rf, lf), (rf < lf, rf)):
        envs = np.nonzero(g & weaker)[0]
        if not len(envs):
            continue
        e = int(envs[0])
        for s, want in ((1 - 1e-3, True), (1 + 1e-3, False)):
            Pf = dict(P, min_force=float(np.float32(force[e] * s)))
            got, R = _standalone(task, base, S, Pf, labels, f"{tag} min_force = force x {s}")
            name = "is_cubeA_grasped" if task == "stack" else "is_grasped"
            # (Peg's kernel reports no grasp flag: there the reward, compared in _standalone, carries it)
            assert R["decided"][name][e] and bool(R["flags"][name][e]) == want and bool(got["flags"].get(name, R["flags"][name])[e]) == want, (tag, e, s)
        done += 1
    assert done, "no grasped env to put the force threshold at"


@pytest.mark.parametrize("N", [128, 1, 17, 67])
@pytest.mark.parametrize("task", TASKS)
def test_epilogue_forms_match_reference(task, N, monkeypatch):
    monkeypatch.setenv("MS_FUSED", "1")
    env = tc.make_env(task, N, BACKEND)
    base = env.unwrapped
    full = N == 128
    reduced = None if full else 3
    grasping = task in tc.OBJ
    tag = f"{task} N={N}"
    P = tc.params(task, base)
    # 1. reset state: standalone kernel, nothing grasped
    S0 = tc.snapshot(base)
    S, labels, expect = tc.build_batch(task, S0, P, seed=3, pick=reduced)
    got, R = _standalone(task, base, S, P, labels, tag + " standalone (free)")
    assert_expect(got["flags"], expect, labels, tag)
    assert_expect(R["flags"], expect, labels, tag + " reference", decided=R["decided"] if task == "pusht" else None)
    if full:
        _coverage(task, R, grasped_batch=False)
    tc.write_buffers(base, S0)
    # 2. scripted grasp, constructed states through the actors, then ONE control step with the epilogue at the kernel's tail
    hold = tc.scripted_grasp(env, task) if grasping else torch.zeros(N, base.single_action_space.shape[0], device=base.device)
    action = tc.apply_tail_cases(env, task, hold)
    Rt = _tail_step(task, env, action, tag + " tail")
    if N >= 17:
        _tail_coverage(task, Rt)
    # 3. grasped batch: the env's own parameters and further structs, alternating on one handle
    if grasping:
        tc.scripted_grasp(env, task)
    S0 = tc.snapshot(base)
    forces = None
    if grasping:
        lf, rf = ref.TASKS[task](S0, P)["forces"]
        forces = (float(np.median(lf)), float(np.median(rf)))
    structs = [(P, "own"), (tc.params(task, base, variant=1, forces=forces), "second")]
    if task == "pusht":
        structs.append((tc.params(task, base, variant=2), "third"))
    structs.append((P, "own again"))
    for rnd, (Pv, name) in enumerate(structs):
        S, labels, expect = tc.build_batch(task, S0, Pv, seed=4 + rnd, pick=reduced)
        got, R = _standalone(task, base, S, Pv, labels, f"{tag} standalone ({name} struct)")
        assert_expect(got["flags"], expect, labels, f"{tag} ({name} struct)")
        if full and rnd == 0:
            _coverage(task, R, grasped_batch=grasping)
        if grasping and rnd == 0 and N >= 17:
            _force_threshold(task, base, S, P, labels, R, tag)
    # 4. copy-out form, 5. containment (nothing is stepped from here on)
    S, labels, _ = tc.build_batch(task, S0, P, seed=9, pick=reduced)
    if full:
        Rc = _copy_out(task, base, S, P, labels, tag + " copy-out")
        _coverage(task, Rc, grasped_batch=grasping, fingers=False, near=False)
    _containment(task, base, S, P, tag + " containment")
    env.close()
