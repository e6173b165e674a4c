"""The per-env bookkeeping around the narrowphase of k_solve16 against the CPU oracle: cache-slot assignment of the
generic-convex pairs (stage B0), the patch pass (anchors, 4-point selection, record layout) on hit lists of 1, 16, 17 and 33
manifolds, and the hits of sleeping bodies that leave the hit list before any manifold is computed ("doomed pairs").

Every case is a small scene run for a few control steps (5 substeps each) on both sides from the same initial state; the
sides run freely, because a state written back through the apply calls wakes bodies and drops the cached contacts these
tests are about. Contact counts per pair must be equal, states within the tolerances tests/test_gpu_parity.py uses for the
same quantities (5e-5 on a free body's pose over the first substeps of a resting contact, 2e-5 after box-box rest).
Only cases whose counts are the same in the f32 and the f64 oracle are kept: that is checked here, on the CPU, for all of
them (a count that depends on rounding says nothing about the kernel). Poses are dyadic fractions (tests/narrowphase_cases.py)."""
import functools

import numpy as np
import pytest
import torch

from maniskill_amd.model import geom
from maniskill_amd.model.compile import ActorRecord, SceneModelBuilder, ShapeRecord
from maniskill_amd.model.scenes import cube_record, ground_record, panda_tabletop_model, table_record
from tests import oracle_backend as ob

H = 1.0 / 128  # half size of the small shapes
PITCH = 1.0 / 32  # grid pitch
TILT = (1.0, 1.0 / 256, 1.0 / 512, 0.0)  # (about half a degree: the deepest corner of a resting hull is unique in f32 and f64)


def _grid(i):
    return np.array([(i % 6 - 2.5) * PITCH, (i // 6 - 2.5) * PITCH, 0.0])


def _hull(i):
    v = np.array([[sx * H, sy * H, sz * H] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64)
    return ShapeRecord("convex", geom.pose(_grid(i)), vertices=v)


def _box(i):
    return ShapeRecord("box", geom.pose(_grid(i)), half_size=np.array([H, H, H]))


def _ball(i):
    return ShapeRecord("sphere", geom.pose(_grid(i)), radius=H)


def _none():
    return ShapeRecord("none", geom.pose())


def _rack(name, per_env, slots, pose):
    env_shapes = [list(s) + [_none() for _ in range(slots - len(s))] for s in per_env]
    return ActorRecord(name, "dynamic", list(env_shapes[0]), initial_pose=pose, env_shapes=env_shapes)


class Case:
    """model, number of envs, control steps, `init(px, model, N)` and `before(px, model, N, step)` (both sides), pose tolerance"""

    def __init__(self, model, N, steps, init=None, before=None, tol=5e-5, bodies=()):
        self.model, self.N, self.steps, self.init, self.before, self.tol, self.bodies = model, N, steps, init, before, tol, bodies


def _rows(px, model, N, name):
    r = model.row_of(name)
    return px.cuda_rigid_body_data.torch()[r * N : (r + 1) * N]


def slot_case(counts, third_body):
    """a rack of `counts[e]` small hulls resting on the table in env e (each a generic-convex pair with the table box) and a lone
    hull beside it: with 16 cache slots per env the 17th pair goes without one. After two control steps the lone hull is taken
    away, its slot is the only one not touched in the substep, and the least-recently-used rule gives it to the pair that
    had none."""
    N, slots = len(counts), max(counts)
    b = SceneModelBuilder()
    b.add_actor(table_record())
    b.add_actor(ground_record())
    b.add_actor(ActorRecord("solo", "dynamic", [ShapeRecord("convex", geom.pose(), vertices=_hull(0).vertices)], initial_pose=geom.pose([-0.25, 0, H + 1.0 / 1024], TILT)))
    b.add_actor(_rack("rack", [[_hull(i) for i in range(n)] for n in counts], slots, geom.pose([0, 0, H + 1.0 / 1024], TILT)))
    if third_body:  # (three free bodies: the four-row kernel, whose shape table holds the 33 hulls)
        b.add_actor(cube_record(name="far", p=(0.375, 0.25, 0.02)))
    model = b.compile(num_envs=N)

    def before(px, model, N, step):
        if step == 2:
            px.gpu_fetch_all()
            _rows(px, model, N, "solo")[:, :3] = torch.tensor([-0.25, 0.25, 0.5], device=px.device)
            px.gpu_apply_all()

    return Case(model, N, 4, before=before, bodies=("rack", "solo", "far") if third_body else ("rack", "solo"))


def patch_case():
    """hit lists of 0, 1, 16, 17, 33, 17 and 16 manifolds: a rack of small boxes (or balls) flat on the table is ONE patch of 4
    points per box (1 per ball), cut to 4; the two-box brick beside it, where it is down, a second patch of 8 points that
    carries a torsional record (patch radius). Envs 2, 3, 4: 14 / 15 boxes / 31 balls + the brick's two; env 5: 17 boxes in one
    patch are 68 candidate points (the one-lane scans); env 6: 16 boxes are 64 (the group's selection at its limit). The third
    body (it makes the model a four-row one, whose shape table holds the rack) falls freely beside them in every env."""
    per_env = [[], [_box(0)], [_box(i) for i in range(14)], [_box(i) for i in range(15)], [_ball(i) for i in range(31)], [_box(i) for i in range(17)],
               [_box(i) for i in range(16)]]
    brick_down = [False, False, True, True, True, False, False]
    N = len(per_env)
    half = np.array([1.0 / 64, 1.0 / 64, 1.0 / 64])
    b = SceneModelBuilder()
    b.add_actor(table_record())
    b.add_actor(ground_record())
    b.add_actor(ActorRecord("brick", "dynamic", [ShapeRecord("box", geom.pose([-1.0 / 32, 0, 0]), half_size=half, patch_radius=1.0 / 128, min_patch_radius=1.0 / 128),
                                                 ShapeRecord("box", geom.pose([1.0 / 32, 0, 0]), half_size=half)], initial_pose=geom.pose([-0.25, 0, 1.0 / 64])))
    b.add_actor(_rack("rack", per_env, 31, geom.pose([0, 0, H])))
    b.add_actor(cube_record(name="far", p=(0.375, 0.25, 0.02)))
    model = b.compile(num_envs=N)

    def init(px, model, N):
        px.gpu_fetch_all()
        z = torch.tensor([1.0 / 64 if d else 0.5 for d in brick_down], device=px.device)
        _rows(px, model, N, "brick")[:, 2] = z.to(_rows(px, model, N, "brick").dtype)
        _rows(px, model, N, "far")[:, 2] = 0.5  # (in no env in range of anything; env 0: no hit at all)
        px.gpu_apply_all()

    return Case(model, N, 3, init=init, tol=2e-5, bodies=("rack", "brick", "far"))


def crowded_wave_case():
    """four envs (one wave) with a rack of three boxes and a two-box body each on the table: everything goes to sleep, then the
    racks are lifted a millimetre and drop back. The wave then has 12 box-box pairs of awake bodies and 8 doomed ones of
    the sleepers: 20 in range, more than the 16 up to which 16-lane groups take them, but only with the doomed ones
    counted -- the counts from before the removal choose the path (one lane per pair). The racks' manifolds, counts and
    states must be the oracle's."""
    N = 4
    half = np.array([1.0 / 64, 1.0 / 64, 1.0 / 64])
    b = SceneModelBuilder()
    b.add_actor(table_record())
    b.add_actor(ground_record())
    b.add_actor(ActorRecord("cube", "dynamic", [ShapeRecord("box", geom.pose([-1.0 / 32, 0, 0]), half_size=half), ShapeRecord("box", geom.pose([1.0 / 32, 0, 0]), half_size=half)],
                            initial_pose=geom.pose([-0.25, 0, 1.0 / 64])))
    b.add_actor(_rack("rack", [[_box(i) for i in range(3)] for _ in range(N)], 3, geom.pose([0, 0, H])))
    model = b.compile(num_envs=N)

    def before(px, model, N, step):
        if step == 10:
            px.gpu_fetch_all()
            _rows(px, model, N, "rack")[:, 2] = H + 1.0 / 1024
            px.gpu_apply_all()

    return Case(model, N, 13, before=before, tol=2e-5, bodies=("rack", "cube"))


CASES = {
    "slots_0_1_16_17": lambda: slot_case([0, 1, 16, 17], False),
    "slots_33": lambda: slot_case([0, 17, 33], True),
    "patches": patch_case,
    "crowded_wave": crowded_wave_case,
}


@functools.lru_cache(maxsize=None)
def case_of(name):
    return CASES[name]()


def run(px, case):
    model, N = case.model, case.N
    if case.init:
        case.init(px, model, N)
    out = []
    for i in range(case.steps):
        if case.before:
            case.before(px, model, N, i)
        px.step(5)
        px.gpu_fetch_all()
        out.append(dict(rb=px.cuda_rigid_body_data.torch().cpu().clone().reshape(model.n_rows, N, 13),
                        cnt=px.read_internal("contact_count", max(model.n_pair, 1)).cpu().clone(),
                        wake=px.read_internal("free_wake", model.n_free).cpu().clone()))
    return out


@functools.lru_cache(maxsize=None)
def oracle_run(name, precision):
    """the oracle's trajectory of a case: computed once, shared by the tests, never written to"""
    case = case_of(name)
    return run(ob.make_system(case.model, case.N, precision=precision), case)


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_have_the_same_counts_in_the_f32_and_f64_oracles(name):
    a, b = oracle_run(name, "f32"), oracle_run(name, "f64")
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x["cnt"], y["cnt"]), (name, i)
        assert torch.equal(x["wake"] > 0, y["wake"] > 0), (name, i)
    assert sum(int(x["cnt"].sum()) for x in b) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_and_states_match_the_oracle(name):
    from maniskill_amd.physx.system import MssimSystem

    case = case_of(name)
    gpu = MssimSystem(device="cuda:0")
    gpu.gpu_init(case.model, case.N)
    got, ref = run(gpu, case), oracle_run(name, "f64")
    assert gpu.overflow_count() == 0
    rows = [case.model.row_of(b) for b in case.bodies]
    for i, (x, y) in enumerate(zip(got, ref)):
        print(name, "step", i, "contacts per env", x["cnt"].sum(0).tolist(), "max |dpose|", float(torch.max(torch.abs(x["rb"][rows, :, :7] - y["rb"][rows, :, :7]))))
        assert torch.equal(x["cnt"], y["cnt"]), (name, i, x["cnt"].sum(0), y["cnt"].sum(0))  # every pair of every env
        assert torch.equal(x["wake"] > 0, y["wake"] > 0), (name, i)
        assert torch.max(torch.abs(x["rb"][rows, :, :7] - y["rb"][rows, :, :7])) < case.tol, (name, i)


def test_the_cases_cover_the_sizes_they_are_about():
    """what the oracle's counts (after the patch reduction: 4 points per body pair) show of the cases: the racks and the lone
    hull rest on the table until the lone hull is taken away; in the patch case env 0 has no contact at all, every rack and
    brick is one patch of 4 points, however many manifolds went into it; in the crowded wave only the racks wake"""
    for name in ("slots_0_1_16_17", "slots_33"):
        ref = oracle_run(name, "f64")
        with_solo, without = ref[1]["cnt"].sum(0), ref[3]["cnt"].sum(0)
        assert torch.all(with_solo > without) and torch.all(without[1:] >= 4), (name, with_solo, without)
    ref = oracle_run("patches", "f64")
    assert ref[0]["cnt"].sum(0).tolist() == [0, 4, 8, 8, 8, 4, 4]  # (nothing | rack | rack, brick | .. | rack | rack)
    ref = oracle_run("crowded_wave", "f64")
    assert torch.all(ref[9]["wake"] == 0) and torch.all(ref[11]["wake"][0] == 0) and torch.all(ref[11]["wake"][1] > 0)
    assert ref[11]["cnt"].sum(0).tolist() == [4, 4, 4, 4]


# ---------------------------------------------------------------- doomed pairs


def _two_cubes_and_a_slab():
    from tests.test_oracle_contacts import _slab_on_table

    return _slab_on_table(True)


@pytest.mark.gpu
def test_a_cube_asleep_on_the_kinematic_table_stays_bit_for_bit_and_wakes_with_the_oracle_when_the_arm_arrives():
    """PickCube's scene content: the cube goes to sleep on the kinematic table beside the fixed ground (its pair with the
    table is then doomed in every substep), stays frozen bit for bit over 50 control steps, and wakes in the same substep
    as in the oracle when the hand is driven down onto it; it is not pushed into the table."""
    from maniskill_amd.physx.system import MssimSystem
    from tests.test_gpu_parity import REST

    model = panda_tabletop_model()
    N = 2
    gpu = MssimSystem(device="cuda:0")
    gpu.gpu_init(model, N)
    cpu = ob.make_system(model, N, precision="f64")
    r = model.row_of("cube")
    q = REST.expand(N, 9).clone()
    for px in (gpu, cpu):
        px.cuda_articulation_qpos.torch()[:] = q.to(px.device)
        px.cuda_articulation_target_qpos.torch()[:] = q.to(px.device)
        px.gpu_apply_all()
        px.step(60)
    wg, wc = gpu.read_internal("free_wake", 1).cpu(), cpu.read_internal("free_wake", 1)
    assert torch.all(wg == 0) and torch.all(wc == 0)
    gpu.gpu_fetch_all()
    frozen = gpu.cuda_rigid_body_data.torch()[r * N : (r + 1) * N].clone()
    for px in (gpu, cpu):
        px.step(250)
    gpu.gpu_fetch_all()
    assert torch.equal(gpu.cuda_rigid_body_data.torch()[r * N : (r + 1) * N], frozen)
    assert int(gpu.read_internal("contact_count", model.n_pair).sum()) == int(cpu.read_internal("contact_count", model.n_pair).sum())
    # the hand comes down onto the cube (tool centre at (0, 0, 0.02) with the fingers closing)
    tq = torch.tensor([[0.0, 0.71518, 0.0, -1.863259, 0.0, 2.497662, 0.785398, 0.0, 0.0]]).expand(N, 9)
    for px in (gpu, cpu):
        px.cuda_articulation_target_qpos.torch()[:] = tq.to(px.device)
        px.gpu_apply_articulation_target_position()
    woke = None
    for i in range(200):
        for px in (gpu, cpu):
            px.step(1)
        wg, wc = gpu.read_internal("free_wake", 1).cpu(), cpu.read_internal("free_wake", 1)
        assert torch.equal(wg > 0, wc > 0), i
        if torch.all(wg > 0):
            woke = i
            break
    assert woke is not None
    for px in (gpu, cpu):
        px.step(20)
        px.gpu_fetch_all()
    a = gpu.cuda_rigid_body_data.torch()[r * N : (r + 1) * N].cpu()
    assert torch.all(a[:, 2] > 0.02 - 1e-3), a[:, 2]


@pytest.mark.gpu
def test_a_hull_asleep_on_the_kinematic_table_keeps_its_pair_and_matches_the_oracle():
    """a sleeping body's generic-convex pair is not doomed (its cache slot's stamps): the slab hull of the persistent-manifold
    test goes to sleep with its manifold, stays frozen, and counts and wake counters follow the oracle throughout"""
    from maniskill_amd.physx.system import MssimSystem

    model = _two_cubes_and_a_slab()
    N = 4
    gpu = MssimSystem(device="cuda:0")
    gpu.gpu_init(model, N)
    cpu = ob.make_system(model, N, precision="f64")
    row = model.row_of("slab")
    for px in (gpu, cpu):
        s = px.cuda_rigid_body_data.torch()[row * N : (row + 1) * N]
        s[:, 2] = 0.02 + 1.0 / 1024
        s[:, 3:7] = torch.tensor(geom.pose(q=TILT)[3:], dtype=s.dtype, device=s.device)
        px.gpu_apply_all()
    frozen = None
    for i in range(24):
        for px in (gpu, cpu):
            px.step(5)
        wg, wc = gpu.read_internal("free_wake", 1).cpu(), cpu.read_internal("free_wake", 1)
        assert torch.equal(wg > 0, wc > 0), i
        gpu.gpu_fetch_all()
        cpu.gpu_fetch_all()
        a, b = gpu.cuda_rigid_body_data.torch()[row * N : (row + 1) * N].cpu(), cpu.cuda_rigid_body_data.torch()[row * N : (row + 1) * N]
        assert torch.max(torch.abs(a[:, :7] - b[:, :7].to(a.dtype))) < 2e-4, i
        if torch.all(wg == 0):
            if frozen is None:
                frozen = a.clone()
            assert torch.equal(a, frozen), i
    assert frozen is not None
