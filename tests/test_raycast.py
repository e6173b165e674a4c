"""The ray caster's host side on the CPU: the float64 reference (tests/raycast_reference.py) pinned by closed forms, the
hull face planes, the scene builder on real task models, the validation header under ASan + UBSan as a stand-alone
program, and the case tables (tests/raycast_cases.py): at most 5 % ambiguous pixels per image, and the float32 run of
the reference within MEASURED of the float64 one. The kernel meets the same tables in tests/test_gpu_raycast.py."""
import os
import subprocess

import numpy as np
import pytest

from maniskill_amd.model import compile as mc
from maniskill_amd.model import geom, mesh
from tests import oracle_backend as ob
from tests import raycast_cases as rcc
from tests import raycast_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKEND = "oracle_f64_raycast"
Q_X_TO_Y = (np.sqrt(0.5), 0, 0, np.sqrt(0.5))  # the shape's +x axis turned to the env's +y


def one_shape(type_, pose, param, planes=None):
    T = rcc.SceneTables(1)
    T.add(type_, -1, pose, param, seg=5, planes=planes, bound_r=1.0 if planes is not None else None)
    return T.arrays()


def forward_camera(W, H, fov=1.0, pose=(0, 0, 0, 1, 0, 0, 0)):
    return rcc.camera(W, H, fov, pose=pose)


def rays(cam):
    u = (np.arange(cam["width"]) + 0.5 - cam["cx"]) / cam["fx"]
    v = (np.arange(cam["height"]) + 0.5 - cam["cy"]) / cam["fy"]
    return np.meshgrid(u, v)


# ------------------------------------------------------------------ closed forms
def test_reference_sphere_on_the_optical_axis():
    d, r = 2.0, 0.5
    cam = forward_camera(9, 7)
    R = rr.render(one_shape(rr.SPHERE, (d, 0, 0, 1, 0, 0, 0), (r,)), cam, None, 1, 0)
    x, y = rays(cam)
    a = 1 + x * x + y * y
    disc = d * d - a * (d * d - r * r)
    assert np.array_equal(R["hit"], disc >= 0) and R["hit"].sum() >= 9
    t = (d - np.sqrt(np.where(disc >= 0, disc, 0))) / a
    assert np.abs(R["t"] - np.where(disc >= 0, t, 0)).max() < 1e-12
    assert abs(R["t"][3, 4] - (d - r)) < 1e-12  # the central pixel looks along the axis
    assert np.array_equal(R["seg"], np.where(disc >= 0, 5, 0))
    assert np.array_equal(R["pos_mm"][3, 4], [0, 0, -1500])
    # position in the OpenGL frame: x right, y up, z backward
    assert np.array_equal(R["pos_mm"][..., 0], np.trunc(1000 * x * R["t"])) and np.array_equal(R["pos_mm"][..., 1], np.trunc(-1000 * y * R["t"]))


def test_reference_ground_plane_under_a_tilted_camera():
    h, pitch = 1.25, 0.6  # looking down by `pitch`: a rotation about the camera's y (left) axis
    cam = forward_camera(8, 6, fov=0.9, pose=(0, 0, h, np.cos(pitch / 2), 0, np.sin(pitch / 2), 0))
    R = rr.render(one_shape(rr.PLANE, (0, 0, 0, *rcc.GROUND_Q), ()), cam, None, 1, 0)
    x, y = rays(cam)
    w, qy = (float(v) for v in cam["pose"][[3, 5]])  # the pose is handed over in float32: the angle it encodes, exactly
    sin_p, cos_p = 2 * w * qy / (w * w + qy * qy), (w * w - qy * qy) / (w * w + qy * qy)
    fall = sin_p + cos_p * y  # -(d_env . z) of the ray (1, -x, -y) in SAPIEN camera axes
    t = h / fall
    want = (fall > 0) & (t <= rr.MAX_DEPTH)
    assert want.all() and np.array_equal(R["hit"], want)
    assert np.abs(R["t"] - t).max() < 1e-12
    # from below the ground (inside the half space) nothing is seen
    below = forward_camera(8, 6, fov=0.9, pose=(0, 0, -h, np.cos(pitch / 2), 0, np.sin(pitch / 2), 0))
    assert not rr.render(one_shape(rr.PLANE, (0, 0, 0, *rcc.GROUND_Q), ()), below, None, 1, 0)["hit"].any()


def test_reference_axis_aligned_box_face():
    d, half = 3.0, (0.5, 0.75, 0.375)
    cam = forward_camera(16, 12, fov=0.8)
    R = rr.render(one_shape(rr.BOX, (d, 0, 0, 1, 0, 0, 0), half), cam, None, 1, 0)
    x, y = rays(cam)
    t = d - half[0]
    inside = (np.abs(x * t) <= half[1]) & (np.abs(y * t) <= half[2])
    assert np.array_equal(R["hit"], inside) and 0 < inside.sum() < inside.size
    assert np.abs(R["t"][inside] - t).max() < 1e-12
    # a camera inside the box sees none of it (its start is in the interior), and a near plane behind the face culls it
    assert not rr.render(one_shape(rr.BOX, (0.1, 0, 0, 1, 0, 0, 0), half), cam, None, 1, 0)["hit"].any()
    assert not rr.render(one_shape(rr.BOX, (d, 0, 0, 1, 0, 0, 0), half), dict(cam, near=t + 1e-3), None, 1, 0)["hit"].any()
    assert rr.render(one_shape(rr.BOX, (d, 0, 0, 1, 0, 0, 0), half), dict(cam, near=t - 1e-3), None, 1, 0)["hit"].sum() == inside.sum()


@pytest.mark.parametrize("type_", [rr.CAPSULE, rr.CYLINDER])
def test_reference_capsule_and_cylinder_end_on_and_side_on(type_):
    d, r, hl = 2.5, 0.25, 0.625  # (exact in float32, as the tables hold them)
    cam = forward_camera(41, 11, fov=0.7)
    x, y = rays(cam)
    a = 1 + x * x + y * y
    # end-on: the axis is the optical axis
    R = rr.render(one_shape(type_, (d, 0, 0, 1, 0, 0, 0), (r, hl)), cam, None, 1, 0)
    if type_ == rr.CAPSULE:  # all that shows is the front ball, centre d - hl
        c = d - hl
        disc = c * c - a * (c * c - r * r)
        t = (c - np.sqrt(np.where(disc >= 0, disc, 0))) / a
        assert abs(R["t"][5, 20] - (d - hl - r)) < 1e-12
    else:                    # the front cap, a disc of radius r at depth d - hl
        t = np.full(x.shape, d - hl)
        disc = r * r - (x * x + y * y) * t * t
    assert np.array_equal(R["hit"], disc >= 0) and R["hit"].sum() >= 5
    assert np.abs(R["t"] - np.where(disc >= 0, t, 0)).max() < 1e-12
    # side-on: the axis along the env's y. On the middle row the side is met at depth d - r along the whole straight part
    R = rr.render(one_shape(type_, (d, 0, 0, *Q_X_TO_Y), (r, hl)), cam, None, 1, 0)
    row = R["t"][5]
    straight = np.abs(x[5] * (d - r)) <= hl
    assert straight.sum() >= 3 and np.abs(row[straight] - (d - r)).max() < 1e-12
    # beyond the straight part a capsule's ball still shows, a cylinder's flat end is edge-on: nothing
    past = np.abs(x[5] * (d - r)) > hl + 1e-9
    if type_ == rr.CYLINDER:
        assert not R["hit"][5][past].any()
    else:
        near_end = past & (np.abs(x[5] * d) < hl + 0.9 * r)
        assert near_end.any() and R["hit"][5][near_end].all() and (row[near_end] > d - r).all()


def test_reference_convex_is_the_box_of_its_planes():
    half = np.array([0.3, 0.2, 0.1])
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * half
    planes = mesh.hull_face_planes(corners)
    pose = (2.0, 0.1, -0.2, *rcc.random_quat(np.random.default_rng(3)))
    cam = forward_camera(32, 24, fov=0.9)
    A = rr.render(one_shape(rr.CONVEX, pose, (), planes=planes), cam, None, 1, 0)
    B = rr.render(one_shape(rr.BOX, pose, tuple(half)), cam, None, 1, 0)
    assert A["hit"].sum() > 20 and np.array_equal(A["hit"], B["hit"]) and np.abs(A["t"] - B["t"]).max() < 1e-6  # (planes are stored as float32)


def test_reference_far_limit_and_occlusion():
    T = rcc.SceneTables(1)
    T.add(rr.BOX, -1, (33.0, 0, 0, 1, 0, 0, 0), (0.2, 50, 50), seg=1)   # face at 32.8 m: beyond the int16 range
    cam = forward_camera(4, 4, fov=0.2)
    assert not rr.render(T.arrays(), cam, None, 1, 0)["hit"].any()
    T.add(rr.BOX, -1, (32.9, 0, 0, 1, 0, 0, 0), (0.2, 50, 50), seg=2)   # face at 32.7 m
    R = rr.render(T.arrays(), cam, None, 1, 0)
    assert R["hit"].all() and (R["seg"] == 2).all() and (R["pos_mm"][..., 2] == -32700 + 0).all()
    assert not rr.render(T.arrays(), dict(cam, far=20.0), None, 1, 0)["hit"].any()
    T.add(rr.SPHERE, -1, (5.0, 0, 0, 1, 0, 0, 0), (0.3,), seg=3)        # in front of the wall, covering the centre only
    R = rr.render(T.arrays(), forward_camera(9, 9, fov=0.5), None, 1, 0)
    assert R["seg"][4, 4] == 3 and R["seg"][0, 0] == 2 and set(np.unique(R["seg"])) == {2, 3}


# ------------------------------------------------------------------ hull face planes
def check_planes(verts, planes, touch_tol):
    v = np.asarray(verts, dtype=np.float64)
    assert np.abs(np.linalg.norm(planes[:, :3], axis=1) - 1).max() < 1e-12
    signed = v @ planes[:, :3].T - planes[:, 3]  # [V, P]
    assert signed.max() <= 1e-9, signed.max()
    touching = (np.abs(signed) <= touch_tol).sum(axis=0)
    assert touching.min() >= 3, touching
    inside = v.mean(axis=0)
    assert ((planes[:, :3] @ inside) < planes[:, 3]).all()  # outward normals


def test_hull_face_planes_of_a_cube():
    cube = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64) * 0.02
    extra = np.array([[0.02, 0.0, 0.0], [0.0, 0.02, 0.01], [0.001, 0.002, 0.003]])  # on a face, on a face, inside
    for verts in (cube, np.concatenate([cube, extra])):
        planes = mesh.hull_face_planes(verts)
        assert planes.shape == (6, 4)
        check_planes(verts, planes, 1e-12)
        assert sorted(map(tuple, np.round(planes[:, :3]).astype(int).tolist())) == sorted([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)])
        assert np.abs(planes[:, 3] - 0.02).max() < 1e-15


def test_hull_face_planes_of_the_panda_link_hulls():
    from maniskill_amd.model.scenes import panda_tabletop_model

    A = panda_tabletop_model().arrays
    hulls = [tuple(h) for t, h in zip(A["shape_type"], A["shape_hull"]) if t == mc.SHAPE_CONVEX]
    assert len(hulls) >= 8
    for first, count in hulls:
        verts = A["hull_verts"][first : first + count].astype(np.float64)
        planes = mesh.hull_face_planes(verts)
        assert 4 <= len(planes) <= 2 * count - 4  # (Euler: a hull of V vertices has at most 2 V - 4 faces)
        # touching: within 1e-9 of the hull's size, what Qhull's own facet merging leaves between a face and its vertices
        check_planes(verts, planes, 1e-9 * max(1.0, np.abs(verts).max()) + 1e-10)


# ------------------------------------------------------------------ the scene builder on task models
@pytest.fixture(scope="module")
def backend():
    return ob.register("f64", BACKEND)


def make_env(env_id, N, backend, **kw):
    import gymnasium as gym

    import maniskill_amd.envs  # noqa: F401

    return gym.make(env_id, num_envs=N, sim_backend=backend, **kw).unwrapped


def check_scene_against_model(env, S):
    model, id_map = env.scene.model, env.segmentation_id_map
    A = model.arrays
    ns = len(A["shape_type"])
    assert all(len(S[k]) == ns for k in ("shape_type", "shape_row", "shape_frame", "shape_param", "shape_bound", "shape_seg", "shape_planes", "shape_env_slot"))
    assert np.array_equal(S["shape_row"], A["shape_row"]) and np.array_equal(S["shape_type"], A["shape_type"])
    # ids: >= 1, unique per struct, in build order (the robot's links first, then the actors as the task built them)
    ids = sorted(id_map)
    assert ids[0] == 1 and len(set(ids)) == len(ids)
    links = env.agent.robot.links
    assert [l._per_scene_id for l in links] == list(range(1, len(links) + 1))
    actors = list(env.scene.actors.values())
    assert [a._per_scene_id for a in actors] == sorted(a._per_scene_id for a in actors)
    for i in range(ns):
        owner = id_map[int(S["shape_seg"][i])]
        assert getattr(owner, "_row_name", None) == model.shape_owner[i] or owner.name == model.shape_owner[i]
        assert (-1 if owner._body_row is None else owner._body_row) == S["shape_row"][i]
        assert int(owner.per_scene_id[0]) == S["shape_seg"][i] and owner.per_scene_id.shape == (env.num_envs,)
        if S["shape_type"][i] == mc.SHAPE_CONVEX:
            first, count = S["shape_planes"][i]
            h0, hn = A["shape_hull"][i]
            signed = A["hull_verts"][h0 : h0 + hn].astype(np.float64) @ S["planes"][first : first + count, :3].T.astype(np.float64) - S["planes"][first : first + count, 3]
            assert count >= 4 and signed.max() < 1e-6 and (np.abs(signed) < 1e-6).sum(axis=0).min() >= 3
        if S["shape_type"][i] != mc.SHAPE_PLANE and S["shape_env_slot"][i] < 0:  # the bound's centre moved to the body frame
            want = geom.transform_point(A["shape_frame"][i].astype(np.float64), A["shape_bound"][i, :3].astype(np.float64))
            assert np.abs(S["shape_bound"][i, :3] - want).max() < 1e-6 and S["shape_bound"][i, 3] == A["shape_bound"][i, 3]
    # bodies without collision shapes (goal sites) have an id and no shape: invisible
    shapeless = [o for o in actors if not o.has_collision_shapes]
    assert all(o._per_scene_id not in set(S["shape_seg"].tolist()) for o in shapeless)


def test_scene_of_pick_cube(backend):
    env = make_env("PickCube-v1", 2, backend)
    try:
        S = mc.raycast_scene(env.scene.model, env._segmentation_ids_by_owner())
        check_scene_against_model(env, S)
        assert S["n_env_shape"] == 0 and (S["shape_env_slot"] == -1).all()
        assert not env.goal_site.has_collision_shapes and env.cube._per_scene_id in S["shape_seg"]
        cam = env._sensors["base_camera"]
        assert (cam.width, cam.height) == (128, 128) and abs(cam.fx - 64.0) < 1e-9 and cam.fx == cam.fy and (cam.cx, cam.cy) == (64.0, 64.0)
        assert cam._desc()["mount_row"] == -1 and cam._pos_seg is None  # (no image memory until something looks)
    finally:
        env.close()


def test_scene_of_peg_insertion_side_per_env_sizes(backend):
    N = 3
    env = make_env("PegInsertionSide-v1", N, backend)
    try:
        model = env.scene.model
        S = mc.raycast_scene(model, env._segmentation_ids_by_owner())
        check_scene_against_model(env, S)
        assert S["n_env_shape"] == model.scalars["n_env_shape"] > 0
        assert np.array_equal(S["shape_env_slot"], model.arrays["shape_env_slot"])
        for key in ("env_shape_frame", "env_shape_param", "env_shape_bound"):
            assert S[key] is model.arrays[key] or np.array_equal(S[key], model.arrays[key])
        slots = S["shape_env_slot"][S["shape_env_slot"] >= 0]
        assert sorted(slots.tolist()) == list(range(S["n_env_shape"]))
        peg = S["shape_seg"] == env.peg._per_scene_id
        assert peg.sum() == 1 and (S["shape_env_slot"][peg] >= 0).all() and (S["shape_row"][peg] == env.peg._body_row).all()
        lengths = S["env_shape_param"].reshape(-1, 4, N)[S["shape_env_slot"][peg][0], 0]
        assert len(set(np.round(lengths, 6).tolist())) == N  # every env its own peg
    finally:
        env.close()


def test_scene_builder_refuses_a_triangle_mesh_model():
    b = mc.SceneModelBuilder()
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.0]])
    tris = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]])
    b.add_actor(mc.ActorRecord("room", "static", [mc.ShapeRecord("trimesh", vertices=verts, triangles=tris)]))
    b.add_actor(mc.ActorRecord("ball", "dynamic", [mc.ShapeRecord("sphere", radius=0.1)]))
    with pytest.raises(ValueError, match="triangle-mesh"):
        mc.raycast_scene(b.compile(num_envs=1), {"room": 1, "ball": 2})


def test_wrist_camera_and_sensor_overrides(backend):
    env = make_env("PullCubeTool-v1", 2, backend, robot_uids="panda_wristcam",
                   sensor_configs=dict(width=32, base_camera=dict(height=24, fov=1.0, pose=[0.5, 0, 0.5, 0, 0, 1, 0])))
    try:
        hand, base = env._sensors["hand_camera"], env._sensors["base_camera"]
        assert list(env._sensors) == ["base_camera", "hand_camera"]
        assert hand.entity is env.agent.robot.links_map["camera_link"] and hand._desc()["mount_row"] == hand.entity._body_row
        assert (hand.width, hand.height) == (32, 128) and (base.width, base.height) == (32, 24)
        assert abs(base.fy - 24 / (2 * np.tan(0.5))) < 1e-9 and np.allclose(base._desc()["pose"], [0.5, 0, 0.5, 0, 0, 1, 0])
        P = hand.get_params()
        assert P["extrinsic_cv"].shape == (2, 3, 4) and P["cam2world_gl"].shape == (2, 4, 4) and P["intrinsic_cv"].shape == (2, 3, 3)
        # the mounted camera sits at the link: cam2world_gl's origin is the link's position, its -z the link's +x (forward)
        link = hand.entity.pose
        assert np.allclose(P["cam2world_gl"][:, :3, 3], link.p, atol=1e-6)
        fwd = link.to_transformation_matrix()[:, :3, 0]
        assert np.allclose(-P["cam2world_gl"][:, :3, 2], fwd, atol=1e-6)
        # extrinsic_cv maps the point one metre in front of the camera to (0, 0, 1)
        front = np.concatenate([(link.p + fwd).numpy(), np.ones((2, 1))], axis=1)
        assert np.allclose(np.einsum("nij,nj->ni", P["extrinsic_cv"].numpy(), front), [[0, 0, 1]] * 2, atol=1e-5)
    finally:
        env.close()


def test_obs_modes_offered_and_refused(backend):
    from maniskill_amd.envs.sapien_env import BaseEnv
    from maniskill_amd.envs.utils.observations import is_raycast_obs_mode

    modes = BaseEnv.SUPPORTED_OBS_MODES
    for m in ("state", "state_dict", "none", "depth", "segmentation", "position", "depth+segmentation", "depth+segmentation+position",
              "depth+state", "depth+segmentation+state_dict", "position+state"):
        assert m in modes, m
    assert len(modes) == 3 + 7 * 3 and len(set(modes)) == len(modes) and all(is_raycast_obs_mode(m) for m in modes[3:])
    for m in ("segmentation+depth", "state+depth", "state_dict+position+depth"):  # any order is taken
        assert is_raycast_obs_mode(m), m
    assert make_env("PickCube-v1", 1, backend, obs_mode="state").obs_mode == "state"
    for m in ("rgb", "rgbd", "pointcloud", "sensor_data", "normal", "albedo", "rgb+depth", "depth+normal", "state+state_dict+depth", "depth+depth", "state+state",
              "", "+depth"):
        assert m not in modes and not is_raycast_obs_mode(m), m
        with pytest.raises(NotImplementedError, match="colour") as err:
            make_env("PickCube-v1", 1, backend, obs_mode=m)
        assert len(str(err.value)) < 600  # (a rule, not a list of every combination)


# ------------------------------------------------------------------ validation under sanitizers
def test_raycast_desc_check_passes_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "raycast_desc_check")
    src = os.path.join(ROOT, "tests", "native", "raycast_desc_check.cpp")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", exe, src]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "raycast_desc_check: ok" in ran.stdout


# ------------------------------------------------------------------ the case tables
@pytest.mark.parametrize("name,N", rcc.CONFIGS)
def test_case_tables_are_mostly_unambiguous(name, N):
    case, ref = rcc.build(name, N), rcc.reference(name, N)
    for ci, cam in enumerate(case["cameras"]):
        shares = [float(amb.mean()) for _, amb in ref[ci]]
        print(f"{name} N={N} camera {ci} ({cam['width']} x {cam['height']}): ambiguous share at most {max(shares):.4f}")
        assert max(shares) <= rcc.MAX_AMBIGUOUS_SHARE, (name, N, ci, shares)


def test_case_tables_show_what_they_are_for():
    seen = set()
    for name, N in rcc.CONFIGS:
        case, ref = rcc.build(name, N), rcc.reference(name, N)
        seen |= {(c["width"], c["height"]) for c in case["cameras"]}
        segs = set().union(*[set(np.unique(R["seg"]).tolist()) for per_env in ref for R, _ in per_env])
        if name == "types":  # every shape type, and the per-env sphere where it exists only
            assert {0, 1, 2, 3, 4, 5, 6, 7} <= segs
            assert all((7 in np.unique(R["seg"])) == (e % 3 != 2) for e, (R, _) in enumerate(ref[0]))
            if N > 1:
                assert not np.array_equal(ref[0][0][0]["seg"], ref[0][1][0]["seg"])  # (envs differ)
        if name == "near_far":  # the ball's front is culled: it shows, but never nearer than `near`; the 40 m wall never shows
            assert {1, 2, 3, 5} <= segs and 4 not in segs
            for R, _ in ref[0]:
                assert R["t"][R["seg"] == 2].min() >= 0.6 and abs(R["t"][R["seg"] == 3].max() - 30.0) < 1e-9
                assert (~R["hit"]).any()
        if name == "many":
            assert len(case["scene"]["shape_type"]) == 72 > 64
            late = set(case["scene"]["shape_seg"][64:].tolist())  # shapes of the second staged chunk are seen
            assert late & segs and 60 in segs
            assert case["cameras"][0]["mount_row"] == 0 and "env_pose" in case["cameras"][1]
    assert seen == {(32, 24), (17, 5), (1, 1)}


def test_float32_reference_within_measured():
    worst, where = 0.0, None
    for name, N in rcc.CONFIGS:
        case, ref = rcc.build(name, N), rcc.reference(name, N)
        for ci, cam in enumerate(case["cameras"]):
            for e in range(N):
                R, amb = ref[ci][e]
                R32 = rr.render(case["scene"], cam, case["rigid"], N, e, dtype=np.float32)
                ok = ~amb
                assert np.array_equal(R32["seg"][ok], R["seg"][ok]), (name, N, ci, e)
                assert np.abs(R32["pos_mm"][ok] - R["pos_mm"][ok]).max(initial=0) <= 1
                both = ok & R["hit"]
                d = float(np.abs(R32["t"][both].astype(np.float64) - R["t"][both]).max(initial=0.0))
                if d > worst:
                    worst, where = d, (name, N, ci, e)
    print(f"largest float32 - float64 depth difference over the unambiguous pixels: {worst:.3e} m at {where}")
    assert worst <= rcc.MEASURED
    assert worst >= 0.5 * rcc.MEASURED, "MEASURED is stale: it is meant to be the measured figure, not a loose bound"
