"""The flat-shaded view on the CPU: the float64 reference (tests/shade_reference.py) pinned by closed forms, its float32
run within a level of it, the case tables' ambiguous share, the header's routines and refusals as a stand-alone program
under ASan + UBSan, and the Python plumbing (colour tables, tiling, render modes, the video wrapper's refusals) on the
oracle backend. The kernel meets the same tables in tests/test_gpu_shade.py."""
import os
import subprocess

import numpy as np
import pytest

from maniskill_amd.model import compile as mc
from tests import oracle_backend as ob
from tests import raycast_cases as rcc
from tests import raycast_mesh_cases as rmc
from tests import raycast_reference as rr
from tests import shade_cases as sc
from tests import shade_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKEND = "oracle_f64_shade"
S3 = 1.0 / np.sqrt(3.0)


def level(k, albedo=1.0):
    return int(np.floor(255 * min(albedo * min(1.0, k), 1.0) + 0.5))


def one_shape(type_, frame, param=(), planes=None, bound_r=None, rgba=(1, 1, 1, 0)):
    T = rcc.SceneTables(1)
    T.add(type_, -1, frame, tuple(param), seg=1, planes=planes, bound_r=bound_r)
    return T.arrays(), dict(shape_rgba=np.array([rgba], dtype=np.float32))


def eye(pos, target, w=9, h=9, fov=0.3, **kw):
    return rcc.camera(w, h, fov, pose=rcc.look_at(pos, target, **kw))


def centre(R, cam):
    return R["rgb"][cam["height"] // 2, cam["width"] // 2]


def render(scene, colours, cam, **kw):
    return sr.render(scene, colours, cam, None, 1, 0, **kw)


# ------------------------------------------------------------------ the reference, by closed forms
def test_sphere_centre_pixel_faces_the_camera():
    scene, col = one_shape(rr.SPHERE, (0, 0, 1, 1, 0, 0, 0), (0.3,), rgba=(1.0, 0.5, 0.25, 0))
    # from above: n = +z, both lights: min(1, 0.3 + 1/sqrt 3 + 1) = 1
    cam = eye((0, 0, 4), (0, 0, 1), up=(1, 0, 0))
    R = render(scene, col, cam)
    assert np.allclose(R["normal"][4, 4], (0, 0, 1), atol=1e-12) and centre(R, cam).tolist() == [255, 128, 64]
    # from -x: n = -x: 0.3 + 1/sqrt 3 from the first light alone; from +x: ambient alone
    for pos, k in (((-3, 0, 1), 0.3 + S3), ((3, 0, 1), 0.3)):
        cam = eye(pos, (0, 0, 1))
        R = render(scene, col, cam)
        assert np.allclose(R["normal"][4, 4], np.sign(pos[0]) * np.array([1, 0, 0]), atol=1e-12)
        assert centre(R, cam).tolist() == [level(k), level(k, 0.5), level(k, 0.25)]
    assert (R["rgb"][0, 0] == sr.BACKGROUND).all() and not R["hit"][0, 0]


@pytest.mark.parametrize("axis,sign,k", [(0, 1, 0.3), (0, -1, 0.3 + S3), (1, 1, 0.3), (1, -1, 0.3 + S3), (2, 1, 1.0), (2, -1, 0.3)])
def test_each_box_face_under_each_light(axis, sign, k):
    """-l . n for n = +-e_axis, l0 = (1, 1, -1) / sqrt 3, l1 = (0, 0, -1): 1/sqrt 3 on -x, -y and +z, and 1 more on +z"""
    scene, col = one_shape(rr.BOX, (0, 0, 0, 1, 0, 0, 0), (0.3, 0.2, 0.1), rgba=(0.8, 0.8, 0.8, 0))
    pos = np.zeros(3)
    pos[axis] = 3.0 * sign
    cam = eye(pos, (0, 0, 0), up=(0, 0, 1) if axis != 2 else (1, 0, 0))
    R = render(scene, col, cam)
    n = np.zeros(3)
    n[axis] = sign
    assert R["hit"][4, 4] and np.allclose(R["normal"][4, 4], n, atol=1e-12) and R["part"][4, 4] == sr.FLAT
    assert centre(R, cam).tolist() == [level(k, 0.8)] * 3


def test_plane_and_ground_checker_parity():
    scene, col = one_shape(rr.PLANE, (0, 0, 0, *rcc.GROUND_Q), rgba=(1, 1, 1, 1.0))
    for x, y in ((0.5, 0.5), (1.5, 0.5), (1.5, 1.5), (-0.5, 0.5), (-0.5, -0.5), (2.5, -1.5)):
        cam = eye((x, y, 3), (x, y, 0), w=1, h=1, up=(1, 0, 0))
        R = render(scene, col, cam)
        # the plane's frame: x is the normal, the board lies in its y and z, which are the env's y and -x (GROUND_Q)
        odd = (int(np.floor(y)) + int(np.floor(-x))) % 2 == 1
        assert np.allclose(R["normal"][0, 0], (0, 0, 1), atol=1e-12)
        assert R["rgb"][0, 0].tolist() == [level(1.0, 0.8 if odd else 1.0)] * 3, (x, y)
    # a cell boundary is ambiguous, the middle of a cell is not
    amb, _ = sr.ambiguous(scene, col, eye((1.0, 0.5, 3), (1.0, 0.5, 0), w=2, h=1, up=(1, 0, 0)), None, 1, 0)
    assert not sr.ambiguous(scene, col, eye((0.5, 0.5, 3), (0.5, 0.5, 0), w=1, h=1, up=(1, 0, 0)), None, 1, 0)[0].any()
    cam = rcc.camera(1, 1, 0.3, pose=rcc.look_at((1.0, 0.5, 3), (1.0, 0.5, 0), up=(1, 0, 0)))
    assert sr.ambiguous(scene, col, cam, None, 1, 0)[0].all()


def test_cylinder_cap_against_side():
    scene, col = one_shape(rr.CYLINDER, (0, 0, 0, 1, 0, 0, 0), (0.2, 0.4))
    cam = eye((-3, 0, 0), (0, 0, 0))  # at the cap: n = -x
    R = render(scene, col, cam)
    assert np.allclose(R["normal"][4, 4], (-1, 0, 0), atol=1e-12) and R["part"][4, 4] == sr.FLAT and centre(R, cam).tolist() == [level(0.3 + S3)] * 3
    cam = eye((0, 0, 3), (0, 0, 0), up=(1, 0, 0))  # at the side from above: n = +z
    R = render(scene, col, cam)
    assert np.allclose(R["normal"][4, 4], (0, 0, 1), atol=1e-12) and R["part"][4, 4] == 0 and centre(R, cam).tolist() == [255] * 3
    cam = eye((0, -3, 0), (0, 0, 0))  # at the side from -y
    R = render(scene, col, cam)
    assert np.allclose(R["normal"][4, 4], (0, -1, 0), atol=1e-12) and centre(R, cam).tolist() == [level(0.3 + S3)] * 3
    # obliquely at the rim: the pixels split into cap and side, and the pixel on the rim is ambiguous
    cam = eye((-2, 0, 2), (-0.4, 0, 0.2), w=17, h=17, fov=0.2)
    amb, R = sr.ambiguous(scene, col, cam, None, 1, 0)
    assert {sr.FLAT, 0} <= set(np.unique(R["part"][R["hit"]]).tolist()) and amb.any() and amb.mean() < 0.2


def test_capsule_three_parts():
    scene, col = one_shape(rr.CAPSULE, (0, 0, 0, 1, 0, 0, 0), (0.2, 0.4))
    for pos, target, n, part in (((0.1, 0, 3), (0.1, 0, 0), (0, 0, 1), 0), ((-3, 0, 0), (0, 0, 0), (-1, 0, 0), 1), ((3, 0, 0), (0, 0, 0), (1, 0, 0), 2)):
        cam = eye(pos, target, up=(0, 1, 0))
        R = render(scene, col, cam)
        assert np.allclose(R["normal"][4, 4], n, atol=1e-12) and R["part"][4, 4] == part, (pos, R["normal"][4, 4], R["part"][4, 4])
    # on the ball at +x, 0.12 off the axis of the ball's centre: n = (0.6, 0, 0.8) (a 3-4-5 triangle on r = 0.2)
    cam = eye((0.52, 0, 3), (0.52, 0, 0), w=1, h=1, up=(0, 1, 0))
    R = render(scene, col, cam)
    assert np.allclose(R["normal"][0, 0], (0.6, 0, 0.8), atol=1e-9) and R["part"][0, 0] == 2
    k = 0.3 + max(0.0, -S3 * (0.6 - 0.8)) + 0.8
    assert R["rgb"][0, 0].tolist() == [level(k)] * 3


def test_hull_of_a_boxs_planes_gives_the_boxs_picture():
    half = np.array([0.3, 0.2, 0.1])
    planes = np.array([[1, 0, 0, half[0]], [-1, 0, 0, half[0]], [0, 1, 0, half[1]], [0, -1, 0, half[1]], [0, 0, 1, half[2]], [0, 0, -1, half[2]]], dtype=np.float64)
    pose = (0.1, -0.05, 0.4, *rcc.random_quat(np.random.default_rng(3)))
    cam = eye((-1.5, 0.6, 1.3), (0.1, 0, 0.4), w=32, h=24, fov=0.4)
    rgba = (0.9, 0.6, 0.3, 0.07)
    A = render(*one_shape(rr.CONVEX, pose, planes=planes, bound_r=float(np.linalg.norm(half)), rgba=rgba), cam)
    B = render(*one_shape(rr.BOX, pose, tuple(half), rgba=rgba), cam)
    assert A["hit"].sum() > 50 and np.array_equal(A["hit"], B["hit"]) and len(np.unique(B["normal"][B["hit"]].round(6), axis=0)) == 3
    assert np.allclose(A["normal"], B["normal"], atol=1e-12) and np.array_equal(A["rgb"], B["rgb"]) and len(np.unique(A["cell"])) == 3


def test_triangle_from_both_sides_is_equally_bright_under_symmetric_light():
    """a vertical triangle in the plane y = 0: seen from -y its normal is -y, from +y it is +y. The second light (straight
    down) gives nothing to either; the first gives 1/sqrt 3 to -y and nothing to +y -- so the sides differ by exactly that,
    and a triangle in the plane x = y (normal (1, -1, 0) / sqrt 2 or its opposite: l0 . n = 0) is equally bright from both"""
    def tri_scene(verts):
        T = rmc.MeshTables(1)
        T.add_mesh(-1, (0, 0, 1, 1, 0, 0, 0), T.mesh(verts, [[0, 1, 2]]), seg=1)
        return T.arrays(), dict(shape_rgba=np.array([[1, 1, 1, 0]], dtype=np.float32))

    scene, col = tri_scene([(-0.5, 0, -0.5), (0.5, 0, -0.5), (0, 0, 0.6)])
    seen = {}
    for side in (-1, 1):
        cam = eye((0, 3 * side, 1), (0, 0, 1))
        R = render(scene, col, cam)
        assert R["hit"][4, 4] and np.allclose(R["normal"][4, 4], (0, side, 0), atol=1e-12)
        seen[side] = centre(R, cam).tolist()
    assert seen[-1] == [level(0.3 + S3)] * 3 and seen[1] == [level(0.3)] * 3
    scene, col = tri_scene([(-0.5, -0.5, -0.5), (0.5, 0.5, -0.5), (0, 0, 0.6)])
    both = []
    for side in (-1, 1):
        cam = eye((3 * side, -3 * side, 1), (0, 0, 1))
        R = render(scene, col, cam)
        assert R["hit"][4, 4] and np.allclose(R["normal"][4, 4], np.array([side, -side, 0]) * np.sqrt(0.5), atol=1e-12)
        both.append(centre(R, cam).tolist())
    assert both[0] == both[1] == [level(0.3)] * 3


# ------------------------------------------------------------------ the case tables
@pytest.mark.parametrize("kind,name,N", sc.all_configs())
def test_case_tables_are_mostly_unambiguous_and_float32_is_within_a_level(kind, name, N):
    """every image used on the GPU: at most MAX_AMBIGUOUS_SHARE of its pixels ambiguous; over the others the float32 run of
    the reference is within MEASURED_LEVELS of the float64 run, channel by channel"""
    case, col, ref = sc.build(kind, name, N), sc.colours(kind, name, N), sc.reference(kind, name, N)
    worst, cells = 0, set()
    for ci, cam in enumerate(case["cameras"]):
        for e in range(N):
            R, amb = ref[ci][e]
            assert amb.mean() <= rcc.MAX_AMBIGUOUS_SHARE, (kind, name, N, ci, e, float(amb.mean()))
            R32 = sr.render(case["scene"], col, cam, case["rigid"], N, e, dtype=np.float32)
            ok = ~amb
            assert np.array_equal(R32["hit"][ok], R["hit"][ok])
            worst = max(worst, int(np.abs(R32["rgb"][ok] - R["rgb"][ok]).max(initial=0)))
            cells |= set(np.unique(R["cell"][ok]).tolist())
    print(f"{kind} {name} N={N}: float32 against float64 at most {worst} level(s)")
    assert worst <= sc.MEASURED_LEVELS
    assert {1, 2} <= cells, "the checkered shape shows both parities on unambiguous pixels"


# ------------------------------------------------------------------ the header on the host, under sanitizers
def test_shade_check_passes_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "shade_check")
    src = os.path.join(ROOT, "tests", "native", "shade_check.cpp")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", exe, src]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "shade_check: ok" in ran.stdout


# ------------------------------------------------------------------ plumbing
def test_tile_images_against_hand_made_cases():
    import torch

    from maniskill_amd.utils.visualization.misc import tile_images

    a, b, c = (np.full((4, 6, 3), v, dtype=np.uint8) for v in (10, 20, 30))
    one = tile_images([a, b, c])  # one row: side by side
    assert one.shape == (4, 18, 3) and (one[:, :6] == 10).all() and (one[:, 6:12] == 20).all() and (one[:, 12:] == 30).all()
    two = tile_images([a, b, c], nrows=2)  # two rows: a over b, then c over nothing
    assert two.shape == (8, 12, 3) and (two[:4, :6] == 10).all() and (two[4:, :6] == 20).all() and (two[:4, 6:] == 30).all() and (two[4:, 6:] == 0).all()
    small, tall = np.full((2, 3, 3), 7, dtype=np.uint8), np.full((5, 4, 3), 9, dtype=np.uint8)
    mixed = tile_images([small, tall])  # the taller first; the smaller gets a column of its own, padded with zeros
    assert mixed.shape == (5, 7, 3) and (mixed[:, :4] == 9).all() and (mixed[:2, 4:] == 7).all() and (mixed[2:, 4:] == 0).all()
    batch = tile_images([torch.full((2, 4, 6, 3), 1, dtype=torch.uint8), torch.full((2, 4, 6, 3), 2, dtype=torch.uint8)])
    assert isinstance(batch, torch.Tensor) and tuple(batch.shape) == (2, 4, 12, 3) and batch.dtype == torch.uint8 and (batch[:, :, 6:] == 2).all()


@pytest.fixture(scope="module")
def backend():
    return ob.register("f64", BACKEND)


def make_env(env_id, N, backend, **kw):
    import gymnasium as gym

    import maniskill_amd.envs  # noqa: F401

    return gym.make(env_id, num_envs=N, sim_backend=backend, **kw).unwrapped


def rows_of(model, colours, owner):
    return colours["shape_rgba"][[i for i, o in enumerate(model.shape_owner) if o == owner]]


def test_pick_cube_colour_tables(backend):
    env = make_env("PickCube-v1", 2, backend)
    try:
        model, ids = env.scene.model, env._segmentation_ids_by_owner()
        col = mc.raycast_colours(model, ids)
        assert col["shape_rgba"].shape == (int(model.scalars["n_shape"]), 4) and col["shape_rgba"].dtype == np.float32
        assert rows_of(model, col, "cube").tolist() == [[1, 0, 0, 0]]
        ground = rows_of(model, col, "ground")
        assert len(ground) == 1 and ground[0, 3] == mc.GROUND_CELL and np.allclose(ground[0, :3], mc.GROUND_GREY)
        assert np.allclose(rows_of(model, col, "table-workspace")[:, :3], mc.TABLE_WOOD)
        robot = rows_of(model, col, "panda_link3")
        assert len(robot) and (robot[:, 3] == 0).all() and (robot[:, :3] > 0.3).all()
        # the goal site has no collision shape: the viewer's scene draws its visual, green, on its own body row; the sensors' scene does not
        assert [b["owner"] for b in model.visual_bodies] == ["goal_site"]
        plain = mc.raycast_scene(model, ids, meshes=True)
        scene, vcol = mc.raycast_viewer_scene(model, ids)
        assert len(scene["shape_type"]) == len(plain["shape_type"]) + 1 == len(vcol["shape_rgba"])
        assert scene["shape_type"][-1] == rr.SPHERE and scene["shape_row"][-1] == model.row_of("goal_site") >= 0
        assert vcol["shape_rgba"][-1].tolist() == [0, 1, 0, 0] and np.isclose(scene["shape_param"][-1][0], env.goal_thresh)
        assert np.array_equal(vcol["shape_rgba"][:-1], col["shape_rgba"]) and scene["shape_seg"][-1] == env.goal_site._per_scene_id
        for key in ("shape_type", "shape_row", "shape_frame", "shape_param", "shape_bound", "shape_seg", "shape_planes", "shape_env_slot"):
            assert len(scene[key]) == len(scene["shape_type"]) and np.array_equal(np.asarray(scene[key])[:-1], np.asarray(plain[key])), key
    finally:
        env.close()


def test_lift_peg_upright_peg_carries_two_colours(backend):
    env = make_env("LiftPegUpright-v1", 2, backend)
    try:
        model, ids = env.scene.model, env._segmentation_ids_by_owner()
        assert [b["owner"] for b in model.visual_bodies] == ["peg"]
        scene, col = mc.raycast_viewer_scene(model, ids)
        peg = [i for i, o in enumerate(model.shape_owner) if o == "peg"]
        assert len(peg) == 1 and scene["shape_type"][peg[0]] == rr.NONE  # the one collision box gives way to its two halves
        halves = col["shape_rgba"][-2:, :3]
        assert scene["shape_type"][-2:].tolist() == [rr.BOX, rr.BOX] and scene["shape_row"][-2:].tolist() == [model.row_of("peg")] * 2
        assert not np.allclose(halves[0], halves[1]) and np.allclose(scene["shape_frame"][-2:, 0], [-env.peg_half_length / 2, env.peg_half_length / 2])
        assert np.allclose(scene["shape_param"][-2:, 0], env.peg_half_length / 2)
        # the sensors' table keeps the collision box, in the first half's colour
        assert np.allclose(rows_of(model, mc.raycast_colours(model, ids), "peg")[0, :3], halves[0])
    finally:
        env.close()


def test_synthetic_rooms_objects_get_per_env_colours(backend):
    env = make_env("SceneManipulation-v1", 2, backend)
    try:
        model, ids = env.scene.model, env._segmentation_ids_by_owner()
        col = mc.raycast_colours(model, ids)
        N, n_es = 2, int(model.scalars["n_env_shape"])
        assert "env_shape_rgba" in col and col["env_shape_rgba"].shape == (n_es, N, 4) and col["env_shape_rgba"].dtype == np.float32
        per_env_ids = [o for o, v in ids.items() if np.ndim(v) == 1 and len(set(np.asarray(v).tolist()) - {0}) > 1]
        assert per_env_ids, "some body row is shared by actors of the two sub-scenes"
        slots = [int(model.arrays["shape_env_slot"][i]) for i, o in enumerate(model.shape_owner) if o == per_env_ids[0]]
        assert all(s >= 0 for s in slots) and any(not np.array_equal(col["env_shape_rgba"][s, 0], col["env_shape_rgba"][s, 1]) for s in slots)
        assert np.isfinite(col["env_shape_rgba"]).all() and (col["env_shape_rgba"] >= 0).all() and (col["shape_rgba"] >= 0).all()
    finally:
        env.close()


def test_render_refusals_and_colour_observations_stay_refused(backend, tmp_path):
    from maniskill_amd.envs.sapien_env import BaseEnv
    from maniskill_amd.utils.wrappers.record import RecordEpisode

    assert "rgb" not in BaseEnv.SUPPORTED_OBS_MODES and not any("rgb" in m or "pointcloud" in m for m in BaseEnv.SUPPORTED_OBS_MODES)
    for mode in ("rgb", "rgbd", "pointcloud", "sensor_data", "normal", "albedo"):
        with pytest.raises(NotImplementedError, match="colour"):
            make_env("PickCube-v1", 1, backend, obs_mode=mode)
    env = make_env("PickCube-v1", 1, backend)
    try:
        with pytest.raises(NotImplementedError, match="colour") as err:
            env.render()
        assert all(m in str(err.value) for m in ("rgb_array", "sensors", "all"))
        with pytest.raises(NotImplementedError, match="colour"):
            env._sensors["base_camera"].get_obs(rgb=True)
        with pytest.raises(ValueError, match="render_mode"):
            RecordEpisode(env, str(tmp_path), save_video=True)
        assert env.scene.human_render_cameras == {}  # nothing was built for an env that never renders
    finally:
        env.close()
    env = make_env("PickCube-v1", 1, backend, render_mode="human")
    try:
        with pytest.raises(NotImplementedError, match="window"):
            env.render()
    finally:
        env.close()
    env = make_env("PickCube-v1", 1, backend, render_mode="rgb_array", human_render_camera_configs=dict(width=64, height=48))
    try:
        with pytest.raises(NotImplementedError, match="info_on_video"):
            RecordEpisode(env, str(tmp_path), save_video=True, info_on_video=True)
        cams = env._human_render_cameras()
        assert list(cams) == ["render_camera"] and (cams["render_camera"].width, cams["render_camera"].height) == (64, 48) and env.scene.human_render_cameras is cams
        assert cams["render_camera"]._rig is not env._sensors["base_camera"]._rig and cams["render_camera"]._rig.viewer
    finally:
        env.close()


def test_memory_guard_names_what_to_change(backend, monkeypatch):
    env = make_env("PickCube-v1", 2, backend, render_mode="rgb_array", human_render_camera_configs=dict(width=64, height=48))
    try:
        monkeypatch.setenv("MS_RENDER_MAX_BYTES", str(2 * 48 * 64 * 4 - 1))
        with pytest.raises(ValueError, match="num_envs") as err:
            env.render()
        assert "human_render_camera_configs" in str(err.value)
        assert env.RENDER_BUDGET_DEFAULT == 8 << 30 and 4096 * 512 * 512 * 4 <= env.RENDER_BUDGET_DEFAULT < 4096 * 2048 * 2048 * 4
    finally:
        env.close()
