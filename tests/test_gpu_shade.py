"""The shading kernel (maniskill_amd/csrc/mssim_raycast_shade.h, k_raycast_shade<false / true>) against the float64
reference (tests/shade_reference.py) on the case tables of tests/shade_cases.py, its refusals, render() of two envs and
an episode video.

On the pixels the reference does not call ambiguous every channel is within ONE level. That bound is derived, not
measured: a unit normal and two dot products in float32 are some 1e-6 of full scale off, far below one level, so the
rounding to a byte can move by at most one. Alpha is 255 everywhere, pixels the reference calls empty carry the background
colour exactly, GUARD bytes behind the last pixel stay as they were, no pixel is left unwritten, a second launch repeats
the first bit for bit, and a depth render of the same scene before and after the shading launch is bit-identical. The
picture and the depth image come from one walk of the shapes, so on EVERY pixel, the ambiguous ones included, the
background colour stands exactly where the float depth is 0."""
import numpy as np
import pytest
import torch

from maniskill_amd import native
from tests import raycast_reference as rr
from tests import shade_cases as sc
from tests import shade_reference as sr
from tests.test_gpu_raycast import DEVICE, device_cameras, guarded, make_env, make_px

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0x5B  # (no picture has all four bytes of a pixel at this value: alpha is 255)


def guarded_rgba(N, H, W):
    flat = torch.full((N * H * W * 4 + GUARD,), FILL, dtype=torch.uint8, device=DEVICE)
    return flat[: N * H * W * 4].view(N, H, W, 4), flat


def compare(what, rgba, per_env):
    """kernel picture [N, H, W, 4] (numpy) against [(float64 picture, ambiguous)] per env; prints and returns the figures"""
    worst, off_by_one, counted, share = 0, 0, 0, 0.0
    assert (rgba[..., 3] == 255).all(), what
    for e, (R, amb) in enumerate(per_env):
        ok = ~amb
        share = max(share, float(amb.mean()))
        got = rgba[e, ..., :3].astype(np.int64)
        empty = ok & ~R["hit"]
        assert (got[empty] == np.array(sr.BACKGROUND)).all(), (what, e, "a pixel the reference calls empty is not the background colour")
        d = np.abs(got[ok] - R["rgb"][ok])
        worst, off_by_one, counted = max(worst, int(d.max(initial=0))), off_by_one + int((d.max(axis=-1) == 1).sum()), counted + int(ok.sum())
        assert d.max(initial=0) <= 1, (what, e, np.argwhere(ok & (np.abs(got - R["rgb"]).max(-1) > 1))[:4].tolist())
    print(f"{what}: ambiguous share at most {share:.4f}, channels off by at most {worst} level, {off_by_one} of {counted} pixels ({off_by_one / max(counted, 1):.4%}) off by exactly one")
    return worst


def can_shade_to_background(col):
    """whether some colour of the tables, plain or dimmed by the checker, gives the background's bytes at some light level k
    in [AMBIENT, 1] -- with a level to spare on every channel for the kernel's float32: |255 a k - background| <= 1.5"""
    rows = [col["shape_rgba"]] + ([col["env_shape_rgba"].reshape(-1, 4)] if "env_shape_rgba" in col else [])
    a = np.concatenate(rows)[:, :3].astype(np.float64)
    a = np.concatenate([a, sr.CHECKER_DIM * a])
    bg = np.array(sr.BACKGROUND, dtype=np.float64)
    lo, hi = ((bg - 1.5) / (255 * a)).max(axis=1), ((bg + 1.5) / (255 * a)).min(axis=1)
    return bool((np.maximum(lo, sr.AMBIENT) <= np.minimum(hi, 1.0)).any())


@pytest.mark.parametrize("kind,name,N", sc.all_configs())
def test_kernel_matches_reference_on_the_case_tables(kind, name, N):
    case, col, ref = sc.build(kind, name, N), sc.colours(kind, name, N), sc.reference(kind, name, N)
    assert not can_shade_to_background(col), "a surface of this case could carry the background colour: the second direction below would not hold"
    px = make_px(N)
    try:
        px.cuda_rigid_body_data.torch()[:] = torch.from_numpy(case["rigid"]).to(DEVICE)
        rid = px.raycast_create(case["scene"], device_cameras(case["cameras"], DEVICE))
        px.raycast_set_colours(rid, col["shape_rgba"], col.get("env_shape_rgba"))
        for ci, cam in enumerate(case["cameras"]):
            W, H = cam["width"], cam["height"]
            pos, dep, flat_p, flat_d = guarded(N, H, W, DEVICE)
            px.raycast_render(rid, ci, pos, dep)
            depth_before = (flat_p.clone(), flat_d.clone())
            rgba, flat = guarded_rgba(N, H, W)
            px.raycast_shade(rid, ci, rgba)
            first = flat.clone()
            assert (flat[-GUARD:] == FILL).all(), "guard bytes were written"
            assert not (rgba == FILL).all(dim=-1).any(), "a pixel was left unwritten"
            compare(f"{kind} {name} N={N} camera {ci} ({W} x {H})", rgba.cpu().numpy(), ref[ci])
            # one walk for both images: the background colour exactly where the depth camera hit nothing, and nowhere else
            is_background = (rgba == torch.tensor(sr.BACKGROUND + (255,), dtype=torch.uint8, device=DEVICE)).all(dim=-1)
            assert torch.equal(is_background, dep == 0), (kind, name, N, ci, (is_background != (dep == 0)).nonzero()[:4].tolist())
            rgba2, flat2 = guarded_rgba(N, H, W)
            px.raycast_shade(rid, ci, rgba2)
            assert torch.equal(flat2, first), "a second launch differs"
            px.raycast_render(rid, ci, pos, dep)
            assert torch.equal(flat_p, depth_before[0]) and torch.equal(flat_d, depth_before[1]), "the depth render changed across the shading launch"
        px.raycast_destroy(rid)
        with pytest.raises(native.NativeError, match="bad id"):
            px._sim.raycast_shade(rid, 0, rgba.data_ptr())
    finally:
        px.close()


def test_refusals_come_with_a_message_and_the_scene_still_renders():
    N = 2
    case, col = sc.build("plain", "types", 3), sc.colours("plain", "types", 3)  # (shared tables only: the slot's per-env rows are cut to N below)
    scene = dict(case["scene"])
    for key in ("env_shape_frame", "env_shape_param", "env_shape_bound"):
        scene[key] = np.ascontiguousarray(scene[key][:, :N])
    cams = [dict(case["cameras"][0])]
    px = make_px(N)
    try:
        px.cuda_rigid_body_data.torch()[:] = torch.from_numpy(case["rigid"][np.arange(4)[:, None] * 3 + np.arange(N)].reshape(-1, 13)).to(DEVICE)
        rid = px.raycast_create(scene, cams)
        rgba, flat = guarded_rgba(N, 24, 32)
        with pytest.raises(native.NativeError, match="no colours were set"):
            px.raycast_shade(rid, 0, rgba)
        assert (flat == FILL).all()
        bad = col["shape_rgba"].copy()
        bad[2, 1] = np.nan
        with pytest.raises(native.NativeError, match="shape 2"):
            px.raycast_set_colours(rid, bad)
        bad[2, 1] = -0.5
        with pytest.raises(native.NativeError, match="negative or not finite"):
            px.raycast_set_colours(rid, bad)
        with pytest.raises(native.NativeError, match="no colours were set"):  # (a refused table sets nothing)
            px.raycast_shade(rid, 0, rgba)
        with pytest.raises(native.NativeError, match="bad id"):
            px._sim.raycast_set_colours(rid + 7, col["shape_rgba"])
        px.raycast_set_colours(rid, col["shape_rgba"])
        with pytest.raises(native.NativeError, match="bad id"):
            px._sim.raycast_shade(rid + 7, 0, rgba.data_ptr())
        with pytest.raises(native.NativeError, match="bad camera"):
            px._sim.raycast_shade(rid, 3, rgba.data_ptr())
        with pytest.raises(native.NativeError, match="4-byte aligned"):
            px._sim.raycast_shade(rid, 0, rgba.data_ptr() + 1)
        assert (flat == FILL).all(), "a refused call wrote something"
        # a scene without per-env slots takes no per-env table
        T = sc.rcc.SceneTables(N)
        T.add(rr.SPHERE, 0, sc.rcc.IDENT, (0.1,), seg=2)
        rid2 = px.raycast_create(T.arrays(), cams)
        with pytest.raises(native.NativeError, match="without per-env"):
            px._sim.raycast_set_colours(rid2, np.ones((1, 4), dtype=np.float32), np.ones((1, N, 4), dtype=np.float32))
        # after all that the first scene still renders, depth and picture
        pos, dep, _, _ = guarded(N, 24, 32, DEVICE)
        px.raycast_render(rid, 0, pos, dep)
        px.raycast_shade(rid, 0, rgba)
        assert (dep > 0).any() and (rgba[..., 3] == 255).all() and len(torch.unique(rgba[..., :3].reshape(-1, 3), dim=0)) > 4
    finally:
        px.close()


# ------------------------------------------------------------------ envs
def human_camera_desc(env, uid="render_camera"):
    return dict(env.scene.human_render_cameras[uid]._desc())


def test_pick_cube_render_modes():
    N = 2
    kw = dict(human_render_camera_configs=dict(width=64, height=48))
    env = make_env("PickCube-v1", N, render_mode="rgb_array", **kw)
    try:
        env.reset(seed=3)
        assert env.scene.human_render_cameras == {}
        frame = env.render()
        assert frame.dtype == torch.uint8 and tuple(frame.shape) == (N, 48, 64, 3) and frame.device.type == torch.device(DEVICE).type
        pic = frame.cpu().numpy().astype(np.int64)
        desc, rigid = human_camera_desc(env), env.scene.px.cuda_rigid_body_data.torch().cpu().numpy()
        for e in range(N):
            u, v, _ = rr.project(desc, rigid, N, e, env.cube.pose.p[e].cpu().numpy())
            r, g, b = pic[e, int(v), int(u)]
            assert 0 <= u < 64 and 0 <= v < 48 and r >= 70 and r > 3 * max(g, b), (e, u, v, (r, g, b))  # the cube is (1, 0, 0); ambient alone gives 77
            green = (pic[e, ..., 1] >= 70) & (pic[e, ..., 1] > 3 * np.maximum(pic[e, ..., 0], pic[e, ..., 2]))
            assert green.any(), (e, "the goal site is green in rgb_array")
        assert not np.array_equal(pic[0], pic[1])
        assert torch.equal(env.render_rgb_array("render_camera"), frame)
        # sensors: each sensor's shaded picture beside its depth and segmentation pictures; no goal site in any of them
        sensors = env.render_sensors()
        assert sensors.dtype == torch.uint8 and tuple(sensors.shape) == (N, 128, 3 * 128, 3)
        shaded = sensors[:, :, :128].cpu().numpy().astype(np.int64)
        green = (shaded[..., 1] >= 70) & (shaded[..., 1] > 3 * np.maximum(shaded[..., 0], shaded[..., 2]))
        red = (shaded[..., 0] >= 70) & (shaded[..., 0] > 3 * np.maximum(shaded[..., 1], shaded[..., 2]))
        assert not green.any() and all(red[e].any() for e in range(N))
        assert env.goal_site._per_scene_id not in torch.unique(env._sensors["base_camera"].get_obs()["segmentation"]).tolist()
        with pytest.raises(NotImplementedError, match="colour"):
            env._sensors["base_camera"].get_obs(rgb=True)
        # a step moves the robot: the next frame differs
        env.step(0.5 * torch.ones(N, *env.single_action_space.shape, device=env.device))
        assert not torch.equal(env.render(), frame)
    finally:
        env.close()
    env = make_env("PickCube-v1", N, render_mode="all", **kw)
    try:
        env.reset(seed=3)
        both = env.render()
        assert both.dtype == torch.uint8 and tuple(both.shape) == (N, 128, 3 * 128 + 64, 3)
        assert torch.equal(both[:, :, : 3 * 128], env.render_sensors()) and torch.equal(both[:, :48, 3 * 128 :], env.render_rgb_array())
        assert (both[:, 48:, 3 * 128 :] == 0).all()
    finally:
        env.close()


def test_scene_manipulation_with_the_fetch_is_shaded_by_the_mesh_variant():
    from maniskill_amd.model import compile as mc

    N = 2
    env = make_env("SceneManipulation-v1", N, render_mode="rgb_array", build_config_idxs=[0, 1], human_render_camera_configs=dict(width=96, height=96))
    try:
        env.reset(seed=4)
        frame = env.render()
        assert tuple(frame.shape) == (N, 96, 2 * 96, 3) and frame.dtype == torch.uint8  # the room camera beside the one on the robot
        model, ids = env.scene.model, env._segmentation_ids_by_owner()
        scene, col = mc.raycast_viewer_scene(model, ids)
        assert (np.asarray(scene["shape_type"]) == rr.TRIMESH).any() and "env_shape_rgba" in col  # meshes and per-env colours: k_raycast_shade<true>
        room = frame[:, :, :96].cpu().numpy().astype(np.int64)
        # against the reference, pixel for pixel, through the mesh variant
        desc, rigid = human_camera_desc(env), env.scene.px.cuda_rigid_body_data.torch().cpu().numpy()
        hit_shapes = [set() for _ in range(N)]
        for e in range(N):
            amb, R = sr.ambiguous(scene, col, desc, rigid, N, e)
            ok = ~amb
            print(f"SceneManipulation room camera, env {e}: ambiguous share {amb.mean():.4f}")
            assert np.abs(room[e][ok] - R["rgb"][ok]).max() <= 1, e
            hit_shapes[e] = set(np.unique(R["shape"][ok & R["hit"]]).tolist())
            # walls are shaded: more than one brightness of the wall colour; the ground shows both parities of its checker
            walls = [i for i, o in enumerate(model.shape_owner) if o == "walls"]
            wall_px = ok & np.isin(R["shape"], walls)
            assert wall_px.sum() > 50 and len(np.unique(room[e][wall_px], axis=0)) >= 2, e
            assert {1, 2} <= set(np.unique(R["cell"][ok]).tolist()), (e, "the ground checker")
            ground = ok & (R["cell"] > 0)
            assert len(np.unique(room[e][ground], axis=0)) >= 2
        # the movable objects of the two sub-scenes: their own colours, different from each other
        movable = [o for o in env.segmentation_id_map.values() if getattr(o, "_row_name", None) is not None]
        colours = {o.name: tuple(col["env_shape_rgba"][int(model.arrays["shape_env_slot"][model.shape_owner.index(o._row_name)]), int(o._own_idx[0])][:3].round(4)) for o in movable}
        assert len(movable) == 2 * N and len(set(colours.values())) == len(colours), colours
    finally:
        env.close()


def test_record_episode_writes_one_video_of_six_frames(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from maniskill_amd.utils.visualization.misc import video_backend
    from maniskill_amd.utils.wrappers.record import RecordEpisode
    from maniskill_amd.vector.wrappers.gymnasium import ManiSkillVectorEnv

    import gymnasium as gym

    import maniskill_amd.envs  # noqa: F401

    N = 2
    env = gym.make("PickCube-v1", num_envs=N, sim_backend="physx_cuda", render_mode="rgb_array", human_render_camera_configs=dict(width=64, height=48))
    rec = RecordEpisode(env, str(tmp_path), save_trajectory=False, save_video=True, video_fps=10)
    try:
        rec.reset(seed=1)
        for _ in range(5):
            # (the arm keeps moving: an animated PNG merges frames that repeat the one before)
            rec.step(0.5 * torch.ones(N, *env.unwrapped.single_action_space.shape, device=env.unwrapped.device))
    finally:
        rec.close()
    videos = sorted(p.name for p in tmp_path.iterdir() if p.suffix in (".png", ".mp4"))
    assert len(videos) == 1, videos
    if video_backend() == "pil":
        with Image.open(tmp_path / videos[0]) as im:
            assert getattr(im, "n_frames", 1) == 6 and im.size == (N * 64, 48)
    # the vector env passes render() through
    venv = ManiSkillVectorEnv(gym.make("PickCube-v1", num_envs=N, sim_backend="physx_cuda", render_mode="rgb_array", human_render_camera_configs=dict(width=64, height=48)), auto_reset=False)
    try:
        venv.reset(seed=1)
        assert tuple(venv.render().shape) == (N, 48, 64, 3)
    finally:
        venv.close()
