"""The ray-cast kernel (maniskill_amd/csrc/mssim_raycast.h) against the float64 reference on the case tables of
tests/raycast_cases.py, its refusals, and the camera observations of three tasks.

On the pixels the reference does not call ambiguous: segmentation ids equal, the float depth within 4 x MEASURED
(raycast_cases.py), every int16 component within one count. Output tensors carry guard elements behind the last pixel
that must stay as they were; a second render must repeat the first bit for bit. Image sizes 32 x 24, 17 x 5 and 1 x 1
(ragged 16 x 16 tiles), N = 1, 3 and 67, a scene of 72 shapes (two staged chunks of MSSIM_RAYCAST_CHUNK = 64), two and
three cameras of different sizes in one scene."""
import numpy as np
import pytest
import torch

from maniskill_amd import native
from maniskill_amd.model import compile as mc
from tests import raycast_cases as rcc
from tests import raycast_reference as rr

pytestmark = pytest.mark.gpu

DEVICE, BACKEND = "cuda:0", "physx_cuda"
GUARD = 64
POS_FILL, DEPTH_FILL = 12345, -7.0


def make_px(N):
    """a system whose rigid_body_data has N_ROWS body rows (four free balls; the ray-cast scenes are handed in separately)"""
    from maniskill_amd.physx.system import MssimSystem

    b = mc.SceneModelBuilder()
    for k in range(rcc.N_ROWS):
        b.add_actor(mc.ActorRecord(f"body{k}", "dynamic", [mc.ShapeRecord("sphere", radius=0.05)], initial_pose=mc.geom.pose([0.5 * k, 0, 1.0])))
    px = MssimSystem(device=DEVICE, backend=BACKEND)
    px.gpu_init(b.compile(num_envs=N), N)
    return px


def device_cameras(cameras, device):
    out = []
    for c in cameras:
        c = dict(c)
        if c.get("env_pose") is not None:
            c["env_pose"] = torch.from_numpy(c["env_pose"]).to(device).contiguous()
        out.append(c)
    return out


def guarded(N, H, W, device):
    """(pos_seg view, depth view, the two flat buffers): GUARD elements behind the last pixel"""
    flat_p = torch.full((N * H * W * 4 + GUARD,), POS_FILL, dtype=torch.int16, device=device)
    flat_d = torch.full((N * H * W + GUARD,), DEPTH_FILL, dtype=torch.float32, device=device)
    return flat_p[: N * H * W * 4].view(N, H, W, 4), flat_d[: N * H * W].view(N, H, W), flat_p, flat_d


def compare(what, pos_seg, depth, per_env, tol):
    """kernel images [N, H, W, ...] (numpy) against [(float64 render, ambiguous)] per env; prints and returns the figures"""
    worst_d, worst_c, share = 0.0, 0, 0.0
    for e, (R, amb) in enumerate(per_env):
        ok = ~amb
        share = max(share, float(amb.mean()))
        seg = pos_seg[e, ..., 3].astype(np.int64)
        assert np.array_equal(seg[ok], R["seg"][ok]), (what, e, np.argwhere(ok & (seg != R["seg"]))[:4].tolist())
        if depth is not None:
            worst_d = max(worst_d, float(np.abs(depth[e][ok].astype(np.float64) - R["t"][ok]).max(initial=0.0)))
        worst_c = max(worst_c, int(np.abs(pos_seg[e, ..., :3][ok].astype(np.int64) - R["pos_mm"][ok]).max(initial=0)))
        nothing = seg == 0
        assert (pos_seg[e][nothing] == 0).all() and (depth is None or (depth[e][nothing] == 0).all()), (what, e)
    print(f"{what}: ambiguous share at most {share:.4f}, float depth off by at most {worst_d:.3e} m (allowed {tol:.3e}), int16 components by {worst_c} count")
    assert worst_d <= tol and worst_c <= 1, (what, worst_d, worst_c)
    return worst_d, worst_c, share


@pytest.mark.parametrize("name,N", rcc.CONFIGS)
def test_kernel_matches_reference_on_the_case_tables(name, N):
    case, ref = rcc.build(name, N), rcc.reference(name, N)
    px = make_px(N)
    try:
        px.cuda_rigid_body_data.torch()[:] = torch.from_numpy(case["rigid"]).to(DEVICE)
        rid = px.raycast_create(case["scene"], device_cameras(case["cameras"], DEVICE))
        for ci, cam in enumerate(case["cameras"]):
            W, H = cam["width"], cam["height"]
            pos, dep, flat_p, flat_d = guarded(N, H, W, DEVICE)
            px.raycast_render(rid, ci, pos, dep)
            first_p, first_d = flat_p.clone(), flat_d.clone()
            assert (flat_p[-GUARD:] == POS_FILL).all() and (flat_d[-GUARD:] == DEPTH_FILL).all(), "guard elements were written"
            assert not (pos == POS_FILL).all(dim=-1).any() and not (dep == DEPTH_FILL).any(), "a pixel was left unwritten"
            compare(f"{name} N={N} camera {ci} ({W} x {H})", pos.cpu().numpy(), dep.cpu().numpy(), ref[ci], 4 * rcc.MEASURED)
            # without the float depth, and again with it: the same bits
            pos2, _, flat_p2, _ = guarded(N, H, W, DEVICE)
            px.raycast_render(rid, ci, pos2, None)
            assert torch.equal(flat_p2, first_p)
            px.raycast_render(rid, ci, pos, dep)
            assert torch.equal(flat_p, first_p) and torch.equal(flat_d, first_d)
        px.raycast_destroy(rid)
        with pytest.raises(native.NativeError, match="bad id"):
            px._sim.raycast_render(rid, 0, 1, None)
    finally:
        px.close()


def test_small_shapes_far_away_are_not_lost_to_the_bounding_sphere_reject():
    """2 cm balls 20 to 31 m away through a long lens (5 mm per pixel at 30 m): the float bounding-sphere test in front of
    the exact one cancels terms of size distance^2 and must not reject a ray that hits"""
    N = 1
    T = rcc.SceneTables(N)
    for k, d in enumerate((20.0, 25.0, 29.0, 31.0)):
        T.add(rr.SPHERE, -1, (d, 0.021 * (k - 1.5), 0.004 * (k - 1.5), 1, 0, 0, 0), (0.02,), seg=k + 1)
    scene = T.arrays()
    cam = rcc.camera(32, 24, 2 * np.arctan(12 / 6000.0), pose=(0, 0, 0, 1, 0, 0, 0))
    rigid = np.zeros((rcc.N_ROWS * N, 13), dtype=np.float32)
    amb, R = rr.ambiguous(scene, cam, rigid, N, 0)
    assert set(np.unique(R["seg"]).tolist()) == {0, 1, 2, 3, 4} and all((R["seg"] == k).sum() >= 12 for k in (1, 2, 3, 4)) and amb.mean() <= rcc.MAX_AMBIGUOUS_SHARE
    px = make_px(N)
    try:
        rid = px.raycast_create(scene, [cam])
        pos, dep, _, _ = guarded(N, 24, 32, DEVICE)
        px.raycast_render(rid, 0, pos, dep)
        compare("far small balls", pos.cpu().numpy(), dep.cpu().numpy(), [(R, amb)], 4 * rcc.MEASURED)
    finally:
        px.close()


def test_refusals_come_with_a_message_and_no_scene():
    N = 2
    px = make_px(N)
    try:
        good = rcc.build("types", 3)  # (tables for three envs: only their shared parts are used below)
        cams = [rcc.camera(8, 8, 1.0, pose=(0, 0, 1, 1, 0, 0, 0))]

        def scene(**change):
            T = rcc.SceneTables(N)
            T.add(rr.PLANE, -1, (0, 0, 0, *rcc.GROUND_Q), seg=1)
            T.add(rr.SPHERE, 0, rcc.IDENT, (0.1,), seg=2)
            T.add(rr.CONVEX, 1, rcc.IDENT, seg=3, bound_r=0.5, planes=good["scene"]["planes"])
            S = T.arrays()
            for k, (i, v) in change.items():
                S[k] = S[k].copy()
                S[k][i] = v
            return S

        rid = px.raycast_create(scene(), cams)  # the unchanged scene is accepted
        px.raycast_destroy(rid)
        n_planes = len(good["scene"]["planes"])
        for change, words in ((dict(shape_type=(1, rr.TRIMESH)), "triangle mesh"), (dict(shape_row=(1, rcc.N_ROWS)), "body row"),
                              (dict(shape_planes=(2, (1, n_planes))), "plane range"), (dict(shape_planes=(2, (-1, 4))), "plane range")):
            with pytest.raises(native.NativeError, match=words) as err:
                px.raycast_create(scene(**change), cams)
            assert "raycast_create failed" in str(err.value)
        with pytest.raises(native.NativeError, match="mount row"):
            px.raycast_create(scene(), [dict(cams[0], mount_row=rcc.N_ROWS)])
        # nothing was created by the refused calls: the next id is the one after the accepted scene's
        assert px.raycast_create(scene(), cams) == rid + 1
    finally:
        px.close()


# ------------------------------------------------------------------ envs
def make_env(env_id, N, **kw):
    import gymnasium as gym

    import maniskill_amd.envs  # noqa: F401

    return gym.make(env_id, num_envs=N, sim_backend=BACKEND, **kw).unwrapped


def reference_of(env, uid):
    """[(float64 render, ambiguous)] per env of camera `uid`, from the env's own model and pose buffers"""
    cam = env._sensors[uid]
    desc = dict(cam._desc())
    if "env_pose" in desc:
        desc["env_pose"] = desc["env_pose"].cpu().numpy()
    scene = mc.raycast_scene(env.scene.model, env._segmentation_ids_by_owner())
    rigid = env.scene.px.cuda_rigid_body_data.torch().cpu().numpy()
    N = env.num_envs
    return desc, rigid, [rr.ambiguous(scene, desc, rigid, N, e)[::-1] for e in range(N)]


def check_camera(env, obs, uid, what):
    """the camera's observation against the reference: ids, int16 depth and position within a count"""
    desc, rigid, per_env = reference_of(env, uid)
    data = obs["sensor_data"][uid]
    N, H, W = env.num_envs, desc["height"], desc["width"]
    pos_seg = np.zeros((N, H, W, 4), dtype=np.int16)
    if "position" in data:
        pos_seg[..., :3] = data["position"].cpu().numpy()
    else:  # depth alone pins z; x and y are taken from the reference (compared elsewhere)
        pos_seg[..., :3] = np.stack([R["pos_mm"] for R, _ in per_env])
        pos_seg[..., 2] = -data["depth"][..., 0].cpu().numpy()
    pos_seg[..., 3] = data["segmentation"][..., 0].cpu().numpy()
    compare(what, pos_seg, None, per_env, 0.0)
    return desc, rigid, per_env


def test_pick_cube_depth_segmentation():
    N = 4
    # a narrower view, aimed at the middle of the cube's spawn square (+-0.1 m, +-9 degrees from there): the whole square is
    # in view, and at 33 pixels per unit of tan the 4 cm cube covers the pixel its centre falls in, wherever in the pixel
    pose = [float(x) for x in rcc.look_at((0.3, 0.0, 0.6), (0.0, 0.0, 0.02))]
    kw = dict(sensor_configs=dict(base_camera=dict(width=32, height=24, fov=0.7, pose=pose)))
    env = make_env("PickCube-v1", N, obs_mode="depth+segmentation", **kw)
    try:
        obs, _ = env.reset(seed=3)
        assert set(obs) == {"agent", "extra", "sensor_param", "sensor_data"} and set(obs["sensor_data"]) == {"base_camera"}
        data = obs["sensor_data"]["base_camera"]
        assert set(data) == {"depth", "segmentation"}
        for k in ("depth", "segmentation"):
            assert data[k].dtype == torch.int16 and tuple(data[k].shape) == (N, 24, 32, 1) and data[k].device.type == torch.device(DEVICE).type
        par = obs["sensor_param"]["base_camera"]
        assert tuple(par["extrinsic_cv"].shape) == (N, 3, 4) and tuple(par["cam2world_gl"].shape) == (N, 4, 4) and tuple(par["intrinsic_cv"].shape) == (N, 3, 3)
        space = env.observation_space["sensor_data"]["base_camera"]
        assert space["depth"].shape == (N, 24, 32, 1) and space["depth"].dtype == np.int16 and space["segmentation"].dtype == np.int16
        assert env.single_observation_space["sensor_data"]["base_camera"]["segmentation"].shape == (24, 32, 1)
        desc, rigid, per_env = check_camera(env, obs, "base_camera", "PickCube base_camera")
        # the cube's id where the reference projects the cube's centre; the goal site (no collision shape) nowhere
        cube_id, seg = env.cube._per_scene_id, data["segmentation"][..., 0].cpu().numpy()
        assert env.segmentation_id_map[cube_id] is env.cube
        for e in range(N):
            u, v, z = rr.project(desc, rigid, N, e, env.cube.pose.p[e].cpu().numpy())
            assert 0 <= u < 32 and 0 <= v < 24 and seg[e, int(v), int(u)] == cube_id, (e, u, v)
            assert abs(int(data["depth"][e, int(v), int(u), 0]) - 1000 * z) < 40  # (the cube's surface, 2 to 3.5 cm in front of its centre)
        table_id = next(i for i, o in env.segmentation_id_map.items() if o.name.startswith("table"))
        assert {table_id, cube_id} <= set(np.unique(seg).tolist()) and env.goal_site._per_scene_id not in np.unique(seg)  # (the goal site has no shape)
        # a partial reset moves env 2's cube: only that env's image changes
        before = {k: v.clone() for k, v in data.items()}
        obs2, _ = env.reset(seed=11, options=dict(env_idx=[2]))
        after = obs2["sensor_data"]["base_camera"]
        for k in before:
            same = [bool(torch.equal(before[k][e], after[k][e])) for e in range(N)]
            assert same == [True, True, False, True], (k, same)
        # a step renders too (the torch evaluate / reward path plus one ray-cast launch)
        obs3, rew, *_ = env.step(torch.zeros(N, *env.single_action_space.shape, device=env.device))
        assert tuple(rew.shape) == (N,) and not env._fused_ok()
        check_camera(env, obs3, "base_camera", "PickCube base_camera after a step")
        images = env.get_sensor_images()["base_camera"]
        assert images["depth"].dtype == torch.uint8 and tuple(images["depth"].shape) == (N, 24, 32, 3) and tuple(images["segmentation"].shape) == (N, 24, 32, 3)
    finally:
        env.close()


def test_state_plus_depth_carries_the_state_vector(monkeypatch):
    N = 4
    kw = dict(sensor_configs=dict(width=32, height=24))

    def pair():
        return make_env("PickCube-v1", N, obs_mode="state", **kw), make_env("PickCube-v1", N, obs_mode="state+depth", **kw)

    def run(env_s, env_v, same):
        o_s, _ = env_s.reset(seed=5)
        o_v, _ = env_v.reset(seed=5)
        assert set(o_v) == {"state", "sensor_param", "sensor_data"} and set(o_v["sensor_data"]["base_camera"]) == {"depth"}
        assert o_v["state"].shape == o_s.shape and o_v["state"].dtype == o_s.dtype and same(o_v["state"], o_s, 1e-6)
        assert env_v.single_observation_space["state"].shape == env_s.single_observation_space.shape
        for k in range(3):
            action = (0.3 - 0.2 * k) * torch.ones(N, *env_s.single_action_space.shape, device=env_s.device)
            o_s, r_s, *_ = env_s.step(action)
            o_v, r_v, *_ = env_v.step(action)
            assert same(o_v["state"], o_s, 1e-6) and same(r_v, r_s, 1e-5), k

    # both envs on the torch path (MS_FUSED=0): the same state vector and reward, bit for bit
    monkeypatch.setenv("MS_FUSED", "0")
    env_s, env_v = pair()
    try:
        assert not env_s._use_fused_callers and not env_v._use_fused_callers
        run(env_s, env_v, lambda a, b, tol: torch.equal(a, b))
    finally:
        env_s.close()
        env_v.close()
    # as shipped, the state env's outputs come from the fused epilogue and the visual env's from the torch path: the same
    # values to a float32 rounding of entries below 8 in magnitude (1e-6), the reward (a sum of a few such terms) to 1e-5
    monkeypatch.setenv("MS_FUSED", "1")
    env_s, env_v = pair()
    try:
        assert env_s._fused_ok() and not env_v._fused_ok()
        run(env_s, env_v, lambda a, b, tol: torch.allclose(a, b, atol=tol, rtol=0))
    finally:
        env_s.close()
        env_v.close()


def test_peg_insertion_side_per_env_pegs():
    env = make_env("PegInsertionSide-v1", 2, obs_mode="depth+segmentation+position", sensor_configs=dict(width=32, height=24))
    try:
        obs, _ = env.reset(seed=1)
        data = obs["sensor_data"]["base_camera"]
        assert set(data) == {"depth", "segmentation", "position"} and tuple(data["position"].shape) == (2, 24, 32, 3) and data["position"].dtype == torch.int16
        assert torch.equal(data["depth"], -data["position"][..., 2:3])
        assert not torch.equal(env.peg_half_sizes[0], env.peg_half_sizes[1])
        assert not torch.equal(data["segmentation"][0], data["segmentation"][1]) and not torch.equal(data["depth"][0], data["depth"][1])
        check_camera(env, obs, "base_camera", "PegInsertionSide base_camera")
        seg = data["segmentation"][..., 0]
        assert all((seg[e] == env.peg._per_scene_id).any() and (seg[e] == env.box._per_scene_id).any() for e in range(2))
    finally:
        env.close()


def test_pull_cube_tool_wrist_camera():
    N = 2
    env = make_env("PullCubeTool-v1", N, obs_mode="depth+segmentation", robot_uids="panda_wristcam", sensor_configs=dict(width=32, height=24))
    try:
        obs, _ = env.reset(seed=2)
        assert set(obs["sensor_data"]) == {"base_camera", "hand_camera"}
        first = {uid: {k: v.clone() for k, v in d.items()} for uid, d in obs["sensor_data"].items()}
        check_camera(env, obs, "hand_camera", "PullCubeTool hand_camera")
        check_camera(env, obs, "base_camera", "PullCubeTool base_camera")
        assert env._sensors["hand_camera"]._desc()["mount_row"] == env.agent.robot.links_map["camera_link"]._body_row
        # move the arm, nothing else: the hand camera sees something else, the base camera's pixels off the robot do not change
        robot = env.agent.robot
        q = robot.get_qpos().clone()
        q[:, 1] += 0.25
        q[:, 3] += 0.2
        robot.set_qpos(q)
        env.scene._gpu_apply_all()
        env.scene.px.gpu_update_articulation_kinematics()
        env.scene._gpu_fetch_all()
        obs2 = env.get_obs()
        check_camera(env, obs2, "hand_camera", "PullCubeTool hand_camera, arm moved")
        hand, base = obs2["sensor_data"]["hand_camera"], obs2["sensor_data"]["base_camera"]
        assert not torch.equal(hand["depth"], first["hand_camera"]["depth"])
        link_ids = torch.tensor([l._per_scene_id for l in robot.links], device=env.device)
        off_robot = ~torch.isin(first["base_camera"]["segmentation"], link_ids) & ~torch.isin(base["segmentation"], link_ids)
        assert off_robot.float().mean() > 0.3 and not off_robot.all()
        assert torch.equal(base["depth"][off_robot], first["base_camera"]["depth"][off_robot])
        assert torch.equal(base["segmentation"][off_robot], first["base_camera"]["segmentation"][off_robot])
        assert not torch.equal(base["segmentation"], first["base_camera"]["segmentation"])
    finally:
        env.close()


def test_colour_modes_still_raise():
    for mode in ("rgbd", "rgb", "pointcloud"):
        with pytest.raises(NotImplementedError, match="colour"):
            make_env("PickCube-v1", 2, obs_mode=mode)
    env = make_env("PickCube-v1", 2, obs_mode="state")
    try:
        with pytest.raises(NotImplementedError, match="colour"):
            env.render()
    finally:
        env.close()
