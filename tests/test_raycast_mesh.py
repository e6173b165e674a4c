"""Triangle meshes, per-env hulls and per-env ids of the ray caster on the CPU: the mesh reference
(tests/raycast_mesh_reference.py) pinned by closed forms, the case tables (tests/raycast_mesh_cases.py: what they must
contain, at most 5 % ambiguous pixels per image, the float32 run within MEASURED_MESH of the float64 one), the scene
builder on `SceneManipulation-v1`, the Fetch's cameras, and the validation header under ASan + UBSan as a stand-alone
program. The kernel meets the same tables in tests/test_gpu_raycast_mesh.py."""
import os
import subprocess

import numpy as np
import pytest

from maniskill_amd.model import compile as mc
from tests import oracle_backend as ob
from tests import raycast_cases as rcc
from tests import raycast_mesh_cases as rmc
from tests import raycast_mesh_reference as rmr
from tests import raycast_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKEND = "oracle_f64_raycast_mesh"


def mesh_scene(verts, tris, pose=(0, 0, 0, 1, 0, 0, 0), seg=5):
    T = rmc.MeshTables(1)
    T.add_mesh(-1, pose, T.mesh(verts, tris), seg=seg)
    return T.arrays()


def rays(cam):
    u = (np.arange(cam["width"]) + 0.5 - cam["cx"]) / cam["fx"]
    v = (np.arange(cam["height"]) + 0.5 - cam["cy"]) / cam["fy"]
    return np.meshgrid(u, v)


# ------------------------------------------------------------------ closed forms
# a triangle in the plane x = d of the env frame (the camera at the origin looks along +x: x is the z-depth, y = -x_cv d, z = -y_cv d)
TRI = np.array([(0.0, -0.5, -0.4), (0.0, 0.5, -0.4), (0.0, 0.0, 0.6)])


def inside_tri(y, z):
    """closed form of TRI's interior in its plane: above the base, below the two slanted edges"""
    return (z >= -0.4) & (z - 0.6 <= 2.0 * y) & (z - 0.6 <= -2.0 * y)


@pytest.mark.parametrize("winding", ([0, 1, 2], [0, 2, 1]))
def test_reference_triangle_facing_the_camera_and_seen_from_behind(winding):
    """two-sided: either winding, and the camera on either side of the plane, sees the triangle at depth d"""
    d = 2.0
    cam = rcc.camera(21, 17, 1.0, pose=(0, 0, 0, 1, 0, 0, 0))
    x, y = rays(cam)
    want = inside_tri(-x * d, -y * d)
    for pose in ((d, 0, 0, 1, 0, 0, 0), (d, 0, 0, 0, 0, 0, 1)):  # the second turned half round about z: seen from the other side
        R = rmr.render(mesh_scene(TRI, [winding], pose=pose), cam, None, 1, 0)
        flip = pose[6] == 1
        assert np.array_equal(R["hit"], want[:, ::-1] if flip else want) and 20 <= R["hit"].sum() < R["hit"].size
        assert np.abs(R["t"][R["hit"]] - d).max() < 1e-12 and (R["t"][~R["hit"]] == 0).all()
        assert np.array_equal(R["seg"], np.where(R["hit"], 5, 0)) and set(np.unique(R["tri"]).tolist()) == {-1, 0}
        assert np.array_equal(R["pos_mm"][8, 10], [0, 0, -2000])


def test_reference_ray_past_an_edge_misses_and_the_range_applies():
    d = 2.0
    # a one-pixel camera aimed a micrometre or two inside / outside the base edge z = -0.4 (y_cv = 0.2), and the slanted edge
    # (the tables hold the corners as float32: the edge itself is known to some 1e-8)
    for y_cv, x_cv, hit in ((0.2 - 1e-6, 0.0, True), (0.2 + 1e-6, 0.0, False), (0.0, 0.15 - 1e-6, True), (0.0, 0.15 + 1e-6, False)):
        cam = dict(width=1, height=1, fx=1.0, fy=1.0, cx=0.5 - x_cv, cy=0.5 - y_cv, near=0.01, far=100.0, mount_row=-1, pose=np.array([0, 0, 0, 1, 0, 0, 0.0]))
        R = rmr.render(mesh_scene(TRI, [[0, 1, 2]], pose=(d, 0, 0, 1, 0, 0, 0)), cam, None, 1, 0)
        assert bool(R["hit"][0, 0]) == hit, (x_cv, y_cv)
    # nearer than `near`, farther than `far` or than the int16 range: nothing
    cam = rcc.camera(1, 1, 0.5, pose=(0, 0, 0, 1, 0, 0, 0), near=0.5, far=10.0)
    for dist, hit in ((0.4, False), (0.6, True), (9.9, True), (10.1, False)):
        assert bool(rmr.render(mesh_scene(TRI, [[0, 1, 2]], pose=(dist, 0, 0, 1, 0, 0, 0)), cam, None, 1, 0)["hit"][0, 0]) == hit, dist
    far = rcc.camera(1, 1, 0.5, pose=(0, 0, 0, 1, 0, 0, 0))
    assert not rmr.render(mesh_scene(40 * TRI, [[0, 1, 2]], pose=(33.0, 0, 0, 1, 0, 0, 0)), far, None, 1, 0)["hit"][0, 0]
    assert rmr.render(mesh_scene(40 * TRI, [[0, 1, 2]], pose=(32.0, 0, 0, 1, 0, 0, 0)), far, None, 1, 0)["hit"][0, 0]
    # a ray in the triangle's plane misses it: the middle row of a 3 x 3 image looks along z = 0, where this triangle lies
    flat = np.array([(2.0, -0.5, 0.0), (2.0, 0.5, 0.0), (3.0, 0.0, 0.0)])
    edge_on = rmr.render(mesh_scene(flat, [[0, 1, 2]]), rcc.camera(3, 3, 0.5, pose=(0, 0, 0, 1, 0, 0, 0)), None, 1, 0)
    assert not edge_on["hit"].any()


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
def test_reference_shared_edge_is_hit(dtype):
    """rays aimed exactly at points of the edge two triangles share (and at their shared corners) hit one of them, in both
    precisions; behind the pair stands a wall 3 m farther that a hole would show"""
    quad = np.array([(0.0, -0.5, -0.5), (0.0, 0.5, -0.5), (0.0, 0.5, 0.5), (0.0, -0.5, 0.5)])
    T = rmc.MeshTables(1)
    T.add_mesh(-1, (2.0, 0, 0, *rcc.random_quat(np.random.default_rng(3)) * [1, 0.05, 0.05, 0.05]), T.mesh(quad, [[0, 1, 2], [0, 2, 3]]), seg=5)
    T.add(rr.BOX, -1, (5.5, 0, 0, 1, 0, 0, 0), (0.5, 4, 4), seg=9)
    S = T.arrays()
    Rs, ps = rmr.shape_pose(S, 0, None, 1, 0, np.float64)
    for s in np.linspace(0.0, 1.0, 41):  # along the diagonal from corner 0 to corner 2, the ends included
        p = ps + Rs @ (quad[0] + s * (quad[2] - quad[0]))
        x_cv, y_cv = -p[1] / p[0], -p[2] / p[0]
        cam = dict(width=1, height=1, fx=1.0, fy=1.0, cx=0.5 - x_cv, cy=0.5 - y_cv, near=0.01, far=100.0, mount_row=-1, pose=np.array([0, 0, 0, 1, 0, 0, 0.0]))
        R = rmr.render(S, cam, None, 1, 0, dtype=dtype)
        assert R["seg"][0, 0] == 5 and abs(R["t"][0, 0] - p[0]) < (1e-9 if dtype is np.float64 else 1e-5), (s, R["seg"][0, 0], R["t"][0, 0])


def test_reference_brute_force_agrees_with_the_box_it_triangulates():
    """the 12 triangles of a box from outside: the same image as the analytic box, which raycast_reference pins"""
    half = (0.3, 0.2, 0.25)
    pose = (2.0, 0.1, -0.1, *rcc.random_quat(np.random.default_rng(4)))
    cam = rcc.camera(32, 24, 0.8, pose=(0, 0, 0, 1, 0, 0, 0))
    T = rcc.SceneTables(1)
    T.add(rr.BOX, -1, pose, half, seg=5)
    A, M = rr.render(T.arrays(), cam, None, 1, 0), rmr.render(mesh_scene(*rmc.box_mesh(half), pose=pose), cam, None, 1, 0)
    assert np.array_equal(A["hit"], M["hit"]) and A["hit"].sum() > 50 and np.abs(A["t"] - M["t"]).max() < 1e-7  # (float32 corners in the mesh tables)


# ------------------------------------------------------------------ the case tables
@pytest.mark.parametrize("name,N", rmc.CONFIGS)
def test_case_tables_are_mostly_unambiguous(name, N):
    case, ref = rmc.build(name, N), rmc.reference(name, N)
    for ci, cam in enumerate(case["cameras"]):
        shares = [float(amb.mean()) for _, amb in ref[ci]]
        print(f"{name} N={N} camera {ci} ({cam['width']} x {cam['height']}): ambiguous share at most {max(shares):.4f}")
        assert max(shares) <= rcc.MAX_AMBIGUOUS_SHARE, (name, N, ci, shares)


def test_case_tables_show_what_they_are_for():
    seen, sizes = set(), set()
    for name, N in rmc.CONFIGS:
        case, ref = rmc.build(name, N), rmc.reference(name, N)
        S, M = case["scene"], case["meshes"]
        seen |= {(c["width"], c["height"]) for c in case["cameras"]}
        sizes.add(N)
        segs = set().union(*[set(np.unique(R["seg"]).tolist()) for per_env in ref for R, _ in per_env])
        height = lambda m: rmc.bvh_height(S["tri_bvh"], m[2])
        if name == "meshes":
            assert [M[k][1] for k in ("one", "box", "fan")] == [1, 12, 17] and [height(M[k]) for k in ("one", "box", "fan")] == [1, 1, 2]
            assert {0, 1, 2, 3, 4, 5} <= segs
            box = S["shape_seg"].tolist().index(3)
            assert S["shape_row"][box] == 0 and S["shape_type"][box] == rr.TRIMESH     # on a body row, tilted differently per env
            assert all(abs(abs(case["rigid"][e, 3]) - 1) > 1e-3 for e in range(N))
            for e, (R, _) in enumerate(ref[0]):
                here = set(np.unique(R["seg"]).tolist())
                assert (6 in here) == (e % 3 != 2) and (7 in here) == ((e + 1) % 3 != 2), e   # the per-env mesh / hull where they exist only
                assert 20 + e % 5 in here and not ({20, 21, 22, 23, 24} - {20 + e % 5}) & here  # the per-env id of this env alone
            if N >= 3:
                slot_mesh, slot_hull = S["shape_env_slot"][S["shape_seg"].tolist().index(6)], S["shape_env_slot"][S["shape_seg"].tolist().index(7)]
                ep = S["env_shape_param"].reshape(-1, 4, N)
                assert ep[slot_mesh, 3, :3].tolist() == [rr.TRIMESH + 1, rr.TRIMESH + 1, rr.NONE + 1] and ep[slot_mesh, 0, 0] != ep[slot_mesh, 0, 1]
                pl = S["env_shape_planes"].reshape(-1, 2, N)[slot_hull]
                assert ep[slot_hull, 3, :3].tolist() == [rr.CONVEX + 1, rr.NONE + 1, rr.CONVEX + 1] and pl[0, 0] != pl[0, 2]
                # the two per-env meshes and the two hulls give different images
                assert not np.array_equal(ref[0][0][0]["seg"] == 6, ref[0][1][0]["seg"] == 6) and not np.array_equal(ref[0][0][0]["seg"] == 7, ref[0][2][0]["seg"] == 7)
        if name == "terrain":
            assert M["field"][1] >= 300 and height(M["field"]) == 3 and {1, 2} <= segs
        if name == "inside":  # every pixel sees the room's wall (from inside: back faces) or what stands in it
            assert M["room"][1] == 12 and {1, 2, 3} <= segs and all(R["hit"].all() for per_env in ref for R, _ in per_env)
            room = np.asarray(S["shape_frame"][0][:3], dtype=np.float64)
            assert np.abs(np.asarray(case["cameras"][0]["pose"][:3]) - room).max() < 0.8   # the camera is inside the 3 x 2.4 x 1.6 m box
        if name == "many":
            assert len(S["shape_type"]) == 72 > 64 and S["shape_type"][71] == rr.TRIMESH and 60 in segs
    assert seen == {(32, 24), (17, 5), (1, 1)} and sizes == {1, 3, 67}


def test_float32_reference_within_measured():
    worst, where = 0.0, None
    for name, N in rmc.CONFIGS:
        case, ref = rmc.build(name, N), rmc.reference(name, N)
        for ci, cam in enumerate(case["cameras"]):
            for e in range(N):
                R, amb = ref[ci][e]
                R32 = rmr.render(case["scene"], cam, case["rigid"], N, e, dtype=np.float32)
                ok = ~amb
                assert np.array_equal(R32["seg"][ok], R["seg"][ok]), (name, N, ci, e)
                assert np.abs(R32["pos_mm"][ok] - R["pos_mm"][ok]).max(initial=0) <= 1
                both = ok & R["hit"]
                d = float(np.abs(R32["t"][both].astype(np.float64) - R["t"][both]).max(initial=0.0))
                if d > worst:
                    worst, where = d, (name, N, ci, e)
    print(f"largest float32 - float64 depth difference over the unambiguous pixels: {worst:.3e} m at {where}")
    assert worst <= rmc.MEASURED_MESH
    assert worst >= 0.5 * rmc.MEASURED_MESH, "MEASURED_MESH is stale: it is meant to be the measured figure, not a loose bound"


# ------------------------------------------------------------------ the scene builder on the rooms
@pytest.fixture(scope="module")
def backend():
    return ob.register("f64", BACKEND)


def make_env(env_id, N, backend, **kw):
    import gymnasium as gym

    import maniskill_amd.envs  # noqa: F401

    return gym.make(env_id, num_envs=N, sim_backend=backend, **kw).unwrapped


def test_scene_of_the_rooms(backend):
    N = 5
    env = make_env("SceneManipulation-v1", N, backend, build_config_idxs=list(range(N)))
    try:
        model, A = env.scene.model, env.scene.model.arrays
        ids = env._segmentation_ids_by_owner()
        with pytest.raises(ValueError, match="triangle-mesh"):
            mc.raycast_scene(model, ids)
        S = mc.raycast_scene(model, ids, meshes=True)
        ns, n_es = len(A["shape_type"]), int(model.scalars["n_env_shape"])
        # table lengths
        assert all(len(S[k]) == ns for k in ("shape_type", "shape_row", "shape_frame", "shape_param", "shape_bound", "shape_seg", "shape_planes", "shape_env_slot"))
        assert S["tri_soup"].shape == (model.scalars["n_tri"], 12) and S["tri_bvh"].shape == (model.scalars["n_tri_node"], 112) and len(S["tri_soup"]) > 0
        assert S["n_env_shape"] == n_es > 0 and S["env_shape_planes"].shape == (2 * n_es, N) and S["env_shape_seg"].shape == (n_es, N)
        assert S["env_shape_planes"].dtype == np.int32 and S["env_shape_seg"].dtype == np.int16
        ep = A["env_shape_param"].reshape(n_es, 4, N)
        # the scenery: two mesh slots whose mesh differs from env to env, named by first triangle, count and root node
        id_map = env.segmentation_id_map
        names = {i: o.name for i, o in id_map.items()}
        for part in ("walls", "furniture"):
            (i,) = [k for k in range(ns) if names.get(int(S["shape_seg"][k])) == part]
            assert S["shape_type"][i] == mc.SHAPE_TRIMESH and S["shape_row"][i] == -1 and S["shape_env_slot"][i] >= 0
            assert S["shape_param"][i, 2] == A["shape_hull"][i, 0] and S["shape_param"][i, 1] == A["shape_hull"][i, 1]
            rows = ep[S["shape_env_slot"][i]]
            assert (rows[3] == mc.SHAPE_TRIMESH + 1).all() and len(set(rows[0].tolist())) == N
            assert (rows[0] + rows[1] <= len(S["tri_soup"])).all() and (rows[2] < len(S["tri_bvh"])).all()
        # the movable objects: per-env plane ranges are the planes of the hull each env really has, per-env ids the owner's
        pl = S["env_shape_planes"].reshape(n_es, 2, N)
        movable = [a for a in env.scene.actors.values() if getattr(a, "_row_name", None) is not None]
        assert len(movable) == 2 * N and len({a._per_scene_id for a in movable}) == 2 * N
        checked = 0
        for i in range(ns):
            slot = S["shape_env_slot"][i]
            if slot < 0 or S["shape_type"][i] != mc.SHAPE_CONVEX:
                continue
            owners = [a for a in movable if a._row_name == model.shape_owner[i]]
            assert len(owners) == N  # one object per layout on this row
            for e in range(N):
                (owner,) = [a for a in owners if e in a._own_idx.tolist()]
                if ep[slot, 3, e] == mc.SHAPE_NONE + 1:  # (this env's object has fewer parts)
                    continue
                assert ep[slot, 3, e] == mc.SHAPE_CONVEX + 1
                assert S["env_shape_seg"][slot, e] == owner._per_scene_id == int(owner.per_scene_id[e]) and id_map[owner._per_scene_id] is owner
                first, count = pl[slot, :, e]
                v0, vn = int(ep[slot, 0, e]), int(ep[slot, 1, e])
                signed = A["hull_verts"][v0 : v0 + vn].astype(np.float64) @ S["planes"][first : first + count, :3].T.astype(np.float64) - S["planes"][first : first + count, 3]
                assert count >= 4 and signed.max() < 1e-6 and (np.abs(signed) < 1e-6).sum(axis=0).min() >= 3, (i, e)
                checked += 1
        assert checked >= 4 * N
        assert len({tuple(pl[s, :, e]) for s in range(n_es) for e in range(N)}) > 10  # the hulls do differ from env to env
        # the same hull is stored once: plane ranges are disjoint or equal
        ranges = sorted({(int(a), int(b)) for a, b in np.concatenate([S["shape_planes"], pl.transpose(0, 2, 1).reshape(-1, 2)]) if b > 0})
        assert all(a0 + n0 <= a1 for (a0, n0), (a1, _) in zip(ranges, ranges[1:])) and ranges[-1][0] + ranges[-1][1] == len(S["planes"])
        assert {"walls", "furniture", "ground"} <= set(names.values()) and {a.name for a in movable} <= set(names.values())
    finally:
        env.close()


def test_fetch_camera_configs(backend):
    env = make_env("Empty-v1", 2, backend, robot_uids="fetch")
    try:
        assert list(env._sensors) == ["base_camera", "fetch_head", "fetch_hand"]
        links = env.agent.robot.links_map
        head, hand = env._sensors["fetch_head"], env._sensors["fetch_hand"]
        for cam, link, p in ((head, "head_camera_link", [0, 0, 0]), (hand, "gripper_link", [-0.1, 0, 0.1])):
            assert (cam.width, cam.height) == (128, 128) and abs(cam.fx - 64 / np.tan(1.0)) < 1e-9 and cam.fx == cam.fy and (cam.cx, cam.cy) == (64.0, 64.0)
            assert cam.config.fov == 2 and cam.config.near == 0.01 and cam.config.far == 100
            assert cam.entity is links[link] and cam._desc()["mount_row"] == links[link]._body_row
            assert np.allclose(cam._desc()["pose"], [*p, 1, 0, 0, 0])
        from maniskill_amd.envs.sapien_env import BaseEnv

        assert env.SUPPORTED_OBS_MODES is BaseEnv.SUPPORTED_OBS_MODES and len(BaseEnv.SUPPORTED_OBS_MODES) == 3 + 7 * 3
    finally:
        env.close()


def test_scene_manipulation_cameras_by_robot(backend):
    env = make_env("SceneManipulation-v1", 2, backend, robot_uids="panda", scene_builder_cls="SyntheticRoomsStatic", build_config_idxs=[0, 2])
    try:
        assert list(env._sensors) == ["base_camera"] and env._sensors["base_camera"]._desc()["mount_row"] == -1
        S = mc.raycast_scene(env.scene.model, env._segmentation_ids_by_owner(), meshes=True)
        assert (S["shape_type"] == mc.SHAPE_TRIMESH).sum() == 2 and "env_shape_seg" not in S and "env_shape_planes" not in S
    finally:
        env.close()
    env = make_env("SceneManipulation-v1", 2, backend, build_config_idxs=[1, 3])
    try:
        assert list(env._sensors) == ["fetch_head", "fetch_hand"]
    finally:
        env.close()


# ------------------------------------------------------------------ validation under sanitizers
def test_raycast_mesh_desc_check_passes_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "raycast_mesh_desc_check")
    src = os.path.join(ROOT, "tests", "native", "raycast_mesh_desc_check.cpp")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", exe, src]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "raycast_mesh_desc_check: ok" in ran.stdout
