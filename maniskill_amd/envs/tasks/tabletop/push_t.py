"""PushT-v1 (task definition restated from mani_skill/envs/tasks/tabletop/push_t.py:20-538): push a T-shaped block
with the panda_stick into a fixed goal T on the table; success = the block covers >= 90 % of the goal T's area, as
measured by the reference's 64 x 64 "pseudo-render" in the goal frame. Same scene content, randomisation, observation
keys, reward shaping and limits; no render materials (the camera is inert in this build).

The pseudo-render and the reward are also computed by a native epilogue (mssim_task_pusht_outputs,
include/mssim_hip_tasks.h) from the constants this env builds once in _load_scene: the uv grid, the 3 x 3
world-to-goal transform and the T template. tests/test_gpu_push_t.py holds the two paths against each other."""
from typing import Any, Dict

import numpy as np
import sapien
import torch
from transforms3d.euler import euler2quat

from maniskill_amd.envs.sapien_env import BaseEnv
from maniskill_amd.model import geom
from maniskill_amd.physx.components import PhysxMaterial
from maniskill_amd.sensors.camera import CameraConfig
from maniskill_amd.utils import sapien_utils
from maniskill_amd.utils.registration import register_env
from maniskill_amd.utils.scene_builder.table import TableSceneBuilder
from maniskill_amd.utils.structs.pose import Pose
from maniskill_amd.utils.structs.types import GPUMemoryConfig, SimConfig


class WhiteTableSceneBuilder(TableSceneBuilder):
    """the reference's table scene of PushT: a white table (nothing to do without a renderer) and, for panda_stick, a
    second noisy initial qpos drawn after the one of TableSceneBuilder.initialize (both draws are kept, in that order,
    so that the episode RNG stream matches the reference)"""

    PANDA_STICK_QPOS = np.array([0.662, 0.212, 0.086, -2.685, -0.115, 2.898, 1.673])

    def initialize(self, env_idx: torch.Tensor):
        super().initialize(env_idx)
        if self.env.robot_uids == "panda_stick":
            self.env.agent.reset(self._noisy_qpos(env_idx, self.PANDA_STICK_QPOS))
            self.env.agent.robot.set_pose(self._pose_cache["root"])


@register_env("PushT-v1", max_episode_steps=100)
class PushTEnv(BaseEnv):
    SUPPORTED_ROBOTS = ["panda_stick"]

    # T centre-of-mass spawn box (relative to the goal T) and the uniform yaw
    tee_spawnbox_xlength = 0.2
    tee_spawnbox_ylength = 0.3
    tee_spawnbox_xoffset = -0.1
    tee_spawnbox_yoffset = -0.1
    # goal T on the table, the end-effector goal marker
    goal_offset = torch.tensor([-0.156, -0.1])
    goal_z_rot = (5 / 3) * np.pi
    ee_starting_pos2D = torch.tensor([-0.321, 0.284, 1e-3])
    ee_starting_pos3D = torch.tensor([-0.321, 0.284, 0.024])
    intersection_thresh = 0.90
    # T block
    T_mass = 0.8
    T_dynamic_friction = 3
    T_static_friction = 3
    com_y = 0.0375  # the T's frame is its centre of mass: 0.0375 from the centre of the horizontal bar, towards the stem

    def __init__(self, *args, robot_uids="panda_stick", robot_init_qpos_noise=0.02, **kwargs):
        self.robot_init_qpos_noise = robot_init_qpos_noise
        super().__init__(*args, robot_uids=robot_uids, **kwargs)

    @property
    def _default_sim_config(self):
        return SimConfig(gpu_memory_config=GPUMemoryConfig(found_lost_pairs_capacity=2**25, max_rigid_patch_count=2**18))

    @property
    def _default_sensor_configs(self):
        pose = sapien_utils.look_at(eye=[0.3, 0, 0.6], target=[-0.1, 0, 0.1])
        return [CameraConfig("base_camera", pose=pose, width=128, height=128, fov=np.pi / 2, near=0.01, far=100)]

    @property
    def _default_human_render_camera_configs(self):
        pose = sapien_utils.look_at(eye=[0.3, 0, 0.6], target=[-0.1, 0, 0.1])
        return CameraConfig("render_camera", pose=pose, width=512, height=512, fov=1, near=0.01, far=100)

    def _load_agent(self, options: dict):
        super()._load_agent(options, sapien.Pose(p=[-0.615, 0, 0]))

    def _create_tee(self, name: str, target: bool):
        """two boxes about the centre of mass; the goal T is kinematic and visual-only"""
        box1_half_w, box1_half_h = 0.2 / 2, 0.05 / 2
        half_thickness = 0.04 / 2 if not target else 1e-4
        builder = self.scene.create_actor_builder()
        poses = (sapien.Pose([0.0, -self.com_y, 0.0]), sapien.Pose([0.0, 4 * box1_half_h - self.com_y, 0.0]))
        sizes = ([box1_half_w, box1_half_h, half_thickness], [box1_half_h, 0.75 * box1_half_w, half_thickness])
        builder.initial_pose = sapien.Pose(p=[0, 0, 0.1])
        if target:
            for p, s in zip(poses, sizes):
                builder.add_box_visual(pose=p, half_size=s)
            return builder.build_kinematic(name=name)
        mat = PhysxMaterial(static_friction=self.T_static_friction, dynamic_friction=self.T_dynamic_friction, restitution=0)
        for p, s in zip(poses, sizes):
            builder.add_box_collision(pose=p, half_size=s, material=mat)
        # mass 0.8 kg; centre of mass and inertia those of the boxes at uniform density, scaled to that mass
        items = [geom.transform_inertial(r.pose, *r.mass_properties()) for r in builder.shapes]
        m, c, I = geom.combine_inertials(items)
        builder.set_mass_and_inertia(self.T_mass, sapien.Pose(p=c), I * (self.T_mass / m))
        return builder.build(name=name)

    def _load_scene(self, options: dict):
        self._fused_state = None
        self.ee_starting_pos2D = self.ee_starting_pos2D.to(self.device)
        self.ee_starting_pos3D = self.ee_starting_pos3D.to(self.device)
        self.table_scene = WhiteTableSceneBuilder(env=self, robot_init_qpos_noise=self.robot_init_qpos_noise)
        self.table_scene.build()
        self.tee = self._create_tee("Tee", target=False)
        self.goal_tee = self._create_tee("goal_Tee", target=True)
        builder = self.scene.create_actor_builder()
        builder.add_cylinder_visual(radius=0.02, half_length=1e-4)
        builder.initial_pose = sapien.Pose(p=[0, 0, 0.1])
        self.ee_goal_pos = builder.build_kinematic(name="goal_ee")

        # the pseudo-render's constants, computed as the reference does (on the host, float32)
        res, uv_half_width = 64, 0.15
        self.res, self.uv_half_width = res, uv_half_width
        oned_grid = torch.arange(res, dtype=torch.float32).view(1, res).repeat(res, 1) - (res / 2)
        uv_grid = (torch.cat([oned_grid.unsqueeze(0), (-1 * oned_grid.T).unsqueeze(0)], dim=0) + 0.5) / ((res / 2) / uv_half_width)
        self.uv_grid = uv_grid.to(self.device)
        self.homo_uv = torch.cat([self.uv_grid, torch.ones_like(self.uv_grid[0]).unsqueeze(0)], dim=0)
        center_of_mass = (0, 0.0375)
        box1 = torch.tensor([[-0.1, 0.025], [0.1, 0.025], [-0.1, -0.025], [0.1, -0.025]])
        box2 = torch.tensor([[-0.025, 0.175], [0.025, 0.175], [-0.025, 0.025], [0.025, 0.025]])
        box1[:, 1] -= center_of_mass[1]
        box2[:, 1] -= center_of_mass[1]
        box1 = (box1 * ((res / 2) / uv_half_width) + res / 2).long()
        box2 = (box2 * ((res / 2) / uv_half_width) + res / 2).long()
        tee_render = torch.zeros(res, res)
        # (image rows are the y axis, flipped: set in the transpose, then flip)
        tee_render.T[box1[0, 0] : box1[1, 0], box1[2, 1] : box1[0, 1]] = 1
        tee_render.T[box2[0, 0] : box2[1, 0], box2[2, 1] : box2[0, 1]] = 1
        self.tee_render = tee_render.flip(0).to(self.device)
        goal_fake_quat = torch.tensor([(torch.tensor([self.goal_z_rot]) / 2).cos(), 0, 0, 0.0]).unsqueeze(0)
        zrot = self.quat_to_zrot(goal_fake_quat).squeeze(0)
        goal_trans = torch.eye(3)
        goal_trans[:2, :2] = zrot[:2, :2]
        goal_trans[0:2, 2] = self.goal_offset
        self.world_to_goal_trans = torch.linalg.inv(goal_trans).to(self.device)

    # ---- pseudo-render (the reference's, step for step) ----
    def quat_to_z_euler(self, quats):
        assert len(quats.shape) == 2 and quats.shape[-1] == 4
        # yaw of a quaternion about z from q_w alone, the double cover resolved by the sign of q_z: 2 acos(sign(q_z) q_w)
        signs = torch.ones_like(quats[:, -1])
        signs[quats[:, -1] < 0] = -1.0
        qw = quats[:, 0] * signs
        return 2 * qw.acos()

    def quat_to_zrot(self, quats):
        assert len(quats.shape) == 2 and quats.shape[-1] == 4
        alphas = self.quat_to_z_euler(quats)
        rot_mats = torch.zeros(quats.shape[0], 3, 3).to(quats.device)
        rot_mats[:, 2, 2] = 1
        rot_mats[:, 0, 0] = alphas.cos()
        rot_mats[:, 1, 1] = alphas.cos()
        rot_mats[:, 0, 1] = -alphas.sin()
        rot_mats[:, 1, 0] = alphas.sin()
        return rot_mats

    def pseudo_render_intersection_count(self):
        """template pixels of the goal T hit by at least one pixel of the block's T mapped into the goal frame [N]"""
        tee_to_world_trans = self.quat_to_zrot(self.tee.pose.q)
        tee_to_world_trans[:, 0:2, 2] = self.tee.pose.p[:, :2]
        tee_to_goal_trans = self.world_to_goal_trans @ tee_to_world_trans
        b = tee_to_world_trans.shape[0]
        res = self.uv_grid.shape[1]
        tees_in_goal_frame = (tee_to_goal_trans @ self.homo_uv.view(3, -1)).view(b, 3, res, res)
        tees_in_goal_frame = tees_in_goal_frame[:, 0:2, :, :] / tees_in_goal_frame[:, -1, :, :].unsqueeze(1)
        tee_coords = tees_in_goal_frame[:, :, self.tee_render == 1].view(b, 2, -1)
        # .long() truncates toward zero
        tee_indices = (tee_coords * ((res / 2) / self.uv_half_width) + (res / 2)).long().view(b, 2, -1)
        final_renders = torch.zeros(b, res, res).to(self.device)
        num_tee_pixels = tee_indices.shape[-1]
        batch_indices = torch.arange(b).view(-1, 1).repeat(1, num_tee_pixels).to(self.device)
        # out-of-range pixels go to (0, 0), which after the permute and flip lies outside the template
        invalid_xs = (tee_indices[:, 0, :] < 0) | (tee_indices[:, 0, :] >= self.res)
        invalid_ys = (tee_indices[:, 1, :] < 0) | (tee_indices[:, 1, :] >= self.res)
        tee_indices[:, 0, :][invalid_xs] = 0
        tee_indices[:, 1, :][invalid_xs] = 0
        tee_indices[:, 0, :][invalid_ys] = 0
        tee_indices[:, 1, :][invalid_ys] = 0
        final_renders[batch_indices, tee_indices[:, 0, :], tee_indices[:, 1, :]] = 1
        final_renders = final_renders.permute(0, 2, 1).flip(1)
        return (final_renders.bool() & self.tee_render.bool()).sum(dim=[-1, -2]).float()

    def goal_area(self) -> torch.Tensor:
        return self.tee_render.bool().sum().float()

    def pseudo_render_intersection(self):
        """intersection / goal area in [0, 1]"""
        return self.pseudo_render_intersection_count() / self.goal_area()

    def _initialize_episode(self, env_idx: torch.Tensor, options: dict):
        dev = self.device  # explicit devices, see PickCubeEnv._initialize_episode
        b = len(env_idx)
        self.table_scene.initialize(env_idx)
        target_region_xyz = torch.zeros((b, 3), device=dev)
        target_region_xyz[:, 0] += float(self.goal_offset[0])
        target_region_xyz[:, 1] += float(self.goal_offset[1])
        target_region_xyz[..., 2] = 1e-3
        goal_q = torch.tensor(euler2quat(0, 0, self.goal_z_rot), dtype=torch.float32, device=dev)
        self.goal_tee.set_pose(Pose.create_from_pq(p=target_region_xyz, q=goal_q))
        target_region_xyz[..., 0] += torch.rand(b, device=dev) * self.tee_spawnbox_xlength + self.tee_spawnbox_xoffset
        target_region_xyz[..., 1] += torch.rand(b, device=dev) * self.tee_spawnbox_ylength + self.tee_spawnbox_yoffset
        target_region_xyz[..., 2] = 0.04 / 2 + 1e-3
        q_euler_angle = torch.rand(b, device=dev) * (2 * torch.pi)
        q = torch.zeros((b, 4), device=dev)
        q[:, 0] = (q_euler_angle / 2).cos()
        q[:, -1] = (q_euler_angle / 2).sin()
        self.tee.set_pose(Pose.create_from_pq(p=target_region_xyz, q=q))
        xyz = torch.zeros((b, 3), device=dev)
        xyz[:] = self.ee_starting_pos2D
        ee_q = torch.tensor(euler2quat(0, np.pi / 2, 0), dtype=torch.float32, device=dev)
        self.ee_goal_pos.set_pose(Pose.create_from_pq(p=xyz, q=ee_q))

    def evaluate(self):
        inter_area = self.pseudo_render_intersection()
        return {"success": inter_area >= self.intersection_thresh}

    def _get_obs_extra(self, info: Dict):
        obs = dict(tcp_pose=self.agent.tcp.pose.raw_pose)
        if self.obs_mode_struct.use_state:
            obs.update(goal_pos=self.goal_tee.pose.p, obj_pose=self.tee.pose.raw_pose)
        return obs

    def compute_dense_reward(self, obs: Any, action: torch.Tensor, info: Dict):
        # rotation: ((cos(yaw - goal yaw) + 1) / 2)^2 / 2, yaw as quat_to_z_euler gives it (in [0, 2 pi])
        tee_z_eulers = self.quat_to_z_euler(self.tee.pose.q)
        rot_rew = (tee_z_eulers - self.goal_z_rot).cos()
        reward = (((rot_rew + 1) / 2) ** 2) / 2
        # planar distance to the goal
        tee_to_goal_pose_dist = torch.linalg.norm(self.tee.pose.p[:, 0:2] - self.goal_tee.pose.p[:, 0:2], axis=1)
        reward += ((1 - torch.tanh(5 * tee_to_goal_pose_dist)) ** 2) / 2
        # the tcp near the block's centre of mass
        tcp_to_push_pose_dist = torch.linalg.norm(self.tee.pose.p - self.agent.tcp.pose.p, axis=1)
        # (far from the block 1 - tanh cancels to a few ulp of 1 and the root magnifies that about 100-fold: this float32
        # expression is good to ~2e-7 there only as long as tanh is rounded to half an ulp. The native epilogue states the same
        # term as sqrt(2 / (exp(10 d) + 1)), which does not cancel; the two agree within the tests' tolerance.)
        reward += ((1 - torch.tanh(5 * tcp_to_push_pose_dist)).sqrt()) / 20
        reward[info["success"]] = 3
        return reward

    def compute_normalized_dense_reward(self, obs: Any, action: torch.Tensor, info: Dict):
        return self.compute_dense_reward(obs=obs, action=action, info=info) / 3.0

    # ---- fused evaluate + obs + reward (one native launch; tests/test_gpu_push_t.py) ----
    def _fused_task_ok(self) -> bool:
        cls = type(self)
        same = all(
            getattr(cls, m) is getattr(PushTEnv, m)
            for m in ("evaluate", "_get_obs_extra", "compute_dense_reward", "compute_normalized_dense_reward", "pseudo_render_intersection",
                      "pseudo_render_intersection_count", "goal_area", "quat_to_z_euler", "quat_to_zrot", "_get_obs_agent", "get_obs",
                      "get_info", "get_reward")
        )
        return (
            same
            and self.robot_uids == "panda_stick"
            and self._obs_mode == "state"
            and self._reward_mode in ("dense", "normalized_dense")
            and len(self.agent.controller.get_state()) == 0
        )

    def pusht_consts(self) -> torch.Tensor:
        """the native epilogue's per-model constants as one int32 device block (mssim_pusht_consts of
        include/mssim_hip_tasks.h): world_to_goal (9 f32, row-major), u of each grid column (64 f32), v of each grid row
        (64 f32), the template as 128 bit words (bit 64 * row + col), the template's pixel count"""
        w2g = self.world_to_goal_trans.detach().to("cpu", torch.float32).reshape(9)
        uv = self.uv_grid.detach().to("cpu", torch.float32)
        u, v = uv[0, 0, :].clone(), uv[1, :, 0].clone()
        assert torch.equal(uv[0], u.expand(64, 64)) and torch.equal(uv[1], v[:, None].expand(64, 64))
        bits = self.tee_render.detach().to("cpu").bool().reshape(128, 32).to(torch.int64)
        words = (bits << torch.arange(32, dtype=torch.int64)).sum(1)
        words = torch.where(words >= 2**31, words - 2**32, words).to(torch.int32)
        area = torch.tensor([int(self.tee_render.bool().sum())], dtype=torch.int32)
        block = torch.cat([w2g.view(torch.int32), u.view(torch.int32), v.view(torch.int32), words, area])
        return block.to(self.device)

    def _fused_step_outputs(self, action, advance: bool = True):
        if not self._fused_ok():
            return None
        from maniskill_amd import native

        px = self.scene.px
        st = getattr(self, "_fused_state", None)
        if st is None or st["px"] is not px:
            consts = self.pusht_consts()
            task = native.PushTTask(
                tcp_row=self.agent.tcp._body_row, tee_row=self.tee._body_row, goal_row=self.goal_tee._body_row,
                goal_z_rot=float(self.goal_z_rot), intersection_thresh=float(self.intersection_thresh),
                reward_div=3.0 if self._reward_mode == "normalized_dense" else 1.0, consts=consts.data_ptr(),
            )
            st = self._fused_state = dict(px=px, task=task, consts=consts)  # (consts keeps the device block alive)
        N, D = self.num_envs, 2 * self.agent.robot.max_dof + 17
        obs = torch.empty((N, D), dtype=torch.float32, device=self.device)
        reward = torch.empty((N,), dtype=torch.float32, device=self.device)
        flags = torch.empty((N, 1), dtype=torch.uint8, device=self.device)
        # (the count of template pixels hit, kept for inspection: tests/test_gpu_push_t.py)
        self._fused_intersection = torch.empty((N,), dtype=torch.float32, device=self.device)
        es = self._fused_bind_counters(st["task"], advance)
        px.task_pusht_outputs(st["task"], obs, reward, flags, self._fused_intersection)
        info = dict(elapsed_steps=es, success=flags.view(torch.bool)[:, 0])
        return obs, reward, info
