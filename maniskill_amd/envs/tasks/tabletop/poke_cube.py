"""PokeCube-v1 (task definition restated from mani_skill/envs/tasks/tabletop/poke_cube.py:20-230):
grasp a peg lying on the table and poke a cube with its head until the cube sits on a goal disc ahead of it.
The reference's quirks are kept, a learner's observations and reward depend on them: the `goal_pos` entry is the PEG's
position, `peg_head_pos` adds the head offset unrotated, and `angle_diff` is not wrapped."""
from typing import Any, Dict

import numpy as np
import sapien
import torch
from transforms3d.euler import euler2quat

from maniskill_amd.envs.sapien_env import BaseEnv
from maniskill_amd.envs.utils import randomization
from maniskill_amd.sensors.camera import CameraConfig
from maniskill_amd.utils import sapien_utils
from maniskill_amd.utils.building import actors
from maniskill_amd.utils.geometry import rotation_conversions
from maniskill_amd.utils.registration import register_env
from maniskill_amd.utils.scene_builder.table import TableSceneBuilder
from maniskill_amd.utils.structs.pose import Pose


@register_env("PokeCube-v1", max_episode_steps=50)
class PokeCubeEnv(BaseEnv):
    SUPPORTED_ROBOTS = ["panda", "fetch"]
    cube_half_size = 0.02
    peg_half_width = 0.025
    peg_half_length = 0.12
    goal_radius = 0.05

    def __init__(self, *args, robot_uids="panda", robot_init_qpos_noise=0.02, **kwargs):
        self.robot_init_qpos_noise = robot_init_qpos_noise
        super().__init__(*args, robot_uids=robot_uids, **kwargs)

    @property
    def _default_sensor_configs(self):
        pose = sapien_utils.look_at(eye=[0.3, 0, 0.6], target=[-0.1, 0, 0.1])
        return [CameraConfig("base_camera", pose, 128, 128, np.pi / 2, 0.01, 100)]

    @property
    def _default_human_render_camera_configs(self):
        pose = sapien_utils.look_at([0.6, 0.7, 0.6], [0.2, 0.2, 0.35])
        return CameraConfig("render_camera", pose, 512, 512, 1, 0.01, 100)

    def _load_agent(self, options: dict):
        super()._load_agent(options, sapien.Pose(p=[-0.615, 0, 0]))

    def _load_scene(self, options: dict):
        self._fused_state = None
        self.table_scene = TableSceneBuilder(self, robot_init_qpos_noise=self.robot_init_qpos_noise)
        self.table_scene.build()
        self.cube = actors.build_cube(
            self.scene, half_size=self.cube_half_size, color=[1, 0, 0, 1], name="cube", body_type="dynamic",
            initial_pose=sapien.Pose(p=[1, 0, self.cube_half_size]),
        )
        blue = np.array([12, 42, 160, 255]) / 255
        self.peg = actors.build_twocolor_peg(
            self.scene, length=self.peg_half_length, width=self.peg_half_width, color_1=blue, color_2=blue, name="peg", body_type="dynamic",
            initial_pose=sapien.Pose(p=[0, 0, self.peg_half_width]),
        )
        self.goal_region = actors.build_red_white_target(
            self.scene, radius=self.goal_radius, thickness=1e-5, name="goal_region", add_collision=False, body_type="kinematic",
            initial_pose=sapien.Pose(),
        )
        self.peg_head_offsets = Pose.create_from_pq(p=[self.peg_half_length, 0, 0], device=self.device)

    @property
    def peg_head_pos(self):
        """(position only: the offset is NOT rotated with the peg -- as the reference's property of this name)"""
        return self.peg.pose.p + self.peg_head_offsets.p

    @property
    def peg_head_pose(self):
        return self.peg.pose * self.peg_head_offsets

    def _initialize_episode(self, env_idx: torch.Tensor, options: dict):
        dev = self.device  # explicit devices, see PickCubeEnv._initialize_episode
        b = len(env_idx)
        self.table_scene.initialize(env_idx)
        # the peg flat on the table, along x
        peg_xyz = torch.rand((b, 3), device=dev) * 0.2 - 0.1
        peg_xyz[..., 2] = self.peg_half_width
        self.peg.set_pose(Pose.create_from_pq(p=peg_xyz, q=[1, 0, 0, 0]))
        # the cube 0.1 ahead of the peg's head, turned about z by up to 30 degrees
        cube_xyz = torch.rand((b, 3), device=dev) * 0.2 - 0.1
        cube_xyz[..., 0] = peg_xyz[..., 0] + self.peg_half_length + 0.1
        cube_xyz[..., 2] = self.cube_half_size
        cube_q = randomization.random_quaternions(b, device=dev, lock_x=True, lock_y=True, lock_z=False, bounds=(-np.pi / 6, np.pi / 6))
        self.cube.set_pose(Pose.create_from_pq(p=cube_xyz, q=cube_q))
        # the goal disc 0.05 + radius ahead of the cube
        goal_xyz = cube_xyz + torch.tensor([0.05 + self.goal_radius, 0, 0], device=dev)
        goal_xyz[..., 2] = 1e-3
        self.goal_region.set_pose(Pose.create_from_pq(p=goal_xyz, q=euler2quat(0, np.pi / 2, 0)))

    def _get_obs_extra(self, info: Dict):
        obs = dict(tcp_pose=self.agent.tcp.pose.raw_pose)
        if self.obs_mode_struct.use_state:
            obs.update(
                cube_pose=self.cube.pose.raw_pose,
                peg_pose=self.peg.pose.raw_pose,
                goal_pos=self.peg.pose.p,  # (the peg's position: as the reference)
                tcp_to_peg_pos=self.peg.pose.p - self.agent.tcp.pose.p,
                peg_to_cube_pos=self.cube.pose.p - self.peg.pose.p,
                cube_to_goal_pos=self.goal_region.pose.p - self.cube.pose.p,
                peghead_to_cube_pos=self.peg_head_pos - self.cube.pose.p,
            )
        return obs

    @staticmethod
    def _euler_z(q: torch.Tensor) -> torch.Tensor:
        """the third angle of the XYZ decomposition of a quaternion's rotation matrix"""
        return rotation_conversions.matrix_to_euler_angles(rotation_conversions.quaternion_to_matrix(q), "XYZ")[:, 2]

    def evaluate(self):
        is_cube_placed = torch.linalg.norm(self.cube.pose.p[..., :2] - self.goal_region.pose.p[..., :2], axis=1) < self.goal_radius
        angle_diff = torch.abs(self._euler_z(self.peg_head_pose.q) - self._euler_z(self.cube.pose.q))
        is_peg_cube_aligned = angle_diff < 0.05
        head_to_cube_dist = torch.linalg.norm(self.peg_head_pos[..., :2] - self.cube.pose.p[..., :2], axis=1)
        is_peg_cube_close = head_to_cube_dist <= self.cube_half_size + 0.005
        is_peg_cube_fit = torch.logical_and(is_peg_cube_aligned, is_peg_cube_close)
        is_peg_grasped = self.agent.is_grasping(self.peg)
        is_robot_static = self.agent.is_static(0.2)
        return {
            "success": is_cube_placed & is_robot_static,
            "is_cube_placed": is_cube_placed,
            "is_peg_cube_fit": is_peg_cube_fit,
            "is_peg_grasped": is_peg_grasped,
            "angle_diff": angle_diff,
            "head_to_cube_dist": head_to_cube_dist,
        }

    def compute_dense_reward(self, obs: Any, action: torch.Tensor, info: Dict):
        # tiers, each overwriting the one before: reach the peg; grasped there: bring the head to the cube, aligned;
        # fit: push the cube to the goal; placed: come to rest
        tcp_to_peg_dist = torch.linalg.norm(self.agent.tcp.pose.p - self.peg.pose.p, axis=1)
        reached = tcp_to_peg_dist < 0.01
        reward = 2 * (1 - torch.tanh(5.0 * tcp_to_peg_dist))

        align_reward = 1 - torch.tanh(5.0 * info["angle_diff"])
        close_reward = 1 - torch.tanh(5.0 * info["head_to_cube_dist"])
        is_peg_grasped = info["is_peg_grasped"] * reached
        reward[is_peg_grasped] = (4 + close_reward + align_reward)[is_peg_grasped]

        cube_to_goal_dist = torch.linalg.norm(self.goal_region.pose.p - self.cube.pose.p, axis=1)
        place_reward = 1 - torch.tanh(5 * cube_to_goal_dist)
        is_peg_cube_fit = info["is_peg_cube_fit"] * is_peg_grasped
        reward[is_peg_cube_fit] = (7 + place_reward)[is_peg_cube_fit]

        static_reward = 1 - torch.tanh(5 * torch.linalg.norm(self.agent.robot.get_qvel()[..., :-2], axis=1))
        reward[info["is_cube_placed"]] += static_reward[info["is_cube_placed"]]

        reward[info["success"]] = 10
        return reward

    def compute_normalized_dense_reward(self, obs: Any, action: torch.Tensor, info: Dict):
        return self.compute_dense_reward(obs=obs, action=action, info=info) / 10.0

    # ---- fused evaluate + obs + reward (one native launch after the control step's; tests/test_gpu_poke_lift.py) ----
    def _fused_task_ok(self) -> bool:
        cls = type(self)
        same = all(
            getattr(cls, m) is getattr(PokeCubeEnv, m)
            for m in ("evaluate", "_euler_z", "peg_head_pos", "peg_head_pose", "_get_obs_extra", "compute_dense_reward", "compute_normalized_dense_reward",
                      "_get_obs_agent", "get_obs", "get_info", "get_reward")
        )
        from maniskill_amd.envs.utils.task_robot import fused_robot_ok

        return (same and fused_robot_ok(self, ("panda",), needs_static=True)
                and self._obs_mode == "state" and self._reward_mode in ("dense", "normalized_dense") and len(self.agent.controller.get_state()) == 0)

    def _fused_step_outputs(self, action, advance: bool = True):
        if not self._fused_ok():
            return None
        from maniskill_amd import native
        from maniskill_amd.envs.utils.task_robot import apply_robot_profile, fused_robot_rows

        px = self.scene.px
        st = getattr(self, "_fused_state", None)
        if st is None or st["px"] is not px:
            finger1_row, finger2_row = fused_robot_rows(self)
            task = native.PokeTask(
                tcp_row=self.agent.tcp._body_row, peg_row=self.peg._body_row, cube_row=self.cube._body_row, goal_row=self.goal_region._body_row,
                finger1_row=finger1_row, finger2_row=finger2_row,
                n_static_dofs=self.agent.robot.max_dof - 2, peg_half_length=self.peg_half_length, cube_half_size=self.cube_half_size,
                goal_radius=self.goal_radius, align_thresh=0.05, reach_thresh=0.01, static_thresh=0.2, min_force=0.5,
                max_angle_deg=85.0, reward_scale=0.1 if self._reward_mode == "normalized_dense" else 1.0,
            )
            st = self._fused_state = dict(px=px, task=task)
        N, D = self.num_envs, 2 * self.agent.robot.max_dof + 36
        obs = torch.empty((N, D), dtype=torch.float32, device=self.device)
        reward = torch.empty((N,), dtype=torch.float32, device=self.device)
        flags = torch.empty((N, 4), dtype=torch.uint8, device=self.device)
        metrics = torch.empty((N, 2), dtype=torch.float32, device=self.device)
        es = self._fused_bind_counters(st["task"], advance)
        apply_robot_profile(self, 0.2)
        px.task_poke_outputs(st["task"], obs, reward, flags, metrics)
        fb = flags.view(torch.bool)
        info = dict(elapsed_steps=es, success=fb[:, 0], is_cube_placed=fb[:, 1], is_peg_cube_fit=fb[:, 2], is_peg_grasped=fb[:, 3],
                    angle_diff=metrics[:, 0], head_to_cube_dist=metrics[:, 1])
        return obs, reward, info
