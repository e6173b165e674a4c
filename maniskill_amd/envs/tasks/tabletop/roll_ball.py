"""RollBall-v1 (task definition restated from mani_skill/envs/tasks/tabletop/roll_ball.py:20-181):
push a ball so that it rolls across the table into a goal disc at the far end; the Panda stands at the table's side.
The dense reward carries a per-env latch, `reached_status`: set once the tcp has been at the hit point behind the ball,
cleared by a reset of that env."""
from typing import Any, Dict

import numpy as np
import sapien
import torch
from transforms3d.euler import euler2quat

from maniskill_amd.envs.sapien_env import BaseEnv
from maniskill_amd.sensors.camera import CameraConfig
from maniskill_amd.utils import sapien_utils
from maniskill_amd.utils.building import actors
from maniskill_amd.utils.registration import register_env
from maniskill_amd.utils.scene_builder.table import TableSceneBuilder
from maniskill_amd.utils.structs.pose import Pose
from maniskill_amd.utils.structs.types import GPUMemoryConfig, SimConfig


@register_env("RollBall-v1", max_episode_steps=80)
class RollBallEnv(BaseEnv):
    SUPPORTED_ROBOTS = ["panda"]
    goal_radius: float = 0.1
    ball_radius: float = 0.035
    hit_offset: float = 0.05  # the hit point lies ball_radius + this behind the ball's centre, seen from the goal
    reach_thresh: float = 0.04
    reached_status: torch.Tensor

    def __init__(self, *args, robot_uids="panda", robot_init_qpos_noise=0.02, **kwargs):
        self.robot_init_qpos_noise = robot_init_qpos_noise
        super().__init__(*args, robot_uids=robot_uids, **kwargs)

    @property
    def _default_sim_config(self):
        return SimConfig(gpu_memory_config=GPUMemoryConfig(found_lost_pairs_capacity=2**25, max_rigid_patch_count=2**18))

    @property
    def _default_sensor_configs(self):
        pose = sapien_utils.look_at(eye=[-0.1, 0.9, 0.3], target=[0.0, 0.0, 0.0])
        return [CameraConfig("base_camera", pose, 128, 128, np.pi / 2, 0.01, 100)]

    @property
    def _default_human_render_camera_configs(self):
        pose = sapien_utils.look_at([-0.6, 1.3, 0.8], [0.0, 0.13, 0.0])
        return CameraConfig("render_camera", pose, 512, 512, 1, 0.01, 100)

    def _load_agent(self, options: dict):
        super()._load_agent(options, sapien.Pose(p=[-0.615, 0, 0]))

    def _load_scene(self, options: dict):
        self._fused_state = None
        self.table_scene = TableSceneBuilder(self, robot_init_qpos_noise=self.robot_init_qpos_noise)
        self.table_scene.build()
        self.ball = actors.build_sphere(self.scene, radius=self.ball_radius, color=[0, 0.2, 0.8, 1], name="ball", initial_pose=sapien.Pose(p=[0, 0, 0.1]))
        self.goal_region = actors.build_red_white_target(
            self.scene, radius=self.goal_radius, thickness=1e-5, name="goal_region", add_collision=False, body_type="kinematic",
            initial_pose=sapien.Pose(p=[0, 0, 0.1]),
        )
        # on the device from the start and never replaced: the native epilogue reads and writes it in place
        self.reached_status = torch.zeros(self.num_envs, dtype=torch.float32, device=self.device)
        self._robot_pose = None

    def _initialize_episode(self, env_idx: torch.Tensor, options: dict):
        dev = self.device  # explicit devices, see PickCubeEnv._initialize_episode
        b = len(env_idx)
        self.table_scene.initialize(env_idx)
        # the root pose the table scene has just set, overwritten: the arm at the table's side, facing -y (the quaternion
        # is not of unit length; kept as the reference writes it)
        if self._robot_pose is None or self._robot_pose.device != dev:
            self._robot_pose = Pose.create_from_pq(p=[-0.1, 1.0, 0], q=[0.7071, 0, 0, -0.7072], device=dev)
        self.agent.robot.set_pose(self._robot_pose)

        xyz = torch.zeros((b, 3), device=dev)
        xyz[..., 0] = (torch.rand((b), device=dev) * 2 - 1) * 0.3 - 0.1
        xyz[..., 1] = torch.rand((b), device=dev) * 0.2 + 0.5
        xyz[..., 2] = self.ball_radius
        self.ball.set_pose(Pose.create_from_pq(p=xyz, q=[1, 0, 0, 0]))

        xyz_goal = torch.zeros((b, 3), device=dev)
        xyz_goal[..., 0] = (torch.rand((b), device=dev) * 2 - 1) * 0.3 - 0.1
        xyz_goal[..., 1] = torch.rand((b), device=dev) * 0.2 - 1.0 + self.goal_radius
        xyz_goal[..., 2] = 1e-3
        self.goal_region.set_pose(Pose.create_from_pq(p=xyz_goal, q=euler2quat(0, np.pi / 2, 0)))
        self.reached_status[env_idx] = 0.0

    def evaluate(self):
        is_obj_placed = torch.linalg.norm(self.ball.pose.p[..., :2] - self.goal_region.pose.p[..., :2], axis=1) < self.goal_radius
        return {"success": is_obj_placed}

    def _get_obs_extra(self, info: Dict):
        obs = dict(tcp_pose=self.agent.tcp.pose.raw_pose)
        if self.obs_mode_struct.use_state:
            obs.update(
                goal_pos=self.goal_region.pose.p,
                ball_pose=self.ball.pose.raw_pose,
                ball_vel=self.ball.linear_velocity,
                tcp_to_ball_pos=self.ball.pose.p - self.agent.tcp.pose.p,
                ball_to_goal_pos=self.goal_region.pose.p - self.ball.pose.p,
            )
        return obs

    def compute_dense_reward(self, obs: Any, action, info: Dict):
        unit_vec = self.ball.pose.p - self.goal_region.pose.p
        unit_vec = unit_vec / torch.linalg.norm(unit_vec, axis=1, keepdim=True)
        tcp_hit_p = self.ball.pose.p + unit_vec * (self.ball_radius + self.hit_offset)
        tcp_to_hit_dist = torch.linalg.norm(tcp_hit_p - self.agent.tcp.pose.p, axis=1)
        self.reached_status[tcp_to_hit_dist < self.reach_thresh] = 1.0
        reaching_reward = 1 - torch.tanh(2 * tcp_to_hit_dist)
        obj_to_goal_dist = torch.linalg.norm(self.ball.pose.p[..., :2] - self.goal_region.pose.p[..., :2], axis=1)
        reached_reward = 1 - torch.tanh(obj_to_goal_dist)
        reward = 20 * reached_reward * self.reached_status + reaching_reward * (1 - self.reached_status) + self.reached_status
        reward[info["success"]] = 30.0
        return reward

    def compute_normalized_dense_reward(self, obs: Any, action, info: Dict):
        return self.compute_dense_reward(obs=obs, action=action, info=info) / 30.0

    # ---- fused evaluate + obs + reward (one native launch after the control step's; tests/test_gpu_roll_pull.py) ----
    def _fused_task_ok(self) -> bool:
        cls = type(self)
        same = all(
            getattr(cls, m) is getattr(RollBallEnv, m)
            for m in ("evaluate", "_get_obs_extra", "compute_dense_reward", "compute_normalized_dense_reward", "_get_obs_agent", "get_obs", "get_info", "get_reward")
        )
        return same and self._obs_mode == "state" and self._reward_mode in ("dense", "normalized_dense") and len(self.agent.controller.get_state()) == 0

    def _fused_step_outputs(self, action, advance: bool = True):
        if not self._fused_ok():
            return None
        from maniskill_amd import native

        px = self.scene.px
        st = getattr(self, "_fused_state", None)
        if st is None or st["px"] is not px:
            task = native.RollTask(tcp_row=self.agent.tcp._body_row, ball_row=self.ball._body_row, goal_row=self.goal_region._body_row,
                                   goal_radius=self.goal_radius, ball_radius=self.ball_radius, hit_offset=self.hit_offset, reach_thresh=self.reach_thresh,
                                   reward_scale=1.0 / 30.0 if self._reward_mode == "normalized_dense" else 1.0)
            st = self._fused_state = dict(px=px, task=task)
        N, D = self.num_envs, 2 * self.agent.robot.max_dof + 26
        obs = torch.empty((N, D), dtype=torch.float32, device=self.device)
        reward = torch.empty((N,), dtype=torch.float32, device=self.device)
        flags = torch.empty((N, 1), dtype=torch.uint8, device=self.device)
        es = self._fused_bind_counters(st["task"], advance)
        # the latch moves with a step's reward only: a reset's outputs (advance=False) leave it as the reset set it
        st["task"].reached, st["task"].update_reached = self.reached_status.data_ptr(), int(advance)
        px.task_roll_outputs(st["task"], obs, reward, flags)
        return obs, reward, dict(elapsed_steps=es, success=flags.view(torch.bool)[:, 0])
