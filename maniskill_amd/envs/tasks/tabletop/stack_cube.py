"""StackCube-v1 (task definition restated from mani_skill/envs/tasks/tabletop/stack_cube.py:19-200):
pick up the red cube A and stack it on the green cube B, then let go; success = A resting on B (to within 5 mm), A
static and not grasped. Same scene content, randomisation, observation keys, reward shaping and limits; no render
materials (the camera is inert in this build)."""
from typing import Any, Dict

import numpy as np
import sapien
import torch

import maniskill_amd.envs.utils.randomization as randomization
from maniskill_amd.envs.sapien_env import BaseEnv
from maniskill_amd.sensors.camera import CameraConfig
from maniskill_amd.utils import common, sapien_utils
from maniskill_amd.utils.building import actors
from maniskill_amd.utils.registration import register_env
from maniskill_amd.utils.scene_builder.table import TableSceneBuilder
from maniskill_amd.utils.structs.pose import Pose


@register_env("StackCube-v1", max_episode_steps=50)
class StackCubeEnv(BaseEnv):
    SUPPORTED_ROBOTS = ["panda_wristcam", "panda", "fetch"]

    def __init__(self, *args, robot_uids="panda_wristcam", robot_init_qpos_noise=0.02, **kwargs):
        self.robot_init_qpos_noise = robot_init_qpos_noise
        super().__init__(*args, robot_uids=robot_uids, **kwargs)

    @property
    def _default_sensor_configs(self):
        pose = sapien_utils.look_at(eye=[0.3, 0, 0.6], target=[-0.1, 0, 0.1])
        return [CameraConfig("base_camera", pose, 128, 128, np.pi / 2, 0.01, 100)]

    @property
    def _default_human_render_camera_configs(self):
        pose = sapien_utils.look_at([0.6, 0.7, 0.6], [0.0, 0.0, 0.35])
        return CameraConfig("render_camera", pose, 512, 512, 1, 0.01, 100)

    def _load_agent(self, options: dict):
        super()._load_agent(options, sapien.Pose(p=[-0.615, 0, 0]))

    def _load_scene(self, options: dict):
        self._fused_state = None
        self.cube_half_size = common.to_tensor([0.02] * 3, device=self.device)
        self.table_scene = TableSceneBuilder(env=self, robot_init_qpos_noise=self.robot_init_qpos_noise)
        self.table_scene.build()
        self.cubeA = actors.build_cube(self.scene, half_size=0.02, color=[1, 0, 0, 1], name="cubeA", initial_pose=sapien.Pose(p=[0, 0, 0.1]))
        self.cubeB = actors.build_cube(self.scene, half_size=0.02, color=[0, 1, 0, 1], name="cubeB", initial_pose=sapien.Pose(p=[1, 0, 0.1]))

    def _initialize_episode(self, env_idx: torch.Tensor, options: dict):
        dev = self.device  # explicit devices, see PickCubeEnv._initialize_episode
        b = len(env_idx)
        self.table_scene.initialize(env_idx)
        xyz = torch.zeros((b, 3), device=dev)
        xyz[:, 2] = 0.02
        xy = torch.rand((b, 2), device=dev) * 0.2 - 0.1
        sampler = randomization.UniformPlacementSampler(bounds=[[-0.1, -0.2], [0.1, 0.2]], batch_size=b, device=dev)
        radius = float(torch.linalg.norm(torch.tensor([0.02, 0.02]))) + 0.001
        cubeA_xy = xy + sampler.sample(radius, 100)
        cubeB_xy = xy + sampler.sample(radius, 100, verbose=False)

        xyz[:, :2] = cubeA_xy
        qs = randomization.random_quaternions(b, device=dev, lock_x=True, lock_y=True, lock_z=False)
        self.cubeA.set_pose(Pose.create_from_pq(p=xyz.clone(), q=qs))
        xyz[:, :2] = cubeB_xy
        qs = randomization.random_quaternions(b, device=dev, lock_x=True, lock_y=True, lock_z=False)
        self.cubeB.set_pose(Pose.create_from_pq(p=xyz, q=qs))

    def evaluate(self):
        offset = self.cubeA.pose.p - self.cubeB.pose.p
        xy_flag = torch.linalg.norm(offset[..., :2], axis=1) <= torch.linalg.norm(self.cube_half_size[:2]) + 0.005
        z_flag = torch.abs(offset[..., 2] - self.cube_half_size[..., 2] * 2) <= 0.005
        is_cubeA_on_cubeB = torch.logical_and(xy_flag, z_flag)
        # (the reference's note: GPU sims report sizeable angular velocities of a cube that hardly rotates, hence 0.5)
        is_cubeA_static = self.cubeA.is_static(lin_thresh=1e-2, ang_thresh=0.5)
        is_cubeA_grasped = self.agent.is_grasping(self.cubeA)
        success = is_cubeA_on_cubeB * is_cubeA_static * (~is_cubeA_grasped)
        return {
            "is_cubeA_grasped": is_cubeA_grasped,
            "is_cubeA_on_cubeB": is_cubeA_on_cubeB,
            "is_cubeA_static": is_cubeA_static,
            "success": success.bool(),
        }

    def _get_obs_extra(self, info: Dict):
        obs = dict(tcp_pose=self.agent.tcp.pose.raw_pose)
        if "state" in self.obs_mode:
            obs.update(
                cubeA_pose=self.cubeA.pose.raw_pose,
                cubeB_pose=self.cubeB.pose.raw_pose,
                tcp_to_cubeA_pos=self.cubeA.pose.p - self.agent.tcp.pose.p,
                tcp_to_cubeB_pos=self.cubeB.pose.p - self.agent.tcp.pose.p,
                cubeA_to_cubeB_pos=self.cubeB.pose.p - self.cubeA.pose.p,
            )
        return obs

    def _gripper_width(self) -> torch.Tensor:
        """fully open finger gap, qlimits[-1].hi * 2 (the reference notes this as Panda-specific)"""
        return (self.agent.robot.get_qlimits()[0, -1, 1] * 2).to(self.device)

    def compute_dense_reward(self, obs: Any, action: torch.Tensor, info: Dict):
        # reaching
        tcp_pos = self.agent.tcp.pose.p
        cubeA_pos, cubeB_pos = self.cubeA.pose.p, self.cubeB.pose.p
        reward = 2 * (1 - torch.tanh(5 * torch.linalg.norm(tcp_pos - cubeA_pos, axis=1)))
        # grasp and place
        goal_xyz = torch.hstack([cubeB_pos[:, 0:2], (cubeB_pos[:, 2] + self.cube_half_size[2] * 2)[:, None]])
        place_reward = 1 - torch.tanh(5.0 * torch.linalg.norm(goal_xyz - cubeA_pos, axis=1))
        is_cubeA_grasped = info["is_cubeA_grasped"]
        reward[is_cubeA_grasped] = (4 + place_reward)[is_cubeA_grasped]
        # ungrasp and static
        ungrasp_reward = torch.sum(self.agent.robot.get_qpos()[:, -2:], axis=1) / self._gripper_width()
        ungrasp_reward[~is_cubeA_grasped] = 1.0
        v = torch.linalg.norm(self.cubeA.linear_velocity, axis=1)
        av = torch.linalg.norm(self.cubeA.angular_velocity, axis=1)
        static_reward = 1 - torch.tanh(v * 10 + av)
        on = info["is_cubeA_on_cubeB"]
        reward[on] = (6 + (ungrasp_reward + static_reward) / 2.0)[on]
        reward[info["success"]] = 8
        return reward

    def compute_normalized_dense_reward(self, obs: Any, action: torch.Tensor, info: Dict):
        return self.compute_dense_reward(obs=obs, action=action, info=info) / 8

    # ---- fused evaluate + obs + reward (one native launch; identical results, tests/test_gpu_stack_cube.py) ----
    def _fused_task_ok(self) -> bool:
        cls = type(self)
        same = all(
            getattr(cls, m) is getattr(StackCubeEnv, m)
            for m in ("evaluate", "_get_obs_extra", "compute_dense_reward", "compute_normalized_dense_reward", "_gripper_width", "_get_obs_agent", "get_obs",
                      "get_info", "get_reward")
        )
        from maniskill_amd.envs.utils.task_robot import fused_robot_ok

        # (panda_wristcam: the Panda's kinematics and fingers on another mount; the camera adds nothing to the state obs)
        ok = (
            same
            and fused_robot_ok(self, ("panda", "panda_wristcam"))
            and self._obs_mode == "state"
            and self._reward_mode in ("dense", "normalized_dense")
            and len(self.agent.controller.get_state()) == 0
        )
        return ok

    def _fused_step_outputs(self, action, advance: bool = True):
        if not self._fused_ok():
            return None
        from maniskill_amd import native
        from maniskill_amd.envs.utils.task_robot import fused_robot_rows

        px = self.scene.px
        st = getattr(self, "_fused_state", None)
        if st is None or st["px"] is not px:
            hs = self.cube_half_size.float()
            finger1_row, finger2_row = fused_robot_rows(self)
            task = native.StackTask(
                tcp_row=self.agent.tcp._body_row, cubeA_row=self.cubeA._body_row, cubeB_row=self.cubeB._body_row,
                finger1_row=finger1_row, finger2_row=finger2_row,
                # (the thresholds as evaluate() computes them in float32, so that the flags agree bit for bit)
                cube_half_size=float(hs[2]), on_xy_thresh=float(torch.linalg.norm(hs[:2]) + 0.005), on_z_thresh=0.005,
                gripper_width=float(self._gripper_width()), static_lin_thresh=1e-2, static_ang_thresh=0.5, min_force=0.5, max_angle_deg=85.0,
                reward_scale=0.125 if self._reward_mode == "normalized_dense" else 1.0,
            )
            st = self._fused_state = dict(px=px, task=task)
        N, D = self.num_envs, 2 * self.agent.robot.max_dof + 30
        obs = torch.empty((N, D), dtype=torch.float32, device=self.device)
        reward = torch.empty((N,), dtype=torch.float32, device=self.device)
        flags = torch.empty((N, 4), dtype=torch.uint8, device=self.device)
        es = self._fused_bind_counters(st["task"], advance)
        px.task_stack_outputs(st["task"], obs, reward, flags)
        fb = flags.view(torch.bool)
        info = dict(elapsed_steps=es, is_cubeA_grasped=fb[:, 3], is_cubeA_on_cubeB=fb[:, 1], is_cubeA_static=fb[:, 2], success=fb[:, 0])
        return obs, reward, info
