"""LiftPegUpright-v1 (task definition restated from mani_skill/envs/tasks/tabletop/lift_peg_upright.py:21-144):
a peg lies flat on the table; stand it on one of its ends. As in the reference, the upright test reads the THIRD angle of
the XYZ decomposition of the peg's rotation (within 0.08 of +-pi/2), not the "y angle" its description names, and the
reaching term is set to 1 where the peg is grasped before it is divided by 5."""
from typing import Any, Dict

import numpy as np
import sapien
import torch
from transforms3d.euler import euler2quat

from maniskill_amd.envs.sapien_env import BaseEnv
from maniskill_amd.sensors.camera import CameraConfig
from maniskill_amd.utils import sapien_utils
from maniskill_amd.utils.building import actors
from maniskill_amd.utils.geometry import rotation_conversions
from maniskill_amd.utils.registration import register_env
from maniskill_amd.utils.scene_builder.table import TableSceneBuilder
from maniskill_amd.utils.structs.pose import Pose


@register_env("LiftPegUpright-v1", max_episode_steps=50)
class LiftPegUprightEnv(BaseEnv):
    SUPPORTED_ROBOTS = ["panda", "fetch"]
    peg_half_width = 0.025
    peg_half_length = 0.12

    def __init__(self, *args, robot_uids="panda", robot_init_qpos_noise=0.02, **kwargs):
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
        self.table_scene = TableSceneBuilder(env=self, robot_init_qpos_noise=self.robot_init_qpos_noise)
        self.table_scene.build()
        self.peg = actors.build_twocolor_peg(
            self.scene, length=self.peg_half_length, width=self.peg_half_width, color_1=np.array([176, 14, 14, 255]) / 255,
            color_2=np.array([12, 42, 160, 255]) / 255, name="peg", body_type="dynamic", initial_pose=sapien.Pose(p=[0, 0, 0.1]),
        )

    def _initialize_episode(self, env_idx: torch.Tensor, options: dict):
        dev = self.device  # explicit devices, see PickCubeEnv._initialize_episode
        b = len(env_idx)
        self.table_scene.initialize(env_idx)
        xyz = torch.zeros((b, 3), device=dev)
        xyz[..., :2] = torch.rand((b, 2), device=dev) * 0.2 - 0.1
        xyz[..., 2] = self.peg_half_width
        self.peg.set_pose(Pose.create_from_pq(p=xyz, q=euler2quat(np.pi / 2, 0, 0)))

    def evaluate(self):
        qmat = rotation_conversions.quaternion_to_matrix(self.peg.pose.q)
        euler = rotation_conversions.matrix_to_euler_angles(qmat, "XYZ")
        is_peg_upright = torch.abs(torch.abs(euler[:, 2]) - np.pi / 2) < 0.08
        close_to_table = torch.abs(self.peg.pose.p[:, 2] - self.peg_half_length) < 0.005
        return {"success": is_peg_upright & close_to_table}

    def _get_obs_extra(self, info: Dict):
        obs = dict(tcp_pose=self.agent.tcp.pose.raw_pose)
        if self.obs_mode_struct.use_state:
            obs.update(obj_pose=self.peg.pose.raw_pose)
        return obs

    def compute_dense_reward(self, obs: Any, action, info: Dict):
        # the peg's axis (its x axis) against the vertical: |cos| of the angle between them, (0, 0, -1) is as good
        qmats = rotation_conversions.quaternion_to_matrix(self.peg.pose.q)
        vec = torch.tensor([1.0, 0, 0], device=self.device)
        goal_vec = torch.tensor([0, 0, 1.0], device=self.device)
        rot_vec = (qmats @ vec).view(-1, 3)
        reward = (rot_vec @ goal_vec).view(-1).abs()
        # the centre half a length above the table
        z_dist = torch.abs(self.peg.pose.p[:, 2] - self.peg_half_length)
        reward += 1 - torch.tanh(5 * z_dist)
        # a small reaching term, granted in full while the peg is grasped
        to_grip_dist = torch.linalg.norm(self.peg.pose.p - self.agent.tcp.pose.p, axis=1)
        reaching_rew = 1 - torch.tanh(5 * to_grip_dist)
        reaching_rew[self.agent.is_grasping(self.peg)] = 1
        reward += reaching_rew / 5
        reward[info["success"]] = 3
        return reward

    def compute_normalized_dense_reward(self, obs: Any, action, info: Dict):
        return self.compute_dense_reward(obs=obs, action=action, info=info) / 3.0

    # ---- fused evaluate + obs + reward (one native launch after the control step's; tests/test_gpu_poke_lift.py) ----
    def _fused_task_ok(self) -> bool:
        cls = type(self)
        same = all(
            getattr(cls, m) is getattr(LiftPegUprightEnv, m)
            for m in ("evaluate", "_get_obs_extra", "compute_dense_reward", "compute_normalized_dense_reward", "_get_obs_agent", "get_obs", "get_info", "get_reward")
        )
        from maniskill_amd.envs.utils.task_robot import fused_robot_ok

        return (same and fused_robot_ok(self, ("panda",)) and self._obs_mode == "state"
                and self._reward_mode in ("dense", "normalized_dense") and len(self.agent.controller.get_state()) == 0)

    def _fused_step_outputs(self, action, advance: bool = True):
        if not self._fused_ok():
            return None
        from maniskill_amd import native
        from maniskill_amd.envs.utils.task_robot import fused_robot_rows

        px = self.scene.px
        st = getattr(self, "_fused_state", None)
        if st is None or st["px"] is not px:
            finger1_row, finger2_row = fused_robot_rows(self)
            task = native.LiftPegTask(
                tcp_row=self.agent.tcp._body_row, peg_row=self.peg._body_row,
                finger1_row=finger1_row, finger2_row=finger2_row,
                peg_half_length=self.peg_half_length, upright_thresh=0.08, height_thresh=0.005, min_force=0.5, max_angle_deg=85.0,
                reward_scale=1.0 / 3.0 if self._reward_mode == "normalized_dense" else 1.0,
            )
            st = self._fused_state = dict(px=px, task=task)
        N, D = self.num_envs, 2 * self.agent.robot.max_dof + 14
        obs = torch.empty((N, D), dtype=torch.float32, device=self.device)
        reward = torch.empty((N,), dtype=torch.float32, device=self.device)
        flags = torch.empty((N, 1), dtype=torch.uint8, device=self.device)
        es = self._fused_bind_counters(st["task"], advance)
        px.task_liftpeg_outputs(st["task"], obs, reward, flags)
        return obs, reward, dict(elapsed_steps=es, success=flags.view(torch.bool)[:, 0])
