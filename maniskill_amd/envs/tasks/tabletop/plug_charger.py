"""PlugCharger-v1 (task definition restated from mani_skill/envs/tasks/tabletop/plug_charger.py:20-278):
pick up a two-pin charger and plug it into a receptacle that stands 10 cm above the table. Success = the charger within
5 mm and 0.2 rad of the goal pose, which is the receptacle's pose turned by pi about z. The charger is one dynamic body of
three boxes (a base and two 16 x 1.5 x 6.4 mm pegs), the receptacle a kinematic body of five boxes that leave two slots with
0.5 mm clearance per side: the smallest geometry of the project's tasks.
The reference's quirks are kept: the dense reward is zero, and the goal pose is computed at reset and stored, so a
receptacle moved afterwards leaves the goal where it was. Here the stored goal is a [N, 7] tensor written for the envs
being reset alone."""
from typing import Any, Dict

import numpy as np
import sapien
import torch
from transforms3d.euler import euler2quat

from maniskill_amd.envs.sapien_env import BaseEnv
from maniskill_amd.envs.utils import randomization
from maniskill_amd.sensors.camera import CameraConfig
from maniskill_amd.utils import sapien_utils
from maniskill_amd.utils.geometry import rotation_conversions
from maniskill_amd.utils.registration import register_env
from maniskill_amd.utils.scene_builder.table import TableSceneBuilder
from maniskill_amd.utils.structs.pose import Pose
from maniskill_amd.utils.structs.types import SimConfig


@register_env("PlugCharger-v1", max_episode_steps=200)
class PlugChargerEnv(BaseEnv):
    SUPPORTED_ROBOTS = ["panda_wristcam"]
    _base_size = [2e-2, 1.5e-2, 1.2e-2]  # charger base half size
    _peg_size = [8e-3, 0.75e-3, 3.2e-3]  # charger peg half size
    _peg_gap = 7e-3  # the pegs' centres lie this far from the charger's axis
    _clearance = 5e-4  # per side
    _receptacle_size = [1e-2, 5e-2, 5e-2]  # receptacle half size
    dist_thresh = 5e-3
    angle_thresh = 0.2

    def __init__(self, *args, robot_uids="panda_wristcam", robot_init_qpos_noise=0.02, **kwargs):
        self.robot_init_qpos_noise = robot_init_qpos_noise
        super().__init__(*args, robot_uids=robot_uids, **kwargs)

    @property
    def _default_sim_config(self):
        return SimConfig()

    @property
    def _default_sensor_configs(self):
        pose = sapien_utils.look_at(eye=[0.3, 0, 0.6], target=[-0.1, 0, 0.1])
        return [CameraConfig("base_camera", pose, 128, 128, np.pi / 2, 0.01, 100)]

    @property
    def _default_human_render_camera_configs(self):
        pose = sapien_utils.look_at([0.3, 0.4, 0.1], [0, 0, 0])
        return CameraConfig("render_camera", pose, 512, 512, 1, 0.01, 100, mount=self.receptacle)

    def _build_charger(self, peg_size, base_size, gap):
        """the pegs along +x from the body's origin, at +-gap in y; the base behind the origin"""
        builder = self.scene.create_actor_builder()
        for p, half in (([peg_size[0], gap, 0], peg_size), ([peg_size[0], -gap, 0], peg_size), ([-base_size[0], 0, 0], base_size)):
            builder.add_box_collision(sapien.Pose(p), half)
            builder.add_box_visual(sapien.Pose(p), half)
        builder.initial_pose = sapien.Pose(p=[0, 0, base_size[2]])
        return builder.build(name="charger")

    @staticmethod
    def receptacle_boxes(peg_size, receptacle_size, gap):
        """(position, half size) of the five boxes, in the receptacle's frame: the plates above and below the slots, the
        blocks outside them in y, and the filler between them. `peg_size` is the slot's half size (peg + clearance)."""
        sy = 0.5 * (receptacle_size[1] - peg_size[1] - gap)
        sz = 0.5 * (receptacle_size[2] - peg_size[2])
        dx = -receptacle_size[0]
        dy = peg_size[1] + gap + sy
        dz = peg_size[2] + sz
        return [
            ([dx, 0, dz], [receptacle_size[0], receptacle_size[1], sz]),
            ([dx, 0, -dz], [receptacle_size[0], receptacle_size[1], sz]),
            ([dx, dy, 0], [receptacle_size[0], sy, receptacle_size[2]]),
            ([dx, -dy, 0], [receptacle_size[0], sy, receptacle_size[2]]),
            ([dx, 0, 0], [receptacle_size[0], gap - peg_size[1], peg_size[2]]),
        ]

    def _build_receptacle(self, peg_size, receptacle_size, gap):
        builder = self.scene.create_actor_builder()
        for p, half in self.receptacle_boxes(peg_size, receptacle_size, gap):
            builder.add_box_collision(sapien.Pose(p), half)
            builder.add_box_visual(sapien.Pose(p), half)
        builder.initial_pose = sapien.Pose(p=[0, 0, 0.1])
        return builder.build_kinematic(name="receptacle")

    def _load_agent(self, options: dict):
        super()._load_agent(options, sapien.Pose(p=[-0.615, 0, 0]))

    def _load_scene(self, options: dict):
        self._fused_state = None
        self.scene_builder = TableSceneBuilder(self, robot_init_qpos_noise=self.robot_init_qpos_noise)
        self.scene_builder.build()
        self.charger = self._build_charger(self._peg_size, self._base_size, self._peg_gap)
        slot = [self._peg_size[0], self._peg_size[1] + self._clearance, self._peg_size[2] + self._clearance]
        self.receptacle = self._build_receptacle(slot, self._receptacle_size, self._peg_gap)
        # the stored goal, p and q(wxyz) per env: written by _initialize_episode in place (the native epilogue keeps its address)
        self._goal_pose_raw = torch.zeros((self.num_envs, 7), dtype=torch.float32, device=self.device)
        self._goal_pose_raw[:, 3] = 1.0

    def _initialize_episode(self, env_idx: torch.Tensor, options: dict):
        with torch.device(self.device):
            b = len(env_idx)
            self.scene_builder.initialize(env_idx)

            qpos = np.array([0.0, np.pi / 8, 0, -np.pi * 5 / 8, 0, np.pi * 3 / 4, np.pi / 4, 0.04, 0.04])
            if self._enhanced_determinism:  # per-env streams, as PegInsertionSideEnv._initialize_episode
                qpos = self._batched_episode_rng[env_idx].normal(0, self.robot_init_qpos_noise, len(qpos)) + qpos
            else:
                qpos = self._episode_rng.normal(0, self.robot_init_qpos_noise, (b, len(qpos))) + qpos
            qpos[:, -2:] = 0.04
            self.agent.robot.set_qpos(qpos)
            self.agent.robot.set_pose(sapien.Pose([-0.615, 0, 0]))

            xy = randomization.uniform(low=torch.tensor([-0.1, -0.2]), high=torch.tensor([-0.01 - self._peg_size[0] * 2, 0.2]), size=(b, 2))
            pos = torch.zeros((b, 3))
            pos[:, :2] = xy
            pos[:, 2] = self._base_size[2]
            ori = randomization.random_quaternions(b, self.device, lock_x=True, lock_y=True, bounds=(-np.pi / 3, np.pi / 3))
            self.charger.set_pose(Pose.create_from_pq(pos, ori))

            xy = randomization.uniform(low=torch.tensor([0.01, -0.1]), high=torch.tensor([0.1, 0.1]), size=(b, 2))
            pos = torch.zeros((b, 3))
            pos[:, :2] = xy
            pos[:, 2] = 0.1
            ori = randomization.random_quaternions(b, self.device, lock_x=True, lock_y=True, bounds=(np.pi - np.pi / 8, np.pi + np.pi / 8))
            receptacle_pose = Pose.create_from_pq(pos, ori)
            self.receptacle.set_pose(receptacle_pose)

            goal = receptacle_pose * sapien.Pose(q=euler2quat(0, 0, np.pi))
            self._goal_pose_raw[env_idx] = goal.raw_pose

    @property
    def goal_pose(self) -> Pose:
        """the goal as stored at reset (not the receptacle's current pose)"""
        return Pose.create(self._goal_pose_raw)

    @property
    def charger_base_pose(self):
        return self.charger.pose * sapien.Pose([-self._base_size[0], 0, 0])

    def _compute_distance(self):
        obj_pose, goal_pose = self.charger.pose, self.goal_pose
        obj_to_goal_dist = torch.linalg.norm(goal_pose.p - obj_pose.p, axis=1)
        obj_to_goal_quat = rotation_conversions.quaternion_multiply(rotation_conversions.quaternion_invert(goal_pose.q), obj_pose.q)
        obj_to_goal_angle = torch.linalg.norm(rotation_conversions.quaternion_to_axis_angle(obj_to_goal_quat), axis=1)
        obj_to_goal_angle = torch.min(obj_to_goal_angle, torch.pi * 2 - obj_to_goal_angle)
        return obj_to_goal_dist, obj_to_goal_angle

    def evaluate(self):
        obj_to_goal_dist, obj_to_goal_angle = self._compute_distance()
        success = (obj_to_goal_dist <= self.dist_thresh) & (obj_to_goal_angle <= self.angle_thresh)
        return dict(obj_to_goal_dist=obj_to_goal_dist, obj_to_goal_angle=obj_to_goal_angle, success=success)

    def _get_obs_extra(self, info: Dict):
        obs = dict(tcp_pose=self.agent.tcp.pose.raw_pose)
        if self.obs_mode_struct.use_state:
            obs.update(charger_pose=self.charger.pose.raw_pose, receptacle_pose=self.receptacle.pose.raw_pose, goal_pose=self.goal_pose.raw_pose)
        return obs

    def compute_dense_reward(self, obs: Any, action: torch.Tensor, info: Dict):
        return torch.zeros(self.num_envs, device=self.device)

    def compute_normalized_dense_reward(self, obs: Any, action: torch.Tensor, info: Dict):
        return self.compute_dense_reward(obs=obs, action=action, info=info) / 1.0

    # ---- fused evaluate + obs + reward (one native launch after the control step's; tests/test_gpu_plug_charger.py) ----
    def _fused_task_ok(self) -> bool:
        cls = type(self)
        same = all(
            getattr(cls, m) is getattr(PlugChargerEnv, m)
            for m in ("evaluate", "_compute_distance", "goal_pose", "_get_obs_extra", "compute_dense_reward", "compute_normalized_dense_reward", "_get_obs_agent",
                      "get_obs", "get_info", "get_reward")
        )
        from maniskill_amd.envs.utils.task_robot import fused_robot_ok

        # (no grasp and no static rule in this task: the robot matters through its state columns and its tcp alone)
        return (same and fused_robot_ok(self, ("panda_wristcam",)) and self._obs_mode == "state"
                and self._reward_mode in ("dense", "normalized_dense") and len(self.agent.controller.get_state()) == 0)

    def _fused_step_outputs(self, action, advance: bool = True):
        if not self._fused_ok():
            return None
        from maniskill_amd import native

        px = self.scene.px
        st = getattr(self, "_fused_state", None)
        goal = self._goal_pose_raw
        if st is None or st["px"] is not px or st["goal_ptr"] != goal.data_ptr():
            task = native.PlugTask(
                tcp_row=self.agent.tcp._body_row, charger_row=self.charger._body_row, receptacle_row=self.receptacle._body_row,
                goal_pose=goal.data_ptr(), dist_thresh=self.dist_thresh, angle_thresh=self.angle_thresh, reward_scale=1.0,
            )
            st = self._fused_state = dict(px=px, task=task, goal_ptr=goal.data_ptr())
        N, D = self.num_envs, 2 * self.agent.robot.max_dof + 28
        obs = torch.empty((N, D), dtype=torch.float32, device=self.device)
        reward = torch.empty((N,), dtype=torch.float32, device=self.device)
        flags = torch.empty((N, 1), dtype=torch.uint8, device=self.device)
        metrics = torch.empty((N, 2), dtype=torch.float32, device=self.device)
        es = self._fused_bind_counters(st["task"], advance)
        px.task_plug_outputs(st["task"], obs, reward, flags, metrics)
        info = dict(elapsed_steps=es, obj_to_goal_dist=metrics[:, 0], obj_to_goal_angle=metrics[:, 1], success=flags.view(torch.bool)[:, 0])
        return obs, reward, info
