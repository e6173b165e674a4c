"""DrawTriangle-v1 (task definition restated from mani_skill/envs/tasks/drawing/draw_triangle.py:22-386): a white canvas
lies on the table with the dark outline of an equilateral triangle (0.3 m edges) at a random place and yaw; the panda_stick
draws on the canvas by bringing its tip down: at every control step a "dot" is placed under the tip if the tip is below
0.028 m. Success = every dot drawn lies within 25 mm of one of the 153 reference points of the outline, and every reference
point has a dot within 25 mm.

The drawing is a per-env table, not actors. The reference keeps 300 kinematic dot actors per env and moves one per step;
here `env.dots` is a float32 tensor [N, 300, 2] of xy positions, `env.dot_near` an int8 [N, 300] with the reference's
`dots_dist` values (-1 not drawn, 0 drawn away from the outline, 1 drawn near it), `env.ref_hit` a bool [N, 153] and
`env.draw_step` an int32 [N] counter. `env.dots` is NOT a list of actors: there is no `env.dots[i].pose`. The dots have no
collision and never move once placed, so the simulation holds no row for them; the shaded view paints them from the table.

Kept from the reference: dot k is written at control step k of the episode whether or not the tip touches (an untouched
step leaves a "not drawn" entry, so an episode of 300 steps uses the whole table), the strict comparisons, the key order of
the observation. NOT kept: the reference reduces `torch.all(dots_dist[mask])` over the whole batch and keeps one `draw_step`
for all envs, which any partial reset sets to zero. Here both are per env: an env succeeds iff every one of ITS drawn dots is
near and all of ITS reference points are hit, and its counter restarts at its own reset. With num_envs = 1 the two readings
coincide. A step past the table (a 301st without a reset) draws nothing.

The table is updated by `_after_control_step` on the torch path and by the native epilogue (mssim_task_draw_outputs,
include/mssim_hip_tasks.h) where that runs; both keep the tensors' addresses. tests/test_gpu_draw_triangle.py holds the two
against each other and against tests/draw_reference.py."""
import math
from typing import Dict

import numpy as np
import sapien
import torch
from transforms3d.euler import euler2quat

from maniskill_amd.envs.sapien_env import BaseEnv
from maniskill_amd.envs.utils import randomization
from maniskill_amd.sensors.camera import CameraConfig
from maniskill_amd.utils import sapien_utils
from maniskill_amd.utils.geometry.rotation_conversions import quaternion_to_matrix
from maniskill_amd.utils.registration import register_env
from maniskill_amd.utils.scene_builder.table import TableSceneBuilder
from maniskill_amd.utils.structs.pose import Pose
from maniskill_amd.utils.structs.types import SceneConfig, SimConfig


@register_env("DrawTriangle-v1", max_episode_steps=300)
class DrawTriangleEnv(BaseEnv):
    MAX_DOTS = 300  # the "ink": dots per episode
    DOT_THICKNESS = 0.003
    CANVAS_THICKNESS = 0.02
    BRUSH_RADIUS = 0.01
    BRUSH_COLORS = [[0.8, 0.2, 0.2, 1]]
    THRESHOLD = 0.025
    N_REF = 153  # 3 edges x 51 points

    SUPPORTED_REWARD_MODES = ("sparse", "none")
    SUPPORTED_ROBOTS = ["panda_stick"]

    def __init__(self, *args, robot_uids="panda_stick", **kwargs):
        super().__init__(*args, robot_uids=robot_uids, **kwargs)

    @property
    def _default_sim_config(self):
        # few contacts are expected (the tip on the canvas at most) and the brush is part of the robot: a small contact
        # offset and four position sweeps, no velocity sweep. The control step honours all three.
        return SimConfig(sim_freq=100, control_freq=20, scene_config=SceneConfig(contact_offset=0.01, solver_position_iterations=4, solver_velocity_iterations=0))

    @property
    def _default_sensor_configs(self):
        pose = sapien_utils.look_at(eye=[0.3, 0, 0.8], target=[0, 0, 0.1])
        return [CameraConfig("base_camera", pose=pose, width=320, height=240, fov=1.2, near=0.01, far=100)]

    @property
    def _default_human_render_camera_configs(self):
        pose = sapien_utils.look_at(eye=[0.3, 0, 0.8], target=[0, 0, 0.1])
        return CameraConfig("render_camera", pose=pose, width=1280, height=960, fov=1.2, near=0.01, far=100)

    def _load_agent(self, options: dict):
        super()._load_agent(options, sapien.Pose(p=[-0.615, 0, 0]))

    def _create_goal_triangle(self, name, base_color):
        """three thin visual boxes, the edges of an equilateral triangle about the body's origin; kinematic, no collision"""
        half_w, half_h, half_thickness = 0.3 / 2, 0.01 / 2, 0.001 / 2
        radius = half_w / math.sqrt(3)
        theta = np.pi / 2
        c = [np.array([radius * math.cos(theta + k * 2 * np.pi / 3), radius * math.sin(theta + k * 2 * np.pi / 3), 0.01]) for k in range(3)]
        self.original_verts = np.array([(c[0] + c[2]) - c[1], (c[0] + c[1]) - c[2], (c[1] + c[2]) - c[0]])
        builder = self.scene.create_actor_builder()
        for centre, yaw in zip(c, (theta - np.pi / 2, theta - 5 * np.pi / 6, theta - np.pi / 6)):
            builder.add_box_visual(pose=sapien.Pose(list(centre), euler2quat(0, 0, yaw)), half_size=[half_w, half_h, half_thickness], material=base_color)
        builder.initial_pose = sapien.Pose(p=[0, 0, 0.1])
        return builder.build_kinematic(name=name)

    def _load_scene(self, options: dict):
        self._fused_state = None
        self.table_scene = TableSceneBuilder(self, robot_init_qpos_noise=0)
        self.table_scene.build()
        half = [0.4, 0.6, self.CANVAS_THICKNESS / 2]
        builder = self.scene.create_actor_builder()
        builder.add_box_visual(half_size=half, material=[1, 1, 1, 1])
        builder.add_box_collision(half_size=half)
        builder.initial_pose = sapien.Pose(p=[-0.1, 0, self.CANVAS_THICKNESS / 2])
        self.canvas = builder.build_static(name="canvas")
        self.goal_tri = self._create_goal_triangle("goal_tri", np.array([10, 10, 10, 255]) / 255)
        # the drawing and the goal's geometry: on the device from the start and never replaced (the native epilogue reads
        # and writes them in place)
        N, dev = self.num_envs, self.device
        self.dots = torch.zeros((N, self.MAX_DOTS, 2), dtype=torch.float32, device=dev)
        self.dot_near = torch.full((N, self.MAX_DOTS), -1, dtype=torch.int8, device=dev)
        self.ref_hit = torch.zeros((N, self.N_REF), dtype=torch.bool, device=dev)
        self.draw_step = torch.zeros(N, dtype=torch.int32, device=dev)
        self.vertices = torch.zeros((N, 3, 3), dtype=torch.float32, device=dev)
        self.triangles = torch.zeros((N, self.N_REF, 2), dtype=torch.float32, device=dev)
        self._dot_appended = False
        # the two thresholds as float32 values, so that every path compares with the same number
        self.z_thresh = float(np.float32(self.CANVAS_THICKNESS + self.DOT_THICKNESS + 0.005))
        self.near_thresh2 = float(np.float32(self.THRESHOLD**2))

    def _initialize_episode(self, env_idx: torch.Tensor, options: dict):
        dev = self.device  # explicit devices, see PickCubeEnv._initialize_episode
        b = len(env_idx)
        self.table_scene.initialize(env_idx)
        target_pos = torch.zeros((b, 3), device=dev)
        target_pos[:, :2] = torch.rand((b, 2), device=dev) * 0.02 - 0.1
        target_pos[:, -1] = 0.01
        qs = randomization.random_quaternions(b, dev, lock_x=True, lock_y=True)
        self.goal_tri.set_pose(Pose.create_from_pq(p=target_pos, q=qs))
        # corners and reference points in float64, as the reference computes them, rounded once to the float32 the
        # observation and the native epilogue carry
        verts = torch.from_numpy(self.original_verts).to(dev).expand(b, 3, 3)
        verts = (quaternion_to_matrix(qs).double() @ verts.transpose(-1, -2)).transpose(-1, -2) + target_pos.double().unsqueeze(1)
        self.vertices[env_idx] = verts.float()
        self.triangles[env_idx] = self.generate_triangle_with_points(50, verts[:, :, :-1]).float()
        self.dots[env_idx] = 0.0
        self.dot_near[env_idx] = -1
        self.ref_hit[env_idx] = False
        self.draw_step[env_idx] = 0

    @staticmethod
    def generate_triangle_with_points(n, vertices):
        """[b, 3, 2] corners -> [b, 3 (n + 1), 2]: per edge the points at linspace(0, 1, n + 2)[:-1] from its first corner"""
        t = torch.linspace(0, 1, n + 2, device=vertices.device)[:-1].to(vertices.dtype).view(1, -1, 1)
        edges = []
        for i in range(vertices.shape[1]):
            start, end = vertices[:, i, :].unsqueeze(1), vertices[:, (i + 1) % vertices.shape[1], :].unsqueeze(1)
            edges.append(start * (1 - t) + end * t)
        return torch.cat(edges, dim=1)

    def _after_control_step(self):
        """the torch path's dot append (the native epilogue does the same where the step takes it: `_no_step_hooks`)"""
        self.scene._gpu_fetch_all()
        self._append_dot()
        self._dot_appended = True

    def _append_dot(self):
        """dot draw_step[e] of every env from its tcp, and what it hits; a counter at MAX_DOTS appends nothing"""
        N, ar = self.num_envs, torch.arange(self.num_envs, device=self.device)
        tcp = self.agent.tcp.pose.p
        live = self.draw_step < self.MAX_DOTS
        k = self.draw_step.clamp(max=self.MAX_DOTS - 1).long()
        drawn = live & (tcp[:, 2] < self.z_thresh)
        xy = torch.where(drawn.unsqueeze(1), tcp[:, :2], torch.zeros_like(tcp[:, :2]))
        dx, dy = tcp[:, 0:1] - self.triangles[..., 0], tcp[:, 1:2] - self.triangles[..., 1]
        hit = drawn.unsqueeze(1) & (dx * dx + dy * dy < self.near_thresh2)
        near = torch.where(drawn, hit.any(1).to(torch.int8), torch.full((N,), -1, dtype=torch.int8, device=self.device))
        self.dots[ar, k] = torch.where(live.unsqueeze(1), xy, self.dots[ar, k])
        self.dot_near[ar, k] = torch.where(live, near, self.dot_near[ar, k])
        self.ref_hit |= hit
        self.draw_step += live.to(torch.int32)

    def evaluate(self):
        return {"success": (self.dot_near != 0).all(1) & self.ref_hit.all(1)}

    def _get_obs_extra(self, info: Dict):
        obs = dict(tcp_pose=self.agent.tcp.pose.raw_pose)
        if self.obs_mode_struct.use_state:
            N = self.num_envs
            obs.update(
                goal_pose=self.goal_tri.pose.raw_pose.reshape(N, -1),
                tcp_to_verts_pos=(self.vertices - self.agent.tcp.pose.p.unsqueeze(1)).reshape(N, -1),
                goal_pos=self.goal_tri.pose.p.reshape(N, -1),
                vertices=self.vertices.reshape(N, -1),
            )
        return obs

    # ---- the drawing in the shaded view: discs on the canvas, painted over the viewer's picture ----
    def _picture_overlay(self, camera):
        if not camera._rig.viewer:  # the sensors' views keep to the collision geometry
            return
        from maniskill_amd import native

        r, g, b = (int(math.floor(255 * min(c, 1.0) + 0.5)) for c in self.BRUSH_COLORS[0][:3])  # (both lights reach an upward face: the albedo itself)
        layer = native.DotLayer(dots=self.dots.data_ptr(), dot_near=self.dot_near.data_ptr(), count=self.draw_step.data_ptr(), max_dots=self.MAX_DOTS,
                                z=self.CANVAS_THICKNESS + self.DOT_THICKNESS, radius=self.BRUSH_RADIUS, rgba=r | (g << 8) | (b << 16) | (255 << 24))
        camera.draw_dots(layer)

    # ---- fused dot append + evaluate + obs (one native launch after the control step's; tests/test_gpu_draw_triangle.py) ----
    def _no_step_hooks(self) -> bool:
        """the dot append is this task's one step hook, and the native epilogue performs it: with that epilogue next, the
        control step may run as the one deferred launch"""
        cls = type(self)
        mine = (cls._after_control_step is DrawTriangleEnv._after_control_step and cls._before_control_step is BaseEnv._before_control_step
                and not self._substep_hooks_overridden() and hasattr(self.scene.px, "step_action"))
        return bool(self._fused_epilogue_next) and mine and not getattr(self.agent.controller, "needs_per_substep_update", False)

    def _fused_task_ok(self) -> bool:
        cls = type(self)
        same = all(
            getattr(cls, m) is getattr(DrawTriangleEnv, m)
            for m in ("evaluate", "_append_dot", "_after_control_step", "_get_obs_extra", "_get_obs_agent", "get_obs", "get_info", "get_reward", "compute_sparse_reward")
        )
        return (same and self.robot_uids == "panda_stick" and self._obs_mode == "state" and self._reward_mode in ("sparse", "none")
                and len(self.agent.controller.get_state()) == 0)

    def _fused_step_outputs(self, action, advance: bool = True):
        appended, self._dot_appended = self._dot_appended, False
        if not self._fused_ok():
            return None
        from maniskill_amd import native

        px = self.scene.px
        st = getattr(self, "_fused_state", None)
        if st is None or st["px"] is not px:
            task = native.DrawTask(
                tcp_row=self.agent.tcp._body_row, goal_row=self.goal_tri._body_row, vertices=self.vertices.data_ptr(), triangles=self.triangles.data_ptr(),
                dots=self.dots.data_ptr(), dot_near=self.dot_near.data_ptr(), ref_hit=self.ref_hit.data_ptr(), draw_step=self.draw_step.data_ptr(),
                max_dots=self.MAX_DOTS, n_ref=self.N_REF, z_thresh=self.z_thresh, near_thresh2=self.near_thresh2,
                reward_scale=1.0 if self._reward_mode == "sparse" else 0.0,
            )
            st = self._fused_state = dict(px=px, task=task)
        N, D = self.num_envs, 2 * self.agent.robot.max_dof + 35
        obs = torch.empty((N, D), dtype=torch.float32, device=self.device)
        reward = torch.empty((N,), dtype=torch.float32, device=self.device)
        flags = torch.empty((N, 1), dtype=torch.uint8, device=self.device)
        es = self._fused_bind_counters(st["task"], advance)
        # the dot is appended with a step's outputs only, and once: a reset's outputs (advance=False) read the tables, and so
        # does a step whose `_after_control_step` has run (an action the native map does not take)
        st["task"].update = int(advance and not appended)
        px.task_draw_outputs(st["task"], obs, reward, flags)
        return obs, reward, dict(elapsed_steps=es, success=flags.view(torch.bool)[:, 0])
