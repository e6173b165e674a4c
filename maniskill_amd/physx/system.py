"""`px`-shaped system object over the native core.

Counterpart of `sapien.physx.PhysxGpuSystem` as ManiSkill uses it through `ManiSkillScene.px`
(mani_skill/envs/scene.py:60-68; complete method list in SURVEY.md 8b): `gpu_init`, `step`,
`timestep`, `gpu_apply_*`, `gpu_fetch_*`, `gpu_update_articulation_kinematics`, `cuda_*` buffers
with `.torch()`, contact impulse queries.

The default backend is the HIP library (`maniskill_amd/_native/libmssim.so`) on a `cuda:*`
(ROCm) device and raises if it is missing; other backends only exist if a caller registers them
(`register_backend`), which the package itself never does.
"""
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import native
from ..model.compile import CompiledModel


class CudaArray:
    """Mimics SAPIEN's `CudaArray`: `.torch()` returns the aliased tensor (structs/base.py:112-114)."""

    def __init__(self, tensor: torch.Tensor):
        self._t = tensor

    def torch(self) -> torch.Tensor:
        return self._t

    @property
    def shape(self):
        return tuple(self._t.shape)

    @property
    def ptr(self):
        return self._t.data_ptr()


class ContactPairImpulseQuery:
    def __init__(self, qid: int, impulses: torch.Tensor):
        self.id = qid
        self.cuda_impulses = CudaArray(impulses)


class ContactBodyImpulseQuery(ContactPairImpulseQuery):
    pass


# backend name -> factory(device) -> (NativeLib, native_device_ordinal)
_BACKENDS: Dict[str, Callable] = {}


def register_backend(name: str, factory: Callable):
    """Register an alternative native library for a sim backend name (used by tests to plug the
    CPU oracle in as `physx_cpu`; the package registers nothing but the HIP library)."""
    _BACKENDS[name] = factory


def _hip_backend(device: torch.device):
    if device.type != "cuda":
        raise RuntimeError(
            f"maniskill_amd's simulation backend is HIP-only: device {device} is not a ROCm GPU. "
            "There is no CPU fallback (register a backend explicitly for tests)."
        )
    if not torch.cuda.is_available():
        raise RuntimeError("no ROCm GPU visible: the HIP simulation core cannot run")
    lib = native.NativeLib.load()  # raises NativeError when libmssim.so is not built
    return lib, (device.index if device.index is not None else torch.cuda.current_device())


_BACKENDS["physx_cuda"] = _hip_backend


class MssimSystem:
    """Batched rigid-body system for `num_envs` identical environments."""

    def __init__(self, device="cuda", backend: str = "physx_cuda"):
        self.device = torch.device(device)
        self.backend = backend
        if backend not in _BACKENDS:
            raise RuntimeError(
                f"sim backend {backend!r} is not available; only the HIP backend 'physx_cuda' ships with this package"
            )
        self._lib, self._dev_ordinal = _BACKENDS[backend](self.device)
        self._timestep = 0.01
        self.model: Optional[CompiledModel] = None
        self.num_envs = 0
        self._sim: Optional[native.NativeSim] = None
        self._queries: List = []
        self._raycast_keep: Dict[int, tuple] = {}  # ray-cast scene id -> (tensors its cameras point to, the cameras' (width, height))

    # ------------------------------------------------------------------ lifecycle
    @property
    def timestep(self) -> float:
        return self._timestep

    @timestep.setter
    def timestep(self, dt: float):
        self._timestep = float(dt)
        if self._sim is not None:
            self._sim.set_timestep(self._timestep)

    @property
    def is_initialized(self):
        return self._sim is not None

    def _stream(self):
        if self.device.type == "cuda":
            return torch.cuda.current_stream(self.device).cuda_stream
        return None

    def gpu_init(self, model: CompiledModel, num_envs: int):
        """px.gpu_init() (scene.py:905): compile-time tables are uploaded, state buffers allocated
        and filled with the builders' initial poses."""
        assert self._sim is None, "gpu_init called twice"
        self.model, self.num_envs = model, int(num_envs)
        model.scalars["timestep"] = self._timestep
        if model.scalars.get("n_env_shape", 0) or model.scalars.get("n_env_free", 0):
            assert model.scalars["num_envs"] == self.num_envs, "model with per-env geometry was compiled for a different num_envs"
        else:
            model.scalars["num_envs"] = self.num_envs
        N, R, n = self.num_envs, model.n_rows, model.n_dof
        dev = self.device
        f = dict(dtype=torch.float32, device=dev)
        self._rigid = torch.zeros((max(R, 1) * N, 13), **f)
        self._rigid[:, 3] = 1.0
        self._force = torch.zeros((max(R, 1) * N, 4), **f)
        nd = max(n, 1)
        self._qpos = torch.zeros((N, nd), **f)
        self._qvel = torch.zeros((N, nd), **f)
        self._qacc = torch.zeros((N, nd), **f)
        self._qf = torch.zeros((N, nd), **f)
        self._tqpos = torch.zeros((N, nd), **f)
        self._tqvel = torch.zeros((N, nd), **f)
        self.cuda_rigid_body_data = CudaArray(self._rigid)
        self.cuda_rigid_body_force = CudaArray(self._force)
        self.cuda_articulation_qpos = CudaArray(self._qpos)
        self.cuda_articulation_qvel = CudaArray(self._qvel)
        self.cuda_articulation_qacc = CudaArray(self._qacc)
        self.cuda_articulation_qf = CudaArray(self._qf)
        self.cuda_articulation_target_qpos = CudaArray(self._tqpos)
        self.cuda_articulation_target_qvel = CudaArray(self._tqvel)
        if dev.type == "cuda":
            with torch.cuda.device(dev):
                self._sim = native.NativeSim(self._lib, model, N, self._dev_ordinal)
        else:
            self._sim = native.NativeSim(self._lib, model, N, -1)
        self._sim.bind(
            rigid_body_data=self._rigid.data_ptr(),
            rigid_body_force=self._force.data_ptr(),
            art_qpos=self._qpos.data_ptr(),
            art_qvel=self._qvel.data_ptr(),
            art_qacc=self._qacc.data_ptr(),
            art_qf=self._qf.data_ptr(),
            art_target_qpos=self._tqpos.data_ptr(),
            art_target_qvel=self._tqvel.data_ptr(),
        )
        # initial poses from the builders
        A = model.arrays
        if model.n_link > 0:
            self._rigid[0:N, :7] = torch.from_numpy(A["init_root_pose"]).to(dev)
        for b in range(model.n_free):
            r = model.n_link + b
            self._rigid[r * N : (r + 1) * N, :7] = torch.from_numpy(A["init_free_pose"][b]).to(dev)
        for k in range(model.n_kin):
            r = model.n_link + model.n_free + k
            self._rigid[r * N : (r + 1) * N, :7] = torch.from_numpy(A["init_kin_pose"][k]).to(dev)
        self._sim.apply(native.ALL, self._stream())
        self._sim.update_kinematics(self._stream())
        self._sim.fetch(native.ALL, self._stream())

    def close(self):
        if self._sim is not None:
            self._sim.close()
            self._sim = None

    # ------------------------------------------------------------------ stepping
    def step(self, n_substeps: int = 1):
        """px.step() (scene.py:374-375). `n_substeps > 1` fuses the substep loop of
        BaseEnv._step_action (sapien_env.py:1016-1021) into one native call."""
        self._sim.step(n_substeps, self._stream())

    def gpu_update_articulation_kinematics(self):
        self._sim.update_kinematics(self._stream())

    def wake_all(self):
        """wake every sleeping free body (their sleep counters are state the buffers do not carry; include/mssim.h)"""
        self._sim.wake_all(self._stream())

    def wake_envs(self, env_idx: torch.Tensor):
        """the same for the listed envs (an int64 index tensor on the system's device): what a reset of those envs does to the
        hidden state (include/mssim.h `wake_envs`); no host synchronisation"""
        idx = env_idx.to(device=self.device, dtype=torch.int64).contiguous()
        self._sim.wake_envs(idx.data_ptr(), int(idx.numel()), self._stream())

    # ------------------------------------------------------------------ apply / fetch
    def _apply(self, what):
        self._sim.apply(what, self._stream())

    def _fetch(self, what):
        self._sim.fetch(what, self._stream())

    def gpu_apply_rigid_dynamic_data(self):
        self._apply(native.RIGID_DATA)

    def gpu_apply_articulation_qpos(self):
        self._apply(native.ART_QPOS)

    def gpu_apply_articulation_qvel(self):
        self._apply(native.ART_QVEL)

    def gpu_apply_articulation_qf(self):
        self._apply(native.ART_QF)

    def gpu_apply_articulation_root_pose(self):
        self._apply(native.ART_ROOT_POSE)

    def gpu_apply_articulation_root_velocity(self):
        self._apply(native.ART_ROOT_VEL)

    def gpu_apply_articulation_target_position(self):
        self._apply(native.ART_TARGET_POS)

    def gpu_apply_articulation_target_velocity(self):
        self._apply(native.ART_TARGET_VEL)

    def gpu_apply_rigid_dynamic_force(self):
        self._apply(native.RIGID_FORCE)

    def gpu_apply_all(self):
        self._apply(native.ALL)

    def gpu_fetch_rigid_dynamic_data(self):
        self._fetch(native.RIGID_DATA)

    def gpu_fetch_articulation_link_pose(self):
        self._fetch(native.LINK_POSE)

    def gpu_fetch_articulation_link_velocity(self):
        self._fetch(native.LINK_VEL)

    def gpu_fetch_articulation_qpos(self):
        self._fetch(native.ART_QPOS)

    def gpu_fetch_articulation_qvel(self):
        self._fetch(native.ART_QVEL)

    def gpu_fetch_articulation_qacc(self):
        self._fetch(native.ART_QACC)

    def gpu_fetch_articulation_target_qpos(self):
        self._fetch(native.ART_TARGET_POS)

    def gpu_fetch_articulation_target_qvel(self):
        self._fetch(native.ART_TARGET_VEL)

    def gpu_fetch_all(self):
        self._fetch(native.ALL)

    def defer_fetch_all(self):
        """gpu_fetch_all owed to the next native call: the task epilogue that follows performs it inside its own
        launch (include/mssim.h `defer_fetch`). Only for callers that issue that call next."""
        self._sim.defer_fetch(native.ALL)

    # ------------------------------------------------------------------ contact queries
    def gpu_create_contact_pair_impulse_query(self, body_pairs: Sequence[Tuple[int, int]]) -> ContactPairImpulseQuery:
        """body_pairs: (row_a, row_b) body rows of `cuda_rigid_body_data` (row index // num_envs),
        -1 for the static world (scene.py:769-772)."""
        pairs = np.asarray(body_pairs, dtype=np.int32).reshape(-1, 2)
        qid = self._sim.create_pair_query(pairs)
        out = torch.zeros((len(pairs) * self.num_envs, 3), dtype=torch.float32, device=self.device)
        q = ContactPairImpulseQuery(qid, out)
        self._queries.append(q)
        return q

    def gpu_query_contact_pair_impulses(self, query: ContactPairImpulseQuery):
        self._sim.query_pair_impulses(query.id, query.cuda_impulses.ptr, self._stream())

    def gpu_create_contact_body_impulse_query(self, body_rows: Sequence[int]) -> ContactBodyImpulseQuery:
        rows = np.asarray(body_rows, dtype=np.int32).reshape(-1)
        qid = self._sim.create_body_query(rows)
        out = torch.zeros((len(rows) * self.num_envs, 3), dtype=torch.float32, device=self.device)
        q = ContactBodyImpulseQuery(qid, out)
        self._queries.append(q)
        return q

    def gpu_query_contact_body_impulses(self, query: ContactBodyImpulseQuery):
        self._sim.query_body_impulses(query.id, query.cuda_impulses.ptr, self._stream())

    # ------------------------------------------------------------------ misc
    def set_drive_properties(self, drive: np.ndarray):
        self.model.arrays["dof_drive"] = np.ascontiguousarray(drive, dtype=np.float32)
        if self._sim is not None:
            self._sim.set_drive_properties(drive)

    def read_internal(self, name: str, max_items: int) -> torch.Tensor:
        out = torch.zeros((max_items, self.num_envs), dtype=torch.float32, device=self.device)
        n = self._sim.read_internal(name, out.data_ptr(), max_items, self._stream())
        return out[:n]

    def link_jacobian(self, link_index: int) -> torch.Tensor:
        """[N, 6, n_dof] geometric Jacobian (linear; angular) of articulation link `link_index` in the root
        frame at the current simulation state (include/mssim.h `link_jacobian`)"""
        out = torch.empty((self.num_envs, 6, self.model.n_dof), dtype=torch.float32, device=self.device)
        self._sim.link_jacobian(link_index, out.data_ptr(), self._stream())
        return out

    # ------------------------------------------------------------------ fused callers (HIP only)
    @property
    def supports_fused_callers(self) -> bool:
        return self.backend == "physx_cuda"

    def set_action_map(self, column, low, high, flags):
        self._sim.set_action_map(column, low, high, flags)

    def set_ee_action_map(self, ee):
        """end-effector block of the action map: `(link_index, column0, rows, low, high, rot_scale, flags)` or None"""
        if ee is None:
            self._sim.set_ee_action_map(-1, 0, 3, 0.0, 0.0, 0.0, 0)
        else:
            self._sim.set_ee_action_map(*ee)

    IK_DEFAULTS = dict(max_iters=60, damping=1e-3, max_step=0.3, tolerance=1e-5)  # Kinematics.compute_ik's iterative branch

    def set_ee_ik_map(self, ik, target_pose: torch.Tensor = None, **settings):
        """iterative-IK block of the action map (include/mssim_hip_tasks.h `set_ee_ik_map`; HIP library only):
        `ik` = `(link_index, column0, rows, mode, low, high, rot_scale, flags)` or None to remove the block;
        `target_pose` [N, 7] f32 is the block's state, read and written in place by every apply (kept alive here);
        `settings` override IK_DEFAULTS. Call `set_action_map` first: it flags the dofs the block drives."""
        if ik is None:
            if self._sim.lib.set_ee_ik_map is not None:  # (a library without the block has none to remove)
                self._sim.set_ee_ik_map(native.EeIkMap(link_index=-1), None)
            self._ik_target_pose = None
            return
        assert target_pose.dtype == torch.float32 and target_pose.is_contiguous() and tuple(target_pose.shape) == (self.num_envs, 7)
        link, column0, rows, mode, low, high, rot_scale, flags = ik
        s = dict(self.IK_DEFAULTS, **settings)
        m = native.EeIkMap(int(link), int(column0), int(rows), int(mode), float(low), float(high), float(rot_scale), int(flags),
                           int(s["max_iters"]), float(s["damping"]), float(s["max_step"]), float(s["tolerance"]))
        self._sim.set_ee_ik_map(m, target_pose.data_ptr())
        self._ik_target_pose = target_pose

    def ee_ik_solve(self, target_pose: torch.Tensor, q0: torch.Tensor = None, return_iters: bool = False):
        """the solve of the block set last, alone: joint positions [N, n_dof] whose path dofs reach `target_pose`
        [N, 7] (root frame), started from `q0` [N, n_dof] (None: the visible qpos); dofs off the path are copied"""
        n = self.model.n_dof
        assert target_pose.dtype == torch.float32 and target_pose.is_contiguous() and tuple(target_pose.shape) == (self.num_envs, 7)
        assert q0 is None or (q0.dtype == torch.float32 and q0.is_contiguous() and tuple(q0.shape) == (self.num_envs, n))
        out = torch.empty((self.num_envs, n), dtype=torch.float32, device=self.device)
        iters = torch.empty(self.num_envs, dtype=torch.int32, device=self.device) if return_iters else None
        self._sim.ee_ik_solve(target_pose.data_ptr(), None if q0 is None else q0.data_ptr(), out.data_ptr(),
                              None if iters is None else iters.data_ptr(), self._stream())
        return (out, iters) if return_iters else out

    def apply_action(self, action: torch.Tensor):
        """affine action -> drive targets in one launch (include/mssim.h `apply_action`)"""
        assert action.dtype == torch.float32 and action.is_contiguous() and action.shape[0] == self.num_envs
        self._sim.apply_action(action.data_ptr(), action.shape[1], self._stream())

    def step_action(self, action: torch.Tensor, n_substeps: int, defer: bool = False):
        """`apply_action` + `step(n_substeps)` in one launch (include/mssim.h `step_action`). `defer`: owed to the
        next native call -- a task epilogue then runs the whole control step as one launch (`defer_step_action`);
        the action tensor is kept alive until that call."""
        assert action.dtype == torch.float32 and action.is_contiguous() and action.shape[0] == self.num_envs
        if defer:
            self._deferred_action = action
            self._sim.defer_step_action(action.data_ptr(), action.shape[1], n_substeps, self._stream())
        else:
            self._sim.step_action(action.data_ptr(), action.shape[1], n_substeps, self._stream())

    task_robot = None  # the profile set last (a tuple of ranges, signed, norm dofs), None: the rules of the task structs

    def set_task_robot(self, ranges=None, signed_compare: bool = False, pick_norm_dofs: int = 0):
        """robot profile of the task epilogues (include/mssim_hip_tasks.h `mssim_set_task_robot`; HIP library only):
        `ranges` = up to two `(first joint, joint count, threshold)` of the robot's is_static, compared signed or by
        absolute value; `pick_norm_dofs` = leading joints of PickCube's reward norm. `ranges=None` removes the profile.
        While one is set every epilogue is a launch of its own."""
        if not ranges:
            if self._sim.lib.set_task_robot is not None:  # (a library without profiles has none to remove)
                self._sim.set_task_robot(None)
            self.task_robot = None
            return
        r = native.TaskRobot(n_ranges=len(ranges), signed_compare=int(bool(signed_compare)), pick_norm_dofs=int(pick_norm_dofs))
        for i, (first, count, thresh) in enumerate(ranges):
            r.first[i], r.count[i], r.thresh[i] = int(first), int(count), float(thresh)
        self._sim.set_task_robot(r)
        self.task_robot = (tuple((int(a), int(b), float(c)) for a, b, c in ranges), bool(signed_compare), int(pick_norm_dofs))

    def task_peg_outputs(self, task, obs: torch.Tensor, reward: torch.Tensor, flags: torch.Tensor, head: torch.Tensor):
        self._sim.task_peg_outputs(task, obs.data_ptr(), reward.data_ptr(), flags.data_ptr(), head.data_ptr(), self._stream())

    def task_push_outputs(self, task, obs: torch.Tensor, reward: torch.Tensor, flags: torch.Tensor):
        self._sim.task_push_outputs(task, obs.data_ptr(), reward.data_ptr(), flags.data_ptr(), self._stream())

    def task_stack_outputs(self, task, obs: torch.Tensor, reward: torch.Tensor, flags: torch.Tensor):
        """StackCube evaluate / obs / reward in one launch (include/mssim_hip_tasks.h; HIP library only)"""
        self._sim.task_stack_outputs(task, obs.data_ptr(), reward.data_ptr(), flags.data_ptr(), self._stream())

    def task_pusht_outputs(self, task, obs: torch.Tensor, reward: torch.Tensor, flags: torch.Tensor, intersection: torch.Tensor = None):
        """PushT evaluate / obs / reward in one launch; `intersection` [N] f32 (optional): template pixels hit
        (include/mssim_hip_tasks.h; HIP library only)"""
        self._sim.task_pusht_outputs(task, obs.data_ptr(), reward.data_ptr(), flags.data_ptr(),
                                     None if intersection is None else intersection.data_ptr(), self._stream())

    def task_roll_outputs(self, task, obs: torch.Tensor, reward: torch.Tensor, flags: torch.Tensor):
        """RollBall evaluate / obs / reward in one launch; the struct points to the env's `reached_status` latch
        (include/mssim_hip_tasks.h; HIP library only)"""
        self._sim.task_roll_outputs(task, obs.data_ptr(), reward.data_ptr(), flags.data_ptr(), self._stream())

    def task_pull_outputs(self, task, obs: torch.Tensor, reward: torch.Tensor, flags: torch.Tensor):
        """PullCube evaluate / obs / reward in one launch (include/mssim_hip_tasks.h; HIP library only)"""
        self._sim.task_pull_outputs(task, obs.data_ptr(), reward.data_ptr(), flags.data_ptr(), self._stream())

    def task_poke_outputs(self, task, obs: torch.Tensor, reward: torch.Tensor, flags: torch.Tensor, metrics: Optional[torch.Tensor]):
        """PokeCube evaluate / obs / reward in one launch; metrics [N][2] f32 = angle_diff, head_to_cube_dist, required
        (include/mssim_hip_tasks.h; HIP library only)"""
        self._sim.task_poke_outputs(task, obs.data_ptr(), reward.data_ptr(), flags.data_ptr(), None if metrics is None else metrics.data_ptr(), self._stream())

    def task_liftpeg_outputs(self, task, obs: torch.Tensor, reward: torch.Tensor, flags: torch.Tensor):
        """LiftPegUpright evaluate / obs / reward in one launch (include/mssim_hip_tasks.h; HIP library only)"""
        self._sim.task_liftpeg_outputs(task, obs.data_ptr(), reward.data_ptr(), flags.data_ptr(), self._stream())

    def task_place_outputs(self, task, obs: torch.Tensor, reward: torch.Tensor, flags: torch.Tensor):
        """PlaceSphere evaluate / obs / reward in one launch (include/mssim_hip_tasks.h; HIP library only)"""
        self._sim.task_place_outputs(task, obs.data_ptr(), reward.data_ptr(), flags.data_ptr(), self._stream())

    def task_pulltool_outputs(self, task, obs: torch.Tensor, reward: torch.Tensor, flags: torch.Tensor, metrics: Optional[torch.Tensor]):
        """PullCubeTool evaluate / obs / reward in one launch; metrics [N][3] f32 = cube_to_workspace_dist, its progress
        term, dense reward / 5, required (include/mssim_hip_tasks.h; HIP library only)"""
        self._sim.task_pulltool_outputs(task, obs.data_ptr(), reward.data_ptr(), flags.data_ptr(), None if metrics is None else metrics.data_ptr(), self._stream())

    def task_plug_outputs(self, task, obs: torch.Tensor, reward: torch.Tensor, flags: torch.Tensor, metrics: Optional[torch.Tensor]):
        """PlugCharger evaluate / obs / reward in one launch; metrics [N][2] f32 = obj_to_goal_dist, obj_to_goal_angle,
        required; `task.goal_pose` points at the env's stored goal tensor (include/mssim_hip_tasks.h; HIP library only)"""
        self._sim.task_plug_outputs(task, obs.data_ptr(), reward.data_ptr(), flags.data_ptr(), None if metrics is None else metrics.data_ptr(), self._stream())

    def task_draw_outputs(self, task, obs: torch.Tensor, reward: torch.Tensor, flags: torch.Tensor):
        """DrawTriangle dot layer / evaluate / obs in one launch; the struct points at the env's dot tables, which the
        launch updates in place where `task.update` is set (include/mssim_hip_tasks.h; HIP library only)"""
        self._sim.task_draw_outputs(task, obs.data_ptr(), reward.data_ptr(), flags.data_ptr(), self._stream())

    # ------------------------------------------------------------------ ray-cast cameras (HIP only)
    def raycast_create(self, scene_arrays: dict, cameras: Sequence[dict]) -> int:
        """a ray-cast scene (`model.compile.raycast_scene`) with its cameras -> id for `raycast_render`
        (include/mssim_hip_tasks.h `mssim_raycast_create`). A camera is a dict: width, height, fx, fy, cx, cy, near, far,
        mount_row (-1: the env frame), pose (7 floats) or env_pose (a contiguous f32 [N, 7] tensor on the system's
        device, read at every render; kept alive here)."""
        descs, keep = [], []
        for c in cameras:
            d = native.CameraDesc(int(c["width"]), int(c["height"]), float(c["fx"]), float(c["fy"]), float(c["cx"]), float(c["cy"]),
                                  float(c["near"]), float(c["far"]), int(c.get("mount_row", -1)))
            pose = c.get("env_pose")
            if pose is not None:
                assert pose.dtype == torch.float32 and pose.is_contiguous() and tuple(pose.shape) == (self.num_envs, 7) and pose.device == self._rigid.device
                keep.append(pose)
                d.env_pose = pose.data_ptr()
                d.pose = (native.C.c_float * 7)(0, 0, 0, 1, 0, 0, 0)
            else:
                d.pose = (native.C.c_float * 7)(*[float(x) for x in np.asarray(c["pose"], dtype=np.float64).reshape(7)])
            descs.append(d)
        rid = self._sim.raycast_create(scene_arrays, descs)
        self._raycast_keep[rid] = (keep, [(int(c["width"]), int(c["height"])) for c in cameras])
        return rid

    def raycast_render(self, rid: int, camera: int, pos_seg: torch.Tensor, depth: Optional[torch.Tensor] = None):
        """one launch on the current stream: `pos_seg` int16 [N, H, W, 4] (x, y, z in mm in the camera's OpenGL frame,
        segmentation id), `depth` optional f32 [N, H, W] z-depth in metres; zeros where nothing is hit"""
        sizes = self._raycast_sizes(rid)
        if not 0 <= camera < len(sizes):
            raise native.NativeError(f"raycast_render: scene {rid} has no camera {camera} (it has {len(sizes)})")
        w, h = sizes[camera]
        assert pos_seg.dtype == torch.int16 and pos_seg.is_contiguous() and tuple(pos_seg.shape) == (self.num_envs, h, w, 4)
        assert depth is None or (depth.dtype == torch.float32 and depth.is_contiguous() and tuple(depth.shape) == (self.num_envs, h, w))
        self._sim.raycast_render(rid, camera, pos_seg.data_ptr(), None if depth is None else depth.data_ptr(), self._stream())

    def raycast_set_colours(self, rid: int, shape_rgba: np.ndarray, env_shape_rgba: Optional[np.ndarray] = None):
        """the colours of a ray-cast scene's shapes for `raycast_shade` (`model.compile.raycast_colours`): host arrays
        shape_rgba f32 [n_shape, 4] -- r, g, b in [0, 1] and a checker cell size in metres, 0 for none -- and optionally
        env_shape_rgba f32 [n_env_shape, N, 4], a colour per env for the shapes in per-env slots"""
        self._raycast_sizes(rid)
        if env_shape_rgba is not None:
            env_shape_rgba = np.asarray(env_shape_rgba, dtype=np.float32)
            if env_shape_rgba.ndim != 3 or env_shape_rgba.shape[1:] != (self.num_envs, 4):
                raise native.NativeError(f"raycast_set_colours: env_shape_rgba must be [slots, {self.num_envs}, 4], got {tuple(env_shape_rgba.shape)}")
        self._sim.raycast_set_colours(rid, shape_rgba, env_shape_rgba)

    def raycast_shade(self, rid: int, camera: int, rgba: torch.Tensor):
        """one launch on the current stream: the flat-shaded view of camera `camera` into `rgba` uint8 [N, H, W, 4]
        (r, g, b, 255; the background colour where nothing is hit). Colours come first (`raycast_set_colours`)."""
        sizes = self._raycast_sizes(rid)
        if not 0 <= camera < len(sizes):
            raise native.NativeError(f"raycast_shade: scene {rid} has no camera {camera} (it has {len(sizes)})")
        w, h = sizes[camera]
        assert rgba.dtype == torch.uint8 and rgba.is_contiguous() and tuple(rgba.shape) == (self.num_envs, h, w, 4)
        self._sim.raycast_shade(rid, camera, rgba.data_ptr(), self._stream())

    def raycast_draw_dots(self, rid: int, camera: int, layer, depth: torch.Tensor, rgba: torch.Tensor):
        """one launch on the current stream: the discs of a dot layer (`native.DotLayer`: an env's table of drawn dots)
        painted over the shaded view `rgba` uint8 [N, H, W, 4] of `raycast_shade`, hidden where `depth` f32 [N, H, W] of
        `raycast_render` for the same camera and state has something nearer"""
        sizes = self._raycast_sizes(rid)
        if not 0 <= camera < len(sizes):
            raise native.NativeError(f"raycast_draw_dots: scene {rid} has no camera {camera} (it has {len(sizes)})")
        w, h = sizes[camera]
        assert rgba.dtype == torch.uint8 and rgba.is_contiguous() and tuple(rgba.shape) == (self.num_envs, h, w, 4)
        assert depth.dtype == torch.float32 and depth.is_contiguous() and tuple(depth.shape) == (self.num_envs, h, w)
        self._sim.raycast_draw_dots(rid, camera, layer, depth.data_ptr(), rgba.data_ptr(), self._stream())

    def raycast_destroy(self, rid: int):
        self._raycast_sizes(rid)
        self._sim.raycast_destroy(rid)
        del self._raycast_keep[rid]

    def _raycast_sizes(self, rid: int):
        if rid not in self._raycast_keep:
            raise native.NativeError(f"no ray-cast scene with id {rid} on this system (raycast_create returns the ids; a destroyed one is gone)")
        return self._raycast_keep[rid][1]

    def tail_step_count(self) -> int:
        """control steps so far that ran as one launch with the task epilogue at the kernel's tail (HIP library only)"""
        return self._sim.tail_step_count()

    def task_pick_outputs(self, task, obs: torch.Tensor, reward: torch.Tensor, flags: torch.Tensor):
        self._sim.task_pick_outputs(task, obs.data_ptr(), reward.data_ptr(), flags.data_ptr(), self._stream())

    def profile_enable(self, on: bool = True):
        """bracket the solve / narrowphase launches with HIP events on their launch stream"""
        self._sim.profile_enable(on)

    def profile_read(self):
        return self._sim.profile_read()

    def overflow_count(self) -> int:
        return self._sim.overflow_count(self._stream())

    # row helpers --------------------------------------------------------------
    def body_rows(self, body_row: int) -> slice:
        """rows of `cuda_rigid_body_data` holding body `body_row` for envs 0..N-1"""
        return slice(body_row * self.num_envs, (body_row + 1) * self.num_envs)

    # sub-scene bookkeeping of the reference (sapien_env.py:1080-1096) -----------------------------------
    def set_scene_offset(self, scene, offset):
        """The reference isolates its envs by spacing them out in ONE PhysX scene. Here every env has its own
        frame, bodies of different envs can never meet, so the offset is recorded for `get_scene_offset` and
        otherwise unused."""
        self.__dict__.setdefault("_scene_offsets", {})[id(scene)] = np.asarray(offset, dtype=np.float32).reshape(3)

    def get_scene_offset(self, scene) -> np.ndarray:
        return self.__dict__.get("_scene_offsets", {}).get(id(scene), np.zeros(3, dtype=np.float32))

    # introspection: the builder-time component objects, filled in by ManiSkillScene._setup; below the env
    # layer (no builders) the lists are made from the compiled model's body names
    def _component_lists(self):
        comps = getattr(self, "_components", None)
        if comps is None and self.model is not None:
            from . import PhysxArticulationLinkComponent, PhysxRigidDynamicComponent, PhysxRigidStaticComponent

            comps = dict(dynamic=[], static=[], links=[])
            for i, name in enumerate(self.model.link_names):
                c = PhysxArticulationLinkComponent()
                c.name, c.index, c.gpu_pose_index = name, i, i * self.num_envs
                comps["links"].append(c)
            for k, name in enumerate(list(self.model.free_names) + list(self.model.kin_names)):
                c = PhysxRigidDynamicComponent()
                c.name, c.kinematic = name, k >= self.model.n_free
                c.gpu_pose_index, c.gpu_index = (self.model.n_link + k) * self.num_envs, k * self.num_envs
                comps["dynamic"].append(c)
            for name in self.model.static_names:
                c = PhysxRigidStaticComponent()
                c.name = name
                comps["static"].append(c)
            self._components = comps
        return comps or dict(dynamic=[], static=[], links=[])

    @property
    def rigid_dynamic_components(self):
        """dynamic and kinematic bodies, in `cuda_rigid_body_data` row order"""
        return list(self._component_lists()["dynamic"])

    @property
    def rigid_static_components(self):
        return list(self._component_lists()["static"])

    @property
    def articulation_link_components(self):
        return list(self._component_lists()["links"])

    def get_contacts(self, env_index: int = 0):
        """body pairs of env `env_index` with a contact in the last substep -> [PhysxContact] (the reference's CPU-only
        `px.get_contacts()`, utils/sapien_utils.py:215-260). One aggregate point per shape pair: impulse on bodies[0]
        (the core exports per-pair impulses, include/mssim.h). Synchronises."""
        from . import PhysxContact, PhysxContactPoint

        m = self.model
        cnt = self.read_internal("contact_count", max(m.n_pair, 1))[:, env_index].cpu().numpy()
        imp = self.read_internal("pair_impulse", max(3 * m.n_pair, 1))[:, env_index].cpu().numpy().reshape(-1, 3)
        lists = self._component_lists()
        by_row = {}
        for c in lists["links"] + lists["dynamic"]:
            by_row[c.gpu_pose_index // max(self.num_envs, 1)] = c
        # (a static body has no row: it is found by the name of its shape's owner)
        statics = {c.name: c for c in lists["static"]}
        world = lists["static"][0] if lists["static"] else None
        out = []
        pair_shape, shape_row = m.arrays["pair_shape"], m.arrays["shape_row"]

        def body_of(shape):
            row = int(shape_row[shape])
            return by_row[row] if row in by_row else statics.get(m.shape_owner[shape], world)

        for p in range(m.n_pair):
            if cnt[p] <= 0:
                continue
            out.append(PhysxContact(body_of(int(pair_shape[p][0])), body_of(int(pair_shape[p][1])), [PhysxContactPoint(impulse=imp[p].copy())]))
        return out

    def sync_poses_gpu_to_cpu(self):
        """viewer hook of the reference (copies poses into the CPU entities for rendering); there are no CPU
        entities here, the buffers read through `cuda_rigid_body_data` are the state"""
        self.gpu_fetch_all()
