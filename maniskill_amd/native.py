"""ctypes binding of the C ABI in include/mssim.h.

`NativeLib(path, prefix)` binds any library that exports the ABI under a symbol prefix. The
product library is `maniskill_amd/_native/libmssim.so` (prefix `mssim_`, HIP/gfx950); loading it
fails loudly if it has not been built -- there is no CPU fallback in this package.
"""
import ctypes as C
import os
from typing import Dict, Optional

import numpy as np

from . import PACKAGE_DIR
from .model.compile import CompiledModel

ABI_VERSION = 6
NATIVE_LIB_PATH = os.environ.get("MSSIM_LIB") or os.path.join(PACKAGE_DIR, "_native", "libmssim.so")  # MSSIM_LIB: debug builds of the same HIP library

# apply / fetch selector bits (include/mssim.h)
RIGID_DATA = 1 << 0
ART_QPOS = 1 << 1
ART_QVEL = 1 << 2
ART_QF = 1 << 3
ART_ROOT_POSE = 1 << 4
ART_ROOT_VEL = 1 << 5
ART_TARGET_POS = 1 << 6
ART_TARGET_VEL = 1 << 7
RIGID_FORCE = 1 << 8
LINK_POSE = 1 << 9
LINK_VEL = 1 << 10
ART_QACC = 1 << 11
ALL = 0xFFF

_I32P = C.POINTER(C.c_int32)
_F32P = C.POINTER(C.c_float)


class ModelDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("n_dof", C.c_int32),
        ("dof_parent", _I32P),
        ("dof_type", _I32P),
        ("dof_frame", _F32P),
        ("dof_axis", _F32P),
        ("dof_limit", _F32P),
        ("dof_drive", _F32P),
        ("dof_armature", _F32P),
        ("body_inertial", _F32P),
        ("body_gravity", _I32P),
        ("n_tendon", C.c_int32),
        ("tendon_dof", _I32P),
        ("tendon_param", _F32P),
        ("n_link", C.c_int32),
        ("link_body", _I32P),
        ("link_frame", _F32P),
        ("n_free", C.c_int32),
        ("free_inertial", _F32P),
        ("free_damping", _F32P),
        ("free_gravity", _I32P),
        ("n_kin", C.c_int32),
        ("n_shape", C.c_int32),
        ("shape_type", _I32P),
        ("shape_body_kind", _I32P),
        ("shape_body_index", _I32P),
        ("shape_row", _I32P),
        ("shape_frame", _F32P),
        ("shape_param", _F32P),
        ("shape_material", _F32P),
        ("shape_hull", _I32P),
        ("shape_bound", _F32P),
        ("n_hull_verts", C.c_int32),
        ("hull_verts", _F32P),
        ("n_pair", C.c_int32),
        ("pair_shape", _I32P),
        ("gravity", C.c_float * 3),
        ("timestep", C.c_float),
        ("contact_offset", C.c_float),
        ("rest_offset", C.c_float),
        ("bounce_threshold", C.c_float),
        ("position_iterations", C.c_int32),
        ("velocity_iterations", C.c_int32),
        ("erp", C.c_float),
        ("max_depenetration_velocity", C.c_float),
        ("sleep_threshold", C.c_float),
        ("num_envs", C.c_int32),
        ("n_env_shape", C.c_int32),
        ("shape_env_slot", _I32P),
        ("env_shape_frame", _F32P),
        ("env_shape_param", _F32P),
        ("env_shape_bound", _F32P),
        ("n_env_free", C.c_int32),
        ("free_env_slot", _I32P),
        ("env_free_inertial", _F32P),
        ("n_tri", C.c_int32),
        ("tri_soup", _F32P),
        ("n_tri_node", C.c_int32),
        ("tri_bvh", _F32P),
    ]


class Buffers(C.Structure):
    _fields_ = [
        ("rigid_body_data", C.c_void_p),
        ("rigid_body_force", C.c_void_p),
        ("art_qpos", C.c_void_p),
        ("art_qvel", C.c_void_p),
        ("art_qacc", C.c_void_p),
        ("art_qf", C.c_void_p),
        ("art_target_qpos", C.c_void_p),
        ("art_target_qvel", C.c_void_p),
    ]


def make_model_desc(model: CompiledModel):
    """Returns (ModelDesc, keepalive) -- keepalive must outlive the create call."""
    d = ModelDesc()
    keep = []
    d.abi_version = ABI_VERSION
    for name, ctype in ModelDesc._fields_:
        if ctype in (_I32P, _F32P):
            a = model.arrays[name]
            want = np.int32 if ctype is _I32P else np.float32
            a = np.ascontiguousarray(a, dtype=want)
            keep.append(a)
            setattr(d, name, a.ctypes.data_as(ctype))
        elif name == "gravity":
            d.gravity = (C.c_float * 3)(*model.scalars["gravity"])
        elif name != "abi_version":
            setattr(d, name, model.scalars[name])
    return d, keep


class PickTask(C.Structure):
    _fields_ = [
        ("tcp_row", C.c_int32), ("obj_row", C.c_int32), ("goal_row", C.c_int32), ("finger1_row", C.c_int32), ("finger2_row", C.c_int32),
        ("n_static_dofs", C.c_int32), ("goal_thresh", C.c_float), ("static_thresh", C.c_float), ("min_force", C.c_float),
        ("max_angle_deg", C.c_float), ("reward_scale", C.c_float), ("elapsed_steps", C.c_void_p), ("elapsed_out", C.c_void_p), ("truncated_out", C.c_void_p), ("time_limit", C.c_int32), ("terminated_out", C.c_void_p),
    ]


class PushTask(C.Structure):
    _fields_ = [("tcp_row", C.c_int32), ("obj_row", C.c_int32), ("goal_row", C.c_int32), ("goal_radius", C.c_float),
                ("cube_half_size", C.c_float), ("reward_scale", C.c_float), ("elapsed_steps", C.c_void_p), ("elapsed_out", C.c_void_p), ("truncated_out", C.c_void_p), ("time_limit", C.c_int32), ("terminated_out", C.c_void_p)]


class PegTask(C.Structure):
    _fields_ = [("tcp_row", C.c_int32), ("peg_row", C.c_int32), ("box_row", C.c_int32), ("finger1_row", C.c_int32), ("finger2_row", C.c_int32),
                ("min_force", C.c_float), ("max_angle_deg", C.c_float), ("reward_scale", C.c_float),
                ("peg_half_sizes", C.c_void_p), ("box_hole_offsets", C.c_void_p), ("box_hole_radii", C.c_void_p),
                ("elapsed_steps", C.c_void_p), ("elapsed_out", C.c_void_p), ("truncated_out", C.c_void_p), ("time_limit", C.c_int32), ("terminated_out", C.c_void_p)]


class StackTask(C.Structure):
    """mssim_stack_task of include/mssim_hip_tasks.h (HIP library only)"""
    _fields_ = [("tcp_row", C.c_int32), ("cubeA_row", C.c_int32), ("cubeB_row", C.c_int32), ("finger1_row", C.c_int32), ("finger2_row", C.c_int32),
                ("cube_half_size", C.c_float), ("on_xy_thresh", C.c_float), ("on_z_thresh", C.c_float), ("gripper_width", C.c_float),
                ("static_lin_thresh", C.c_float), ("static_ang_thresh", C.c_float), ("min_force", C.c_float), ("max_angle_deg", C.c_float),
                ("reward_scale", C.c_float),
                ("elapsed_steps", C.c_void_p), ("elapsed_out", C.c_void_p), ("truncated_out", C.c_void_p), ("time_limit", C.c_int32), ("terminated_out", C.c_void_p)]


class PushTTask(C.Structure):
    """mssim_pusht_task of include/mssim_hip_tasks.h (HIP library only)"""
    _fields_ = [("tcp_row", C.c_int32), ("tee_row", C.c_int32), ("goal_row", C.c_int32),
                ("goal_z_rot", C.c_float), ("intersection_thresh", C.c_float), ("reward_div", C.c_float), ("consts", C.c_void_p),
                ("elapsed_steps", C.c_void_p), ("elapsed_out", C.c_void_p), ("truncated_out", C.c_void_p), ("time_limit", C.c_int32), ("terminated_out", C.c_void_p)]


class RollTask(C.Structure):
    """mssim_roll_task of include/mssim_hip_tasks.h (HIP library only)"""
    _fields_ = [("tcp_row", C.c_int32), ("ball_row", C.c_int32), ("goal_row", C.c_int32),
                ("goal_radius", C.c_float), ("ball_radius", C.c_float), ("hit_offset", C.c_float), ("reach_thresh", C.c_float),
                ("reward_scale", C.c_float), ("reached", C.c_void_p), ("update_reached", C.c_int32),
                ("elapsed_steps", C.c_void_p), ("elapsed_out", C.c_void_p), ("truncated_out", C.c_void_p), ("time_limit", C.c_int32), ("terminated_out", C.c_void_p)]


class PullTask(C.Structure):
    """mssim_pull_task of include/mssim_hip_tasks.h (HIP library only)"""
    _fields_ = [("tcp_row", C.c_int32), ("obj_row", C.c_int32), ("goal_row", C.c_int32), ("goal_radius", C.c_float),
                ("cube_half_size", C.c_float), ("reward_scale", C.c_float),
                ("elapsed_steps", C.c_void_p), ("elapsed_out", C.c_void_p), ("truncated_out", C.c_void_p), ("time_limit", C.c_int32), ("terminated_out", C.c_void_p)]


class PokeTask(C.Structure):
    """mssim_poke_task of include/mssim_hip_tasks.h (HIP library only)"""
    _fields_ = [("tcp_row", C.c_int32), ("peg_row", C.c_int32), ("cube_row", C.c_int32), ("goal_row", C.c_int32), ("finger1_row", C.c_int32), ("finger2_row", C.c_int32),
                ("n_static_dofs", C.c_int32), ("peg_half_length", C.c_float), ("cube_half_size", C.c_float), ("goal_radius", C.c_float), ("align_thresh", C.c_float),
                ("reach_thresh", C.c_float), ("static_thresh", C.c_float), ("min_force", C.c_float), ("max_angle_deg", C.c_float), ("reward_scale", C.c_float),
                ("elapsed_steps", C.c_void_p), ("elapsed_out", C.c_void_p), ("truncated_out", C.c_void_p), ("time_limit", C.c_int32), ("terminated_out", C.c_void_p)]


class LiftPegTask(C.Structure):
    """mssim_liftpeg_task of include/mssim_hip_tasks.h (HIP library only)"""
    _fields_ = [("tcp_row", C.c_int32), ("peg_row", C.c_int32), ("finger1_row", C.c_int32), ("finger2_row", C.c_int32),
                ("peg_half_length", C.c_float), ("upright_thresh", C.c_float), ("height_thresh", C.c_float), ("min_force", C.c_float), ("max_angle_deg", C.c_float),
                ("reward_scale", C.c_float),
                ("elapsed_steps", C.c_void_p), ("elapsed_out", C.c_void_p), ("truncated_out", C.c_void_p), ("time_limit", C.c_int32), ("terminated_out", C.c_void_p)]


class PlaceTask(C.Structure):
    """mssim_place_task of include/mssim_hip_tasks.h (HIP library only)"""
    _fields_ = [("tcp_row", C.c_int32), ("obj_row", C.c_int32), ("bin_row", C.c_int32), ("finger1_row", C.c_int32), ("finger2_row", C.c_int32),
                ("n_static_dofs", C.c_int32), ("radius", C.c_float), ("bin_base_half", C.c_float), ("on_bin_tol", C.c_float), ("static_lin_thresh", C.c_float),
                ("static_ang_thresh", C.c_float), ("robot_static_thresh", C.c_float), ("gripper_width", C.c_float), ("min_force", C.c_float),
                ("max_angle_deg", C.c_float), ("reward_scale", C.c_float),
                ("elapsed_steps", C.c_void_p), ("elapsed_out", C.c_void_p), ("truncated_out", C.c_void_p), ("time_limit", C.c_int32), ("terminated_out", C.c_void_p)]


class PullToolTask(C.Structure):
    """mssim_pulltool_task of include/mssim_hip_tasks.h (HIP library only)"""
    _fields_ = [("tcp_row", C.c_int32), ("cube_row", C.c_int32), ("tool_row", C.c_int32), ("base_row", C.c_int32), ("finger1_row", C.c_int32), ("finger2_row", C.c_int32),
                ("cube_half_size", C.c_float), ("hook_length", C.c_float), ("arm_reach", C.c_float), ("cube_size", C.c_float), ("pulled_close_dist", C.c_float),
                ("min_force", C.c_float), ("max_angle_deg", C.c_float), ("reward_scale", C.c_float),
                ("elapsed_steps", C.c_void_p), ("elapsed_out", C.c_void_p), ("truncated_out", C.c_void_p), ("time_limit", C.c_int32), ("terminated_out", C.c_void_p)]


class PlugTask(C.Structure):
    """mssim_plug_task of include/mssim_hip_tasks.h (HIP library only)"""
    _fields_ = [("tcp_row", C.c_int32), ("charger_row", C.c_int32), ("receptacle_row", C.c_int32), ("goal_pose", C.c_void_p),
                ("dist_thresh", C.c_float), ("angle_thresh", C.c_float), ("reward_scale", C.c_float),
                ("elapsed_steps", C.c_void_p), ("elapsed_out", C.c_void_p), ("truncated_out", C.c_void_p), ("time_limit", C.c_int32), ("terminated_out", C.c_void_p)]


class DrawTask(C.Structure):
    """mssim_draw_task of include/mssim_hip_tasks.h (HIP library only)"""
    _fields_ = [("tcp_row", C.c_int32), ("goal_row", C.c_int32), ("vertices", C.c_void_p), ("triangles", C.c_void_p), ("dots", C.c_void_p),
                ("dot_near", C.c_void_p), ("ref_hit", C.c_void_p), ("draw_step", C.c_void_p), ("max_dots", C.c_int32), ("n_ref", C.c_int32),
                ("z_thresh", C.c_float), ("near_thresh2", C.c_float), ("update", C.c_int32), ("reward_scale", C.c_float),
                ("elapsed_steps", C.c_void_p), ("elapsed_out", C.c_void_p), ("truncated_out", C.c_void_p), ("time_limit", C.c_int32), ("terminated_out", C.c_void_p)]


class DotLayer(C.Structure):
    """mssim_dot_layer of include/mssim_hip_tasks.h (HIP library only)"""
    _fields_ = [("dots", C.c_void_p), ("dot_near", C.c_void_p), ("count", C.c_void_p), ("max_dots", C.c_int32), ("z", C.c_float), ("radius", C.c_float),
                ("rgba", C.c_uint32)]


class TaskRobot(C.Structure):
    """mssim_task_robot of include/mssim_hip_tasks.h (HIP library only): the robot-dependent rules of the task epilogues"""
    _fields_ = [("n_ranges", C.c_int32), ("first", C.c_int32 * 2), ("count", C.c_int32 * 2), ("thresh", C.c_float * 2),
                ("signed_compare", C.c_int32), ("pick_norm_dofs", C.c_int32)]


class EeIkMap(C.Structure):
    """mssim_ee_ik_map of include/mssim_hip_tasks.h (HIP library only)"""
    _fields_ = [("link_index", C.c_int32), ("column0", C.c_int32), ("rows", C.c_int32), ("mode", C.c_int32),
                ("low", C.c_float), ("high", C.c_float), ("rot_scale", C.c_float), ("flags", C.c_int32),
                ("max_iters", C.c_int32), ("damping", C.c_float), ("max_step", C.c_float), ("tolerance", C.c_float)]


_I16P = C.POINTER(C.c_int16)


class RaycastScene(C.Structure):
    """mssim_raycast_scene of include/mssim_hip_tasks.h (HIP library only): host arrays, read once by raycast_create"""
    _fields_ = [("n_shape", C.c_int32), ("shape_type", _I32P), ("shape_row", _I32P), ("shape_frame", _F32P), ("shape_param", _F32P),
                ("shape_bound", _F32P), ("shape_seg", _I16P), ("shape_planes", _I32P), ("n_plane", C.c_int32), ("planes", _F32P),
                ("n_env_shape", C.c_int32), ("shape_env_slot", _I32P), ("env_shape_frame", _F32P), ("env_shape_param", _F32P),
                ("env_shape_bound", _F32P),
                ("n_tri", C.c_int32), ("tri_soup", _F32P), ("n_tri_node", C.c_int32), ("tri_bvh", _F32P), ("env_shape_planes", _I32P),
                ("env_shape_seg", _I16P)]


# members of the scene a caller may leave out (NULL / 0: no meshes, the shared plane range and id in every env)
_RAYCAST_OPTIONAL = ("tri_soup", "tri_bvh", "env_shape_planes", "env_shape_seg")


class CameraDesc(C.Structure):
    """mssim_camera_desc of include/mssim_hip_tasks.h (HIP library only)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("near", C.c_float), ("far", C.c_float), ("mount_row", C.c_int32), ("pose", C.c_float * 7), ("env_pose", C.c_void_p)]


def make_raycast_scene(arrays: dict):
    """Returns (RaycastScene, keepalive) from the arrays of `model.compile.raycast_scene` (or hand-made ones with the
    same keys); keepalive must outlive the create call."""
    d, keep = RaycastScene(), []
    d.n_shape, d.n_plane, d.n_env_shape = len(arrays["shape_type"]), len(arrays["planes"]), int(arrays.get("n_env_shape", 0))
    d.n_tri = len(arrays["tri_soup"]) if arrays.get("tri_soup") is not None else 0
    d.n_tri_node = len(arrays["tri_bvh"]) if arrays.get("tri_bvh") is not None else 0
    for name, ctype in RaycastScene._fields_:
        if name in _RAYCAST_OPTIONAL and arrays.get(name) is None:
            continue
        if ctype in (_I32P, _F32P, _I16P):
            a = np.ascontiguousarray(arrays[name], dtype={_I32P: np.int32, _F32P: np.float32, _I16P: np.int16}[ctype])
            keep.append(a)
            setattr(d, name, a.ctypes.data_as(ctype))
    return d, keep


class NativeError(RuntimeError):
    pass


class NativeLib:
    """One loaded library exporting the mssim ABI under `prefix`."""

    _cache: Dict[tuple, "NativeLib"] = {}

    def __init__(self, path: str, prefix: str = "mssim_"):
        if not os.path.exists(path):
            raise NativeError(
                f"native simulation library not found: {path}. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
                "There is no CPU fallback."
            )
        self.path, self.prefix = path, prefix
        self.lib = C.CDLL(path)
        f = self._fn
        H = C.c_void_p
        f("create", C.c_int, [C.POINTER(ModelDesc), C.c_int32, C.c_int32, C.POINTER(H)])
        f("destroy", None, [H])
        f("bind_buffers", C.c_int, [H, C.POINTER(Buffers)])
        f("set_timestep", C.c_int, [H, C.c_float])
        f("get_timestep", C.c_float, [H])
        f("apply", C.c_int, [H, C.c_uint32, C.c_void_p])
        f("fetch", C.c_int, [H, C.c_uint32, C.c_void_p])
        f("step", C.c_int, [H, C.c_int32, C.c_void_p])
        f("update_kinematics", C.c_int, [H, C.c_void_p])
        f("wake_all", C.c_int, [H, C.c_void_p])
        f("wake_envs", C.c_int, [H, C.c_void_p, C.c_int32, C.c_void_p])
        f("create_pair_query", C.c_int, [H, _I32P, C.c_int32, _I32P])
        f("query_pair_impulses", C.c_int, [H, C.c_int32, C.c_void_p, C.c_void_p])
        f("create_body_query", C.c_int, [H, _I32P, C.c_int32, _I32P])
        f("query_body_impulses", C.c_int, [H, C.c_int32, C.c_void_p, C.c_void_p])
        f("set_drive_properties", C.c_int, [H, _F32P])
        f("read_internal", C.c_int, [H, C.c_char_p, C.c_void_p, C.c_int32, C.c_void_p])
        f("link_jacobian", C.c_int, [H, C.c_int32, C.c_void_p, C.c_void_p])
        f("overflow_count", C.c_int, [H, C.c_void_p])
        f("set_action_map", C.c_int, [H, _I32P, _F32P, _F32P, _I32P])
        f("set_ee_action_map", C.c_int, [H, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_int32])
        f("apply_action", C.c_int, [H, C.c_void_p, C.c_int32, C.c_void_p])
        f("step_action", C.c_int, [H, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p])
        f("defer_fetch", C.c_int, [H, C.c_uint32])
        f("defer_step_action", C.c_int, [H, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p])
        f("task_pick_outputs", C.c_int, [H, C.POINTER(PickTask), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
        f("task_peg_outputs", C.c_int, [H, C.POINTER(PegTask), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
        f("task_push_outputs", C.c_int, [H, C.POINTER(PushTask), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
        f("profile_enable", C.c_int, [H, C.c_int32])
        f("profile_read", C.c_int, [H, _F32P, _I32P])
        f("last_error", C.c_char_p, [H])
        f("abi_version", C.c_int, [])
        if self.abi_version() != ABI_VERSION:
            raise NativeError(f"{path}: ABI version {self.abi_version()} != {ABI_VERSION}")
        # extras of the HIP library alone (include/mssim_hip_tasks.h), outside the ABI that the oracle shares: bound
        # when present, None otherwise
        H = C.c_void_p
        for name, restype, argtypes in (
            ("task_stack_outputs", C.c_int, [H, C.POINTER(StackTask), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
            ("task_pusht_outputs", C.c_int, [H, C.POINTER(PushTTask), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
            ("task_roll_outputs", C.c_int, [H, C.POINTER(RollTask), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
            ("task_pull_outputs", C.c_int, [H, C.POINTER(PullTask), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
            ("task_poke_outputs", C.c_int, [H, C.POINTER(PokeTask), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
            ("task_liftpeg_outputs", C.c_int, [H, C.POINTER(LiftPegTask), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
            ("task_place_outputs", C.c_int, [H, C.POINTER(PlaceTask), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
            ("task_pulltool_outputs", C.c_int, [H, C.POINTER(PullToolTask), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
            ("task_plug_outputs", C.c_int, [H, C.POINTER(PlugTask), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
            ("task_draw_outputs", C.c_int, [H, C.POINTER(DrawTask), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
            ("raycast_draw_dots", C.c_int, [H, C.c_int32, C.c_int32, C.POINTER(DotLayer), C.c_void_p, C.c_void_p, C.c_void_p]),
            ("tail_step_count", C.c_int64, [H]),
            ("set_task_robot", C.c_int, [H, C.POINTER(TaskRobot)]),
            ("set_ee_ik_map", C.c_int, [H, C.POINTER(EeIkMap), C.c_void_p]),
            ("ee_ik_solve", C.c_int, [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
            ("raycast_create", C.c_int, [H, C.POINTER(RaycastScene), C.POINTER(CameraDesc), C.c_int32, _I32P]),
            ("raycast_destroy", C.c_int, [H, C.c_int32]),
            ("raycast_render", C.c_int, [H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
            ("raycast_set_colours", C.c_int, [H, C.c_int32, _F32P, _F32P]),
            ("raycast_shade", C.c_int, [H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
        ):
            if hasattr(self.lib, self.prefix + name):
                self._fn(name, restype, argtypes)
            else:
                setattr(self, name, None)

    EXPORTS = [
        "create", "destroy", "bind_buffers", "set_timestep", "get_timestep", "apply", "fetch", "step",
        "update_kinematics", "wake_all", "wake_envs", "create_pair_query", "query_pair_impulses", "create_body_query",
        "query_body_impulses", "set_drive_properties", "read_internal", "link_jacobian", "overflow_count", "set_action_map", "set_ee_action_map",
        "apply_action", "step_action", "defer_fetch", "defer_step_action", "task_pick_outputs", "task_push_outputs", "task_peg_outputs", "profile_enable",
        "profile_read", "last_error",
        "abi_version",
    ]

    def _fn(self, name, restype, argtypes):
        fn = getattr(self.lib, self.prefix + name)
        fn.restype, fn.argtypes = restype, argtypes
        setattr(self, name, fn)

    @classmethod
    def load(cls, path: Optional[str] = None, prefix: str = "mssim_") -> "NativeLib":
        path = path or NATIVE_LIB_PATH
        key = (os.path.abspath(path), prefix)
        if key not in cls._cache:
            cls._cache[key] = cls(path, prefix)
        return cls._cache[key]


class NativeSim:
    """Owns one `mssim_handle`."""

    def __init__(self, lib: NativeLib, model: CompiledModel, num_envs: int, device: int):
        self.lib, self.model, self.num_envs, self.device = lib, model, num_envs, device
        desc, keep = make_model_desc(model)
        h = C.c_void_p()
        rc = lib.create(C.byref(desc), num_envs, device, C.byref(h))
        if rc != 0:
            msg = lib.last_error(None)
            raise NativeError(f"mssim create failed ({rc}): {msg.decode() if msg else ''}")
        self.h = h
        self._queries = {}

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.last_error(self.h)
            raise NativeError(f"mssim {what} failed ({rc}): {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bind(self, **ptrs):
        b = Buffers()
        for k, v in ptrs.items():
            setattr(b, k, v)
        self._check(self.lib.bind_buffers(self.h, C.byref(b)), "bind_buffers")

    def apply(self, what, stream=None):
        self._check(self.lib.apply(self.h, what, stream), "apply")

    def fetch(self, what, stream=None):
        self._check(self.lib.fetch(self.h, what, stream), "fetch")

    def defer_step_action(self, action_ptr, action_dim, n_substeps, stream=None):
        self._check(self.lib.defer_step_action(self.h, action_ptr, action_dim, n_substeps, stream), "defer_step_action")

    def defer_fetch(self, what):
        self._check(self.lib.defer_fetch(self.h, what), "defer_fetch")

    def step(self, n_substeps=1, stream=None):
        self._check(self.lib.step(self.h, n_substeps, stream), "step")

    def wake_all(self, stream=None):
        self._check(self.lib.wake_all(self.h, stream), "wake_all")

    def wake_envs(self, env_idx_ptr, n_idx, stream=None):
        self._check(self.lib.wake_envs(self.h, env_idx_ptr, n_idx, stream), "wake_envs")

    def update_kinematics(self, stream=None):
        self._check(self.lib.update_kinematics(self.h, stream), "update_kinematics")

    def set_timestep(self, dt):
        self._check(self.lib.set_timestep(self.h, dt), "set_timestep")

    def get_timestep(self):
        return float(self.lib.get_timestep(self.h))

    def create_pair_query(self, body_pairs):
        a = np.ascontiguousarray(body_pairs, dtype=np.int32).reshape(-1, 2)
        qid = C.c_int32()
        self._check(self.lib.create_pair_query(self.h, a.ctypes.data_as(_I32P), len(a), C.byref(qid)), "create_pair_query")
        return qid.value

    def query_pair_impulses(self, qid, out_ptr, stream=None):
        self._check(self.lib.query_pair_impulses(self.h, qid, out_ptr, stream), "query_pair_impulses")

    def create_body_query(self, rows):
        a = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        qid = C.c_int32()
        self._check(self.lib.create_body_query(self.h, a.ctypes.data_as(_I32P), len(a), C.byref(qid)), "create_body_query")
        return qid.value

    def query_body_impulses(self, qid, out_ptr, stream=None):
        self._check(self.lib.query_body_impulses(self.h, qid, out_ptr, stream), "query_body_impulses")

    def set_drive_properties(self, drive):
        a = np.ascontiguousarray(drive, dtype=np.float32).reshape(-1, 4)
        assert a.shape[0] == self.model.n_dof
        self._check(self.lib.set_drive_properties(self.h, a.ctypes.data_as(_F32P)), "set_drive_properties")

    def read_internal(self, name, out_ptr, max_items, stream=None):
        n = self.lib.read_internal(self.h, name.encode(), out_ptr, max_items, stream)
        if n < 0:
            self._check(n, f"read_internal({name})")
        return n

    def link_jacobian(self, link_index, out_ptr, stream=None):
        self._check(self.lib.link_jacobian(self.h, int(link_index), out_ptr, stream), "link_jacobian")

    def set_action_map(self, column, low, high, flags):
        col = np.ascontiguousarray(column, dtype=np.int32)
        lo = np.ascontiguousarray(low, dtype=np.float32)
        hi = np.ascontiguousarray(high, dtype=np.float32)
        fl = np.ascontiguousarray(flags, dtype=np.int32)
        assert len(col) == len(lo) == len(hi) == len(fl) == self.model.n_dof
        self._check(self.lib.set_action_map(self.h, col.ctypes.data_as(_I32P), lo.ctypes.data_as(_F32P), hi.ctypes.data_as(_F32P), fl.ctypes.data_as(_I32P)), "set_action_map")

    def set_ee_action_map(self, link_index, column0, rows, low, high, rot_scale, flags):
        self._check(self.lib.set_ee_action_map(self.h, int(link_index), int(column0), int(rows), float(low), float(high), float(rot_scale), int(flags)), "set_ee_action_map")

    def apply_action(self, action_ptr, action_dim, stream=None):
        self._check(self.lib.apply_action(self.h, action_ptr, action_dim, stream), "apply_action")

    def step_action(self, action_ptr, action_dim, n_substeps, stream=None):
        self._check(self.lib.step_action(self.h, action_ptr, action_dim, n_substeps, stream), "step_action")

    def task_peg_outputs(self, task: "PegTask", obs_ptr, reward_ptr, flags_ptr, head_ptr, stream=None):
        self._check(self.lib.task_peg_outputs(self.h, C.byref(task), obs_ptr, reward_ptr, flags_ptr, head_ptr, stream), "task_peg_outputs")

    def task_push_outputs(self, task: "PushTask", obs_ptr, reward_ptr, flags_ptr, stream=None):
        self._check(self.lib.task_push_outputs(self.h, C.byref(task), obs_ptr, reward_ptr, flags_ptr, stream), "task_push_outputs")

    def task_stack_outputs(self, task: "StackTask", obs_ptr, reward_ptr, flags_ptr, stream=None):
        if self.lib.task_stack_outputs is None:
            raise NativeError(f"{self.lib.path} has no task_stack_outputs (an extra of the HIP library, include/mssim_hip_tasks.h)")
        self._check(self.lib.task_stack_outputs(self.h, C.byref(task), obs_ptr, reward_ptr, flags_ptr, stream), "task_stack_outputs")

    def task_pusht_outputs(self, task: "PushTTask", obs_ptr, reward_ptr, flags_ptr, intersection_ptr=None, stream=None):
        if self.lib.task_pusht_outputs is None:
            raise NativeError(f"{self.lib.path} has no task_pusht_outputs (an extra of the HIP library, include/mssim_hip_tasks.h)")
        self._check(self.lib.task_pusht_outputs(self.h, C.byref(task), obs_ptr, reward_ptr, flags_ptr, intersection_ptr, stream), "task_pusht_outputs")

    def task_roll_outputs(self, task: "RollTask", obs_ptr, reward_ptr, flags_ptr, stream=None):
        if self.lib.task_roll_outputs is None:
            raise NativeError(f"{self.lib.path} has no task_roll_outputs (an extra of the HIP library, include/mssim_hip_tasks.h)")
        self._check(self.lib.task_roll_outputs(self.h, C.byref(task), obs_ptr, reward_ptr, flags_ptr, stream), "task_roll_outputs")

    def task_pull_outputs(self, task: "PullTask", obs_ptr, reward_ptr, flags_ptr, stream=None):
        if self.lib.task_pull_outputs is None:
            raise NativeError(f"{self.lib.path} has no task_pull_outputs (an extra of the HIP library, include/mssim_hip_tasks.h)")
        self._check(self.lib.task_pull_outputs(self.h, C.byref(task), obs_ptr, reward_ptr, flags_ptr, stream), "task_pull_outputs")

    def task_poke_outputs(self, task: "PokeTask", obs_ptr, reward_ptr, flags_ptr, metrics_ptr, stream=None):
        if self.lib.task_poke_outputs is None:
            raise NativeError(f"{self.lib.path} has no task_poke_outputs (an extra of the HIP library, include/mssim_hip_tasks.h)")
        self._check(self.lib.task_poke_outputs(self.h, C.byref(task), obs_ptr, reward_ptr, flags_ptr, metrics_ptr, stream), "task_poke_outputs")

    def task_liftpeg_outputs(self, task: "LiftPegTask", obs_ptr, reward_ptr, flags_ptr, stream=None):
        if self.lib.task_liftpeg_outputs is None:
            raise NativeError(f"{self.lib.path} has no task_liftpeg_outputs (an extra of the HIP library, include/mssim_hip_tasks.h)")
        self._check(self.lib.task_liftpeg_outputs(self.h, C.byref(task), obs_ptr, reward_ptr, flags_ptr, stream), "task_liftpeg_outputs")

    def task_place_outputs(self, task: "PlaceTask", obs_ptr, reward_ptr, flags_ptr, stream=None):
        if self.lib.task_place_outputs is None:
            raise NativeError(f"{self.lib.path} has no task_place_outputs (an extra of the HIP library, include/mssim_hip_tasks.h)")
        self._check(self.lib.task_place_outputs(self.h, C.byref(task), obs_ptr, reward_ptr, flags_ptr, stream), "task_place_outputs")

    def task_pulltool_outputs(self, task: "PullToolTask", obs_ptr, reward_ptr, flags_ptr, metrics_ptr, stream=None):
        if self.lib.task_pulltool_outputs is None:
            raise NativeError(f"{self.lib.path} has no task_pulltool_outputs (an extra of the HIP library, include/mssim_hip_tasks.h)")
        self._check(self.lib.task_pulltool_outputs(self.h, C.byref(task), obs_ptr, reward_ptr, flags_ptr, metrics_ptr, stream), "task_pulltool_outputs")

    def task_plug_outputs(self, task: "PlugTask", obs_ptr, reward_ptr, flags_ptr, metrics_ptr, stream=None):
        if self.lib.task_plug_outputs is None:
            raise NativeError(f"{self.lib.path} has no task_plug_outputs (an extra of the HIP library, include/mssim_hip_tasks.h)")
        self._check(self.lib.task_plug_outputs(self.h, C.byref(task), obs_ptr, reward_ptr, flags_ptr, metrics_ptr, stream), "task_plug_outputs")

    def task_draw_outputs(self, task: "DrawTask", obs_ptr, reward_ptr, flags_ptr, stream=None):
        if self.lib.task_draw_outputs is None:
            raise NativeError(f"{self.lib.path} has no task_draw_outputs (an extra of the HIP library, include/mssim_hip_tasks.h)")
        self._check(self.lib.task_draw_outputs(self.h, C.byref(task), obs_ptr, reward_ptr, flags_ptr, stream), "task_draw_outputs")

    def raycast_draw_dots(self, rid: int, camera: int, layer: "DotLayer", depth_ptr, rgba_ptr, stream=None):
        if self.lib.raycast_draw_dots is None:
            raise NativeError(f"{self.lib.path} has no raycast_draw_dots (an extra of the HIP library, include/mssim_hip_tasks.h)")
        self._check(self.lib.raycast_draw_dots(self.h, int(rid), int(camera), C.byref(layer), depth_ptr, rgba_ptr, stream), "raycast_draw_dots")

    def tail_step_count(self) -> int:
        """control steps that ran with the task epilogue at the control-step kernel's tail (HIP library only)"""
        if self.lib.tail_step_count is None:
            raise NativeError(f"{self.lib.path} has no tail_step_count (an extra of the HIP library, include/mssim_hip_tasks.h)")
        return int(self.lib.tail_step_count(self.h))

    def set_task_robot(self, robot: Optional["TaskRobot"]):
        """robot profile of the task epilogues (HIP library only); None removes it"""
        if self.lib.set_task_robot is None:
            raise NativeError(f"{self.lib.path} has no set_task_robot (an extra of the HIP library, include/mssim_hip_tasks.h)")
        self._check(self.lib.set_task_robot(self.h, None if robot is None else C.byref(robot)), "set_task_robot")

    def set_ee_ik_map(self, ik: "EeIkMap", target_pose_ptr):
        """iterative-IK block of the action map (HIP library only); `ik.link_index < 0` removes it"""
        if self.lib.set_ee_ik_map is None:
            raise NativeError(f"{self.lib.path} has no set_ee_ik_map (an extra of the HIP library, include/mssim_hip_tasks.h)")
        self._check(self.lib.set_ee_ik_map(self.h, C.byref(ik), target_pose_ptr), "set_ee_ik_map")

    def ee_ik_solve(self, target_pose_ptr, q0_ptr, q_out_ptr, iters_ptr=None, stream=None):
        if self.lib.ee_ik_solve is None:
            raise NativeError(f"{self.lib.path} has no ee_ik_solve (an extra of the HIP library, include/mssim_hip_tasks.h)")
        self._check(self.lib.ee_ik_solve(self.h, target_pose_ptr, q0_ptr, q_out_ptr, iters_ptr, stream), "ee_ik_solve")

    def raycast_create(self, scene_arrays: dict, cameras) -> int:
        """a ray-cast scene and its cameras (a list of CameraDesc) -> id (HIP library only); raises NativeError with the
        library's message where the scene is refused"""
        if self.lib.raycast_create is None:
            raise NativeError(f"{self.lib.path} has no raycast_create (an extra of the HIP library, include/mssim_hip_tasks.h)")
        scene, keep = make_raycast_scene(scene_arrays)
        cams = (CameraDesc * max(len(cameras), 1))(*cameras)
        rid = C.c_int32(-1)
        self._check(self.lib.raycast_create(self.h, C.byref(scene), cams, len(cameras), C.byref(rid)), "raycast_create")
        del keep
        return rid.value

    def raycast_destroy(self, rid: int):
        if self.lib.raycast_destroy is None:
            raise NativeError(f"{self.lib.path} has no raycast_destroy (an extra of the HIP library, include/mssim_hip_tasks.h)")
        self._check(self.lib.raycast_destroy(self.h, int(rid)), "raycast_destroy")

    def raycast_render(self, rid: int, camera: int, pos_seg_ptr, depth_ptr=None, stream=None):
        if self.lib.raycast_render is None:
            raise NativeError(f"{self.lib.path} has no raycast_render (an extra of the HIP library, include/mssim_hip_tasks.h)")
        self._check(self.lib.raycast_render(self.h, int(rid), int(camera), pos_seg_ptr, depth_ptr, stream), "raycast_render")

    def raycast_set_colours(self, rid: int, shape_rgba, env_shape_rgba=None):
        """host arrays, copied by the call: shape_rgba [n_shape, 4] (r, g, b, checker cell size in metres), env_shape_rgba
        [n_env_shape, N, 4] or None"""
        if self.lib.raycast_set_colours is None:
            raise NativeError(f"{self.lib.path} has no raycast_set_colours (an extra of the HIP library, include/mssim_hip_tasks.h)")
        a = np.ascontiguousarray(shape_rgba, dtype=np.float32).reshape(-1, 4)
        e = None if env_shape_rgba is None else np.ascontiguousarray(env_shape_rgba, dtype=np.float32)
        self._check(self.lib.raycast_set_colours(self.h, int(rid), a.ctypes.data_as(_F32P), None if e is None else e.ctypes.data_as(_F32P)), "raycast_set_colours")

    def raycast_shade(self, rid: int, camera: int, rgba_ptr, stream=None):
        if self.lib.raycast_shade is None:
            raise NativeError(f"{self.lib.path} has no raycast_shade (an extra of the HIP library, include/mssim_hip_tasks.h)")
        self._check(self.lib.raycast_shade(self.h, int(rid), int(camera), rgba_ptr, stream), "raycast_shade")

    def task_pick_outputs(self, task: "PickTask", obs_ptr, reward_ptr, flags_ptr, stream=None):
        self._check(self.lib.task_pick_outputs(self.h, C.byref(task), obs_ptr, reward_ptr, flags_ptr, stream), "task_pick_outputs")

    def profile_enable(self, on=True):
        self._check(self.lib.profile_enable(self.h, 1 if on else 0), "profile_enable")

    def profile_read(self):
        """-> {"solve": (ms, launches), "narrow": (ms, launches)} since the last read"""
        ms = (C.c_float * 2)()
        cnt = (C.c_int32 * 2)()
        self._check(self.lib.profile_read(self.h, ms, cnt), "profile_read")
        return {"solve": (float(ms[0]), int(cnt[0])), "narrow": (float(ms[1]), int(cnt[1]))}

    def overflow_count(self, stream=None):
        return int(self.lib.overflow_count(self.h, stream))
