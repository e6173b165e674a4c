"""Camera sensors over the native ray caster (counterpart of mani_skill/sensors/camera.py).

`CameraConfig` is the record task and robot files construct (camera.py:33-68 of the reference). `Camera` renders the
geometric modalities -- depth, actor-level segmentation, camera-frame position -- by casting rays at the compiled
model's collision geometry (include/mssim_hip_tasks.h `mssim_raycast_*`): there are no visual meshes or textures
in this build, and no colour OBSERVATIONS. One launch per camera fills one `int16 [N, H, W, 4]` buffer in the layout of the
reference's minimal shader (x, y, z in millimetres in the camera's OpenGL frame, then the segmentation id). `get_obs`
returns `position` and `segmentation` as views of that buffer, which the next capture overwrites (copy what you keep
across steps), and `depth` as a tensor of its own.

`capture_picture` / `get_picture` give a picture for people: the same geometry flat-shaded, one colour per shape under
two fixed lights (`mssim_raycast_shade`). That is what `env.render()` and the episode videos show. It is not the
reference's rendered `rgb` and is not handed out under that key: `get_obs(rgb=True)` keeps raising.
"""
import copy
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch

from maniskill_amd.utils.structs.pose import Pose


@dataclass
class CameraConfig:
    uid: str
    pose: Pose
    width: int
    height: int
    fov: float = None
    near: float = 0.01
    far: float = 100
    intrinsic: object = None
    entity_uid: Optional[str] = None
    mount: object = None
    shader_pack: Optional[str] = "minimal"
    shader_config: object = None

    def __post_init__(self):
        self.pose = Pose.create(self.pose)


def cameras_by_uid(declared) -> Dict[str, CameraConfig]:
    """what a task or robot declares -- one CameraConfig, a sequence of them, or a mapping uid -> config -- as a fresh
    mapping uid -> config, in declaration order"""
    if isinstance(declared, CameraConfig):
        declared = [declared]
    if isinstance(declared, dict):
        return dict(declared)
    if not isinstance(declared, (list, tuple)):
        raise TypeError(f"camera configs are a CameraConfig, a list of them or a dict, not {type(declared).__name__}")
    return {c.uid: c for c in declared}


_CONFIG_FIELDS = frozenset(CameraConfig.__dataclass_fields__)


def apply_sensor_overrides(cameras: Dict[str, CameraConfig], overrides: Dict[str, object], what: str = "sensor_configs") -> None:
    """The user's `sensor_configs` (or, under that name in `what`, `human_render_camera_configs`) applied in place. A key that is a camera's uid holds a dict of field overrides for
    that camera; any other key is a field set on every camera. Per-camera values win over the ones for all. A pose may
    be a Pose or seven numbers (p, q(wxyz): what a json-serialisable `gym.make` argument can carry)."""

    def checked(fields: dict, where: str) -> dict:
        unknown = sorted(set(fields) - _CONFIG_FIELDS)
        if unknown:
            raise AttributeError(f"{what}{where}: CameraConfig has no field {', '.join(unknown)} (its fields: {', '.join(sorted(_CONFIG_FIELDS))})")
        out = dict(fields)
        if isinstance(out.get("pose"), (list, tuple)):
            p = [float(x) for x in out["pose"]]
            if len(p) != 7:
                raise ValueError(f"{what}{where}: a pose given as numbers is p(3), q(4), got {len(p)} numbers")
            out["pose"] = Pose.create_from_pq(p=p[:3], q=p[3:])
        return out

    for_all = checked({k: v for k, v in overrides.items() if k not in cameras}, "")
    for uid, config in cameras.items():
        own = overrides.get(uid, {})
        if not isinstance(own, dict):
            raise TypeError(f"{what}[{uid!r}] must be a dict of CameraConfig fields")
        for field, value in {**for_all, **checked(own, f"[{uid!r}]")}.items():
            setattr(config, field, copy.deepcopy(value))
        config.pose = Pose.create(config.pose)


# a SAPIEN-axes camera point (x forward, y left, z up) from its OpenCV coordinates (x right, y down, z forward)
_CV_TO_SAPIEN = np.array([[0.0, 0.0, 1.0, 0.0], [-1.0, 0.0, 0.0, 0.0], [0.0, -1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
_GL_TO_CV = np.diag([1.0, -1.0, -1.0, 1.0])


class RaycastRig:
    """The cameras of one env object on one native ray-cast scene. The scene (hull face planes, triangle meshes with
    their BVH, segmentation ids) is built and uploaded at the first capture, so that an env that never looks through its
    cameras pays nothing; the colour tables of the shaded view are built and uploaded at the first picture. `viewer`: the
    scene also draws the visual primitives of bodies whose visuals are not their collision shapes (a goal marker), as the
    human render cameras do; the sensors' scene holds collision geometry alone."""

    def __init__(self, scene, seg_ids: Dict[str, int], viewer: bool = False):
        self.scene, self.seg_ids, self.viewer = scene, seg_ids, viewer
        self.cameras: List["Camera"] = []
        self._id = None
        self._colours = None

    def add(self, camera: "Camera") -> int:
        assert self._id is None, "cameras are added before the first capture"
        self.cameras.append(camera)
        return len(self.cameras) - 1

    def _create(self):
        if self._id is None:
            from maniskill_amd.model.compile import raycast_colours, raycast_scene, raycast_viewer_scene

            if self.viewer:
                arrays, self._colours = raycast_viewer_scene(self.scene.model, self.seg_ids)
            else:
                arrays, self._colours = raycast_scene(self.scene.model, self.seg_ids, meshes=True), raycast_colours(self.scene.model, self.seg_ids)
            self._id = self.scene.px.raycast_create(arrays, [c._desc() for c in self.cameras])
        return self._id

    def shade(self, camera: "Camera"):
        px, rid = self.scene.px, self._create()
        if self._colours is not None:  # (uploaded once, at the first picture)
            px.raycast_set_colours(rid, self._colours["shape_rgba"], self._colours.get("env_shape_rgba"))
            self._colours = None
        if camera._rgba is None:
            camera._rgba = torch.zeros((self.scene.num_envs, camera.height, camera.width, 4), dtype=torch.uint8, device=self.scene.device)
        px.raycast_shade(rid, camera._index, camera._rgba)

    def draw_dots(self, camera: "Camera", layer):
        """a dot layer (`native.DotLayer`) painted over the camera's shaded view, after `shade`: one ray-cast launch for this
        scene's float depth (what hides a dot), one compositing launch. The camera's position / segmentation buffer is
        overwritten on the way, as by a capture."""
        px, rid = self.scene.px, self._create()
        assert camera._rgba is not None, f"{camera.uid}: capture_picture() first"
        if camera._depth is None:
            camera._depth = torch.zeros((self.scene.num_envs, camera.height, camera.width), dtype=torch.float32, device=self.scene.device)
        if camera._pos_seg is None:
            camera._pos_seg = torch.zeros((self.scene.num_envs, camera.height, camera.width, 4), dtype=torch.int16, device=self.scene.device)
        px.raycast_render(rid, camera._index, camera._pos_seg, camera._depth)
        px.raycast_draw_dots(rid, camera._index, layer, camera._depth, camera._rgba)

    def render(self, camera: "Camera"):
        px = self.scene.px
        self._create()
        if camera._pos_seg is None:
            camera._pos_seg = torch.zeros((self.scene.num_envs, camera.height, camera.width, 4), dtype=torch.int16, device=self.scene.device)
        px.raycast_render(self._id, camera._index, camera._pos_seg)


class Camera:
    """One pinhole camera, fixed in the env frame or mounted on a link / actor (camera.py:127-282 of the reference)."""

    def __init__(self, camera_config: CameraConfig, scene, articulation=None, rig: RaycastRig = None):
        self.config = camera_config
        self.scene = scene
        cfg = camera_config
        self.entity = None
        if cfg.mount is not None:
            self.entity = cfg.mount
        elif cfg.entity_uid is not None:
            if articulation is not None:
                self.entity = next((l for l in articulation.get_links() if l.name == cfg.entity_uid), None)
            if self.entity is None:
                raise RuntimeError(f"Mount entity ({cfg.entity_uid}) is not found")
        assert (cfg.fov is None) != (cfg.intrinsic is None), "a camera is given by its fov or by its intrinsic matrix"
        W, H = int(cfg.width), int(cfg.height)
        if cfg.intrinsic is not None:
            K = np.asarray(cfg.intrinsic, dtype=np.float64).reshape(3, 3)
            self.fx, self.fy, self.cx, self.cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
        else:  # the vertical field of view, square pixels
            self.fx = self.fy = H / (2.0 * np.tan(float(cfg.fov) / 2.0))
            self.cx, self.cy = W / 2.0, H / 2.0
        self.width, self.height = W, H
        N, dev = scene.num_envs, scene.device
        self._local = cfg.pose.raw_pose.to(device=dev, dtype=torch.float32)
        assert len(self._local) in (1, N), f"{cfg.uid}: one pose, or one per env"
        self._pos_seg = None  # int16 [N, H, W, 4], allocated at the first capture
        self._rgba = None     # uint8 [N, H, W, 4], allocated at the first picture
        self._depth = None    # float32 [N, H, W], allocated at the first picture with a dot layer
        self._rig = rig
        self._index = rig.add(self) if rig is not None else None

    @property
    def uid(self) -> str:
        return self.config.uid

    def _desc(self) -> dict:
        row = -1 if self.entity is None else self.entity._body_row
        assert row is not None, f"{self.uid}: a camera cannot ride on a static actor (give it the pose instead)"
        d = dict(width=self.width, height=self.height, fx=self.fx, fy=self.fy, cx=self.cx, cy=self.cy, near=self.config.near, far=self.config.far, mount_row=row)
        if len(self._local) == 1:
            d["pose"] = self._local[0].cpu().numpy()
        else:
            d["env_pose"] = self._local.contiguous()
        return d

    def capture(self):
        """one ray-cast launch on the current stream, from the pose buffers as they are (after the fetch)"""
        self._rig.render(self)

    def capture_picture(self):
        """one shading launch on the current stream, from the pose buffers as they are: the flat-shaded view"""
        self._rig.shade(self)

    def draw_dots(self, layer):
        """paints a dot layer over the picture of the last `capture_picture` (`RaycastRig.draw_dots`)"""
        self._rig.draw_dots(self, layer)

    def get_picture(self) -> torch.Tensor:
        """uint8 [N, H, W, 3]: the shaded view of the last `capture_picture`, a VIEW of the camera's RGBA buffer (the next
        picture overwrites it). A picture for people, not the `rgb` observation of a renderer."""
        assert self._rgba is not None, f"{self.uid}: capture_picture() first"
        return self._rgba[..., :3]

    def get_obs(self, rgb: bool = False, depth: bool = True, position: bool = True, segmentation: bool = True, normal: bool = False,
                albedo: bool = False, apply_texture_transforms: bool = True) -> Dict[str, torch.Tensor]:
        """the captured image, in the dtypes and shapes of the reference's minimal shader:
        depth        int16 [N, H, W, 1] millimetres, 0 = nothing. Computed (-z of the buffer): a FRESH tensor on every call,
                     safe to keep.
        position     int16 [N, H, W, 3] millimetres, OpenGL camera frame. A VIEW of the camera's buffer: the next capture
                     overwrites it, copy what you keep.
        segmentation int16 [N, H, W, 1] `per_scene_id`, 0 = background. A VIEW of the buffer, as position."""
        if rgb or normal or albedo:
            raise NotImplementedError("this build's cameras cast rays at geometry: depth, segmentation and position; colour (rgb, normal, albedo) is missing "
                                      "as an observation (get_picture() is a flat-shaded view for people, not a renderer's rgb)")
        assert self._pos_seg is not None, f"{self.uid}: capture() first"
        out = {}
        if depth:
            out["depth"] = -self._pos_seg[..., 2:3]
        if position:
            out["position"] = self._pos_seg[..., :3]
        if segmentation:
            out["segmentation"] = self._pos_seg[..., 3:4]
        return out

    def get_images(self, obs) -> Dict[str, torch.Tensor]:
        return camera_observations_to_images(obs)

    def cam2world(self) -> torch.Tensor:
        """[N, 4, 4] env frame <- camera, SAPIEN axes: the mount's current pose composed with the local one"""
        N = self.scene.num_envs
        local = Pose.create(self._local if len(self._local) == N else self._local.expand(N, 7))
        pose = local if self.entity is None else self.entity.pose * local
        return pose.to_transformation_matrix()

    def get_params(self) -> Dict[str, torch.Tensor]:
        T = self.cam2world()
        cv = T @ torch.as_tensor(_CV_TO_SAPIEN, dtype=T.dtype, device=T.device)
        K = torch.tensor([[self.fx, 0.0, self.cx], [0.0, self.fy, self.cy], [0.0, 0.0, 1.0]], dtype=torch.float32, device=T.device)
        return dict(
            extrinsic_cv=torch.linalg.inv(cv)[:, :3, :4],
            cam2world_gl=cv @ torch.as_tensor(_GL_TO_CV, dtype=T.dtype, device=T.device),
            intrinsic_cv=K.expand(len(T), 3, 3).clone(),
        )


# three odd multipliers spread consecutive ids over the byte range of the three colour channels (the reference's
# pictures of a segmentation use the same ones, so that the two builds' pictures can be laid side by side)
_ID_COLOUR = (11, 61, 127)


def id_colours(ids: torch.Tensor) -> torch.Tensor:
    """uint8 [..., 3] picture of an integer id image [..., 1]: channel c = (id * _ID_COLOUR[c]) mod 256; id 0 is black"""
    if ids.shape[-1] != 1:
        raise ValueError(f"an id image has one channel, got shape {tuple(ids.shape)}")
    mult = torch.tensor(_ID_COLOUR, dtype=torch.int32, device=ids.device)
    return (ids.to(torch.int32) * mult).remainder(256).to(torch.uint8)


def depth_greys(depth: torch.Tensor, max_depth=None) -> torch.Tensor:
    """uint8 [..., 3] grey picture of a depth image [..., 1]: 0 = nothing or nearest, 255 = `max_depth` (the image's own
    maximum by default) and beyond; an empty image stays black"""
    d = depth.to(torch.float32)
    top = d.max().clamp(min=1e-9) if max_depth is None else float(max_depth)
    return (d / top).clamp(0, 1).mul(255).to(torch.uint8).expand(*d.shape[:-1], 3).contiguous()


def camera_observations_to_images(observations: Dict[str, torch.Tensor], max_depth=None) -> Dict[str, torch.Tensor]:
    """uint8 pictures of one camera's observation dict: `depth` and `position` (its -z) as greys, `segmentation` as id colours"""
    pictures = {}
    for key, image in observations.items():
        if key == "segmentation":
            pictures[key] = id_colours(image)
        elif key == "depth":
            pictures[key] = depth_greys(image, max_depth)
        elif key == "position":
            pictures[key] = depth_greys(-image[..., 2:3], max_depth)
    return pictures
