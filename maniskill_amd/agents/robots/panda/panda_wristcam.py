"""Panda with the wrist camera mount (counterpart of
mani_skill/agents/robots/panda/panda_wristcam.py): panda_v3.urdf, same controllers, and the hand
camera on `camera_link` (depth / segmentation / position through the ray caster; no colour)."""
import numpy as np

from maniskill_amd import PACKAGE_ASSET_DIR
from maniskill_amd.agents.registration import register_agent
from maniskill_amd.sensors.camera import CameraConfig
from maniskill_amd.utils.structs.pose import Pose

from .panda import Panda


@register_agent()
class PandaWristCam(Panda):
    uid = "panda_wristcam"
    urdf_path = f"{PACKAGE_ASSET_DIR}/robots/panda/panda_v3.urdf"

    @property
    def _sensor_configs(self):
        return [
            CameraConfig(
                uid="hand_camera",
                pose=Pose.create_from_pq(p=[0, 0, 0], q=[1, 0, 0, 0]),
                width=128,
                height=128,
                fov=np.pi / 2,
                near=0.01,
                far=100,
                mount=self.robot.links_map["camera_link"],
            )
        ]
