from .panda import Panda
from .panda_stick import PandaStick
from .panda_wristcam import PandaWristCam
