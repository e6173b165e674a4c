from .panda import Panda, PandaStick, PandaWristCam
from .fetch import Fetch
