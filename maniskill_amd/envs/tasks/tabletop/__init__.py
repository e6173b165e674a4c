from .pick_cube import PickCubeEnv
from .push_cube import PushCubeEnv
from .peg_insertion_side import PegInsertionSideEnv
from .stack_cube import StackCubeEnv
from .push_t import PushTEnv
from .roll_ball import RollBallEnv
from .pull_cube import PullCubeEnv
