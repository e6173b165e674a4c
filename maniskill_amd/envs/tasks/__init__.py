from .tabletop import PegInsertionSideEnv, PickCubeEnv, PullCubeEnv, PushCubeEnv, PushTEnv, RollBallEnv, StackCubeEnv
from .empty_env import EmptyEnv
