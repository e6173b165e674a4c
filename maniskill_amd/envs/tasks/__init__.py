from .tabletop import PegInsertionSideEnv, PickCubeEnv, PushCubeEnv, StackCubeEnv
from .empty_env import EmptyEnv
