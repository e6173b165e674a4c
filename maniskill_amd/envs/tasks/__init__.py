from .tabletop import PegInsertionSideEnv, PickCubeEnv, PushCubeEnv, PushTEnv, StackCubeEnv
from .empty_env import EmptyEnv
