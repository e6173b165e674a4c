from .tabletop import LiftPegUprightEnv, PegInsertionSideEnv, PickCubeEnv, PokeCubeEnv, PullCubeEnv, PushCubeEnv, PushTEnv, RollBallEnv, StackCubeEnv
from .empty_env import EmptyEnv
