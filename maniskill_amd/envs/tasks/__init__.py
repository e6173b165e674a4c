from .tabletop import (LiftPegUprightEnv, PegInsertionSideEnv, PickCubeEnv, PlaceSphereEnv, PokeCubeEnv, PullCubeEnv, PullCubeToolEnv, PushCubeEnv, PushTEnv,
                       RollBallEnv, StackCubeEnv)
from .empty_env import EmptyEnv
