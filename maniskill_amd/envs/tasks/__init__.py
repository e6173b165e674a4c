from .tabletop import (DrawTriangleEnv, LiftPegUprightEnv, PegInsertionSideEnv, PickCubeEnv, PlaceSphereEnv, PlugChargerEnv, PokeCubeEnv, PullCubeEnv, PullCubeToolEnv, PushCubeEnv, PushTEnv,
                       RollBallEnv, StackCubeEnv)
from .empty_env import EmptyEnv
