"""Colours for the constructed scenes of tests/raycast_cases.py and tests/raycast_mesh_cases.py, and the float64 pictures of
tests/shade_reference.py over them; shared by tests/test_shade.py (CPU) and tests/test_gpu_shade.py (k_raycast_shade
against the reference).

The rule is seeded by the scene's name: every shape draws r, g, b from [0.15, 1], and one shape per scene is checkered
(CHECKERED: shape index and cell size). That is the ground plane with 1 m cells where the cameras see it within a few
metres; where they see it tens of metres away at a glancing angle, a hundredth of a pixel spans a cell and the picture is
not decided by the geometry, so there a bounded shape carries the checker (the ball of "many" is the first of the second
staged chunk; a shape the 1 x 1 camera sees is no candidate, since a hundredth of ITS pixel is centimetres wide). No cell size divides a face's distance from its shape's origin: a point ON a cell boundary has no parity. The
mesh scenes also carry a colour per env for every per-env slot (`env_shape_rgba`), which only k_raycast_shade<true> reads.

CONFIGS / MESH_CONFIGS are the (scene, N) pairs of the two case files, unchanged: under the face and checker rules of
shade_reference.ambiguous every image stays within raycast_cases.MAX_AMBIGUOUS_SHARE (test_shade.py asserts it).

MEASURED_LEVELS is the largest channel difference between the float32 and the float64 run of the reference over the
unambiguous pixels of all those images, measured by test_shade.py::test_float32_reference_within_a_level. The GPU test's
bound is not taken from it: one level follows from the arithmetic (a unit normal and two dot products in float32 are some
1e-6 of full scale off, so a rounding to a byte moves by at most one).
"""
import functools
import zlib

import numpy as np

from tests import raycast_cases as rcc
from tests import raycast_mesh_cases as rmc
from tests import raycast_reference as rr
from tests import shade_reference as sr

CONFIGS = rcc.CONFIGS
MESH_CONFIGS = rmc.CONFIGS
MEASURED_LEVELS = 0  # (measured: the float32 run rounds every unambiguous channel of every image to the float64 run's byte)
CHECKERED = {("plain", "types"): (0, 1.0), ("plain", "near_far"): (4, 0.17), ("plain", "many"): (64, 0.05),
             ("mesh", "meshes"): (0, 1.0), ("mesh", "terrain"): (1, 0.11), ("mesh", "inside"): (0, 0.17), ("mesh", "many"): (0, 1.0)}


def build(kind, name, N):
    return (rmc if kind == "mesh" else rcc).build(name, N)


@functools.lru_cache(maxsize=None)
def colours(kind, name, N):
    """dict(shape_rgba [S, 4], env_shape_rgba [slots, N, 4] for the mesh scenes that have slots)"""
    scene = build(kind, name, N)["scene"]
    rng = np.random.default_rng(zlib.crc32(f"{kind}/{name}".encode()))
    S = len(scene["shape_type"])
    rgba = np.zeros((S, 4), dtype=np.float32)
    rgba[:, :3] = rng.uniform(0.15, 1.0, size=(S, 3))
    shape, cell = CHECKERED[(kind, name)]
    rgba[shape, 3] = cell
    out = dict(shape_rgba=rgba)
    slots = int(scene["n_env_shape"])
    if kind == "mesh" and slots:
        env = np.zeros((slots, N, 4), dtype=np.float32)
        env[..., :3] = rng.uniform(0.15, 1.0, size=(slots, N, 3))
        out["env_shape_rgba"] = env
    return out


@functools.lru_cache(maxsize=None)
def reference(kind, name, N):
    """per camera, per env: (float64 picture dict, ambiguous [H, W]) -- computed once, shared by the tests"""
    c, col = build(kind, name, N), colours(kind, name, N)
    return [[sr.ambiguous(c["scene"], col, cam, c["rigid"], N, e)[::-1] for e in range(N)] for cam in c["cameras"]]


def all_configs():
    return [("plain", n, N) for n, N in CONFIGS] + [("mesh", n, N) for n, N in MESH_CONFIGS]
