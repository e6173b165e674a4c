"""Scripted StackCube-v1 policy (test helper): pick cube A, carry it over cube B, set it down and let go.

Closed loop on the `pd_ee_delta_pose` controller (delta of the TCP in the root frame, Euler delta in root-aligned axes;
the Panda's root is axis-aligned with the world): every step commands the clipped offset to the current waypoint, and
turns the hand about z so that the fingers close across two faces of cube A (the cubes are yawed at random)."""
import math

import torch

# (waypoint, gripper, steps): waypoints are functions of (A at the phase's start, B now)
PHASES = (
    ("above_a", 1.0, 25),
    ("at_a", 1.0, 15),
    ("at_a", -1.0, 10),   # close
    ("lift", -1.0, 15),
    ("above_b", -1.0, 25),
    ("on_b", -1.0, 20),
    ("on_b", 1.0, 10),    # release
    ("retreat", 1.0, 20),
)


def _waypoint(name, a0, b):
    up = torch.tensor([0.0, 0.0, 1.0], device=a0.device)
    return {
        "above_a": a0 + 0.08 * up,
        "at_a": a0,
        "lift": a0 + 0.10 * up,
        "above_b": b + 0.10 * up,
        "on_b": b + 0.042 * up,  # A's centre 4 cm above B's, 2 mm to spare
        "retreat": b + 0.12 * up,
    }[name]


def _yaw(q):
    """yaw of a wxyz quaternion's y axis (the Panda's finger-closing axis / a cube face normal)"""
    w, x, y, z = q.unbind(-1)
    yx, yy = 2 * (x * y - w * z), 1 - 2 * (x * x + z * z)
    return torch.atan2(yy, yx)


def run_scripted_stack(env):
    """runs one scripted episode from the env's current state; returns the last step's info"""
    base = env.unwrapped
    assert base.control_mode == "pd_ee_delta_pose"
    N, dev = base.num_envs, base.device
    info = None
    for name, grip, steps in PHASES:
        a0 = base.cubeA.pose.p.clone()
        for _ in range(steps):
            b = base.cubeB.pose.p
            tcp = base.agent.tcp.pose
            act = torch.zeros(N, 7, device=dev)
            act[:, :3] = ((_waypoint(name, a0, b) - tcp.p) / 0.1).clamp(-1, 1)
            # hand yaw onto the nearest face of A (a quarter turn is the cube's symmetry)
            err = _yaw(base.cubeA.pose.q) - _yaw(tcp.q)
            err = torch.remainder(err + math.pi / 4, math.pi / 2) - math.pi / 4
            act[:, 5] = (err / 0.1).clamp(-1, 1)
            act[:, 6] = grip
            _, _, _, _, info = env.step(act)
    return info
