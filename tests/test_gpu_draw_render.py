"""DrawTriangle-v1's drawing in the shaded view (`render_mode="rgb_array"`): the dot layer k_raycast_dots composited over the
viewer rig's picture, at 64 x 48. The camera looks at a point of the canvas away from the goal's outline, with its principal
point on the centre of pixel (32, 24), so that this pixel's ray meets the dot plane at the point itself (checked with
`get_params()`). A dot placed there under the raised arm is red in that pixel and the canvas white around it; the frame before
has no red; with the stick parked over the dot the pixel is not red; the sensors' depth of the same state does not know the
dot."""
import math

import numpy as np
import pytest
import torch

from tests import draw_reference as ref

pytestmark = pytest.mark.gpu
W, H = 64, 48
# where PushT's start configuration holds the stick's tip (tests/test_gpu_draw_triangle.py LOW_QPOS): on the canvas, 0.3 m
# from the goal's outline
SPOT = (-0.321, 0.284)
LOW_QPOS = np.array([0.662, 0.212, 0.086, -2.685, -0.115, 2.898, 1.673])
RED = (204, 51, 51)  # floor(255 c + 0.5) of the brush colour 0.8, 0.2, 0.2: both lights reach an upward face


def _red(pic):
    return (pic[..., 0] > 150) & (pic[..., 1] < 100) & (pic[..., 2] < 100)


def _frame(env):
    env.render()
    base = env.unwrapped
    return base._human_render_cameras()["render_camera"].get_picture().cpu().numpy().copy()


def test_a_dot_shows_on_the_canvas_and_the_arm_hides_it():
    import maniskill_amd.envs  # noqa: F401
    import gymnasium as gym
    from maniskill_amd.utils import sapien_utils

    N = 2
    z = ref.CANVAS_THICKNESS + ref.DOT_THICKNESS
    f = H / (2 * math.tan(0.6))
    pose = sapien_utils.look_at(eye=[0.3, 0.3, 0.8], target=[*SPOT, z])
    view = dict(width=W, height=H, fov=None, intrinsic=[[f, 0, 32.5], [0, f, 24.5], [0, 0, 1]], pose=pose)
    env = gym.make("DrawTriangle-v1", num_envs=N, sim_backend="physx_cuda", render_mode="rgb_array", human_render_camera_configs=view,
                   sensor_configs=dict(width=W, height=H))
    base = env.unwrapped
    env.reset(seed=4)
    before = _frame(env)
    assert before.shape == (N, H, W, 3) and not _red(before).any()
    depth0 = {k: v["depth"].cpu().clone() for k, v in base._get_obs_sensor_data().items()}
    # the spot's projected centre, from the camera's own parameters
    prm = base._human_render_cameras()["render_camera"].get_params()
    E, K = prm["extrinsic_cv"].cpu().double().numpy(), prm["intrinsic_cv"].cpu().double().numpy()
    for e in range(N):
        pc = E[e] @ np.array([*SPOT, z, 1.0])
        u, v = K[e, 0, 0] * pc[0] / pc[2] + K[e, 0, 2], K[e, 1, 1] * pc[1] / pc[2] + K[e, 1, 2]
        assert abs(u - 32.5) < 1e-3 and abs(v - 24.5) < 1e-3, (u, v)
    # one dot on the spot; a table entry that is not drawn, elsewhere on the canvas, paints nothing
    base.dots[:, 0] = torch.tensor(SPOT, device=base.device)
    base.dot_near[:, 0] = 0
    base.dots[:, 1] = torch.tensor([0.1, -0.3], device=base.device)
    base.draw_step[:] = 2
    shown = _frame(env)
    assert (shown[:, 24, 32] == RED).all(), shown[:, 24, 32]
    ring = [(24 + dv, 32 + du) for dv in (-2, 0, 2) for du in (-2, 0, 2) if (dv, du) != (0, 0)]
    for v, u in ring:  # (a pixel is 23 mm at that distance, the disc 10 mm in radius)
        assert (shown[:, v, u] == 255).all(), (v, u, shown[:, v, u])
    changed = (shown != before).any(-1)
    assert changed.sum() >= N and (changed == _red(shown)).all(), "nothing but the dot's pixels changed"
    assert changed[:, 20:29, 28:37].sum() == changed.sum()
    depth1 = {k: v["depth"].cpu().clone() for k, v in base._get_obs_sensor_data().items()}
    assert depth0.keys() == depth1.keys() and all(torch.equal(depth0[k], depth1[k]) for k in depth0), "the sensors see collision geometry only"
    # the stick parked over the dot
    base.agent.robot.set_qpos(torch.from_numpy(np.tile(LOW_QPOS, (N, 1)).astype(np.float32)).to(base.device))
    base.scene._gpu_apply_all()
    base.scene.px.gpu_update_articulation_kinematics()
    base.scene._gpu_fetch_all()
    tip = base.agent.tcp.pose.p.cpu().numpy()
    assert np.abs(tip[:, :2] - np.array(SPOT)).max() < 3e-3 and (tip[:, 2] < 0.03).all(), tip
    hidden = _frame(env)
    assert not _red(hidden)[:, 24, 32].any(), hidden[:, 24, 32]
    env.close()
