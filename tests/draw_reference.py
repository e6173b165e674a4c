"""DrawTriangle's drawing rules in float64 numpy, written from the task's statement (maniskill_amd/envs/tasks/tabletop/
draw_triangle.py, include/mssim_hip_tasks.h `mssim_draw_task`), not from either implementation:

  * dot k of an env is written at control step k of its episode, touched or not; a counter at MAX_DOTS writes nothing
  * drawn  iff tcp.z < 0.02 + 0.003 + 0.005 (strict; a NaN is not drawn)
  * near   iff some reference point of the env lies closer than THRESHOLD to the dot (strict; Euclidean, in the plane)
  * a reference point is hit once a drawn dot lies closer than THRESHOLD to it, and stays hit
  * success of an env iff every one of ITS drawn dots is near and all 153 of ITS reference points are hit

`batch_wide_success` is the reference implementation's formula restated literally (one `all` over the drawn dots of the whole
batch); tests/test_draw_triangle.py shows the two agree for one env. Pinned by hand-made cases there."""
import numpy as np

MAX_DOTS, N_REF = 300, 153
CANVAS_THICKNESS, DOT_THICKNESS, BRUSH_RADIUS, THRESHOLD = 0.02, 0.003, 0.01, 0.025
Z_THRESH = CANVAS_THICKNESS + DOT_THICKNESS + 0.005
EDGE = 0.3
RADIUS = (EDGE / 2) / np.sqrt(3.0)


def original_vertices():
    """[3, 3] corners of the goal triangle in its body frame (z = 0.01), from the three edge centres at 90, 210 and 330 degrees"""
    c = [np.array([RADIUS * np.cos(np.pi / 2 + k * 2 * np.pi / 3), RADIUS * np.sin(np.pi / 2 + k * 2 * np.pi / 3), 0.01]) for k in range(3)]
    return np.array([(c[0] + c[2]) - c[1], (c[0] + c[1]) - c[2], (c[1] + c[2]) - c[0]])


def quat_matrix(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def vertices_of(goal_pose):
    """[3, 3] corners in the env frame for a goal pose p, q(wxyz)"""
    g = np.asarray(goal_pose, dtype=np.float64)
    return original_vertices() @ quat_matrix(g[3:]).T + g[:3]


def reference_points(verts_xy):
    """[3, 2] -> [153, 2]: per edge 51 points at linspace(0, 1, 52)[:-1] from its first corner"""
    v = np.asarray(verts_xy, dtype=np.float64)
    t = np.linspace(0.0, 1.0, 52)[:-1, None]
    return np.concatenate([v[i] * (1 - t) + v[(i + 1) % 3] * t for i in range(3)], 0)


def new_state(N):
    return dict(dots=np.zeros((N, MAX_DOTS, 2)), dot_near=np.full((N, MAX_DOTS), -1, dtype=np.int8), ref_hit=np.zeros((N, N_REF), dtype=bool),
                draw_step=np.zeros(N, dtype=np.int64))


def append(state, tcp, triangles):
    """one control step: tcp [N, 3], triangles [N, 153, 2]; updates `state` in place"""
    tcp, triangles = np.asarray(tcp, dtype=np.float64), np.asarray(triangles, dtype=np.float64)
    for e in range(len(tcp)):
        k = int(state["draw_step"][e])
        if k >= MAX_DOTS:
            continue
        drawn = bool(tcp[e, 2] < Z_THRESH)
        if drawn:
            with np.errstate(invalid="ignore"):
                close = np.hypot(triangles[e, :, 0] - tcp[e, 0], triangles[e, :, 1] - tcp[e, 1]) < THRESHOLD
            state["dots"][e, k] = tcp[e, :2]
            state["dot_near"][e, k] = 1 if close.any() else 0
            state["ref_hit"][e] |= close
        else:
            state["dots"][e, k] = 0.0
            state["dot_near"][e, k] = -1
        state["draw_step"][e] = k + 1
    return state


def success(state):
    """[N] bool, per env"""
    return np.array([bool(np.all(state["dot_near"][e][state["dot_near"][e] > -1])) and bool(state["ref_hit"][e].all()) for e in range(len(state["draw_step"]))])


def margins(tcp, triangles):
    """how far a step's input is from either decision: (tcp.z - Z_THRESH, min distance to a reference point - THRESHOLD) per env"""
    tcp, triangles = np.asarray(tcp, dtype=np.float64), np.asarray(triangles, dtype=np.float64)
    d = np.hypot(triangles[..., 0] - tcp[:, None, 0], triangles[..., 1] - tcp[:, None, 1])
    return tcp[:, 2] - Z_THRESH, d - THRESHOLD


def batch_wide_success(dots_dist, ref_dist):
    """the reference implementation's success_check after its table update, literally: torch.all(dots_dist[mask]) over the
    WHOLE batch, and torch.all(ref_dist, dim=-1) per env -> [N] bool"""
    mask = dots_dist > -1
    return np.logical_and(np.all(dots_dist[mask]), np.all(ref_dist, axis=-1))


def observation(qpos, qvel, tcp_pose, goal_pose, vertices):
    """[N, 2 n + 35] float64 in the reference's key order: qpos | qvel | tcp_pose 7 | goal_pose 7 | vertices - tcp.p 9 | goal_pos 3 | vertices 9"""
    N = len(qpos)
    v = np.asarray(vertices, dtype=np.float64).reshape(N, 3, 3)
    t = np.asarray(tcp_pose, dtype=np.float64)
    g = np.asarray(goal_pose, dtype=np.float64)
    return np.concatenate([np.asarray(qpos, np.float64), np.asarray(qvel, np.float64), t, g, (v - t[:, None, :3]).reshape(N, 9), g[:, :3], v.reshape(N, 9)], 1)
