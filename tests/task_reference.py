"""Float64 statement of the five task epilogues (PickCube, PushCube, PegInsertionSide, StackCube, PushT): plain numpy,
written from what the task classes (envs/tasks/tabletop/*.py) and Panda.is_grasping / is_static state, independent of
both the torch path and the HIP kernels. Test infrastructure only.

Every function takes a *snapshot* `S` of what the epilogue reads, as float32 arrays converted to float64 here (so input
rounding is not part of any difference), and a dict `P` of task parameters:

  S["rigid"]  [R, N, 13]   rigid_body_data rows: p3, q4 (wxyz), linear velocity 3, angular velocity 3
  S["qpos"], S["qvel"]  [N, n_dof]
  S["imp"]    [n_pair, N, 3]  the last substep's impulse of every shape pair, on shape A (include/mssim.h)
  S["cnt"]    [n_pair, N]     contact count of the pair
  S["pair_shape"] [n_pair, 2], S["shape_row"] [n_shape], S["dt"]

and returns a dict:
  obs [N, D] f64, exact [D] bool (columns that are copies or one subtraction: asserted bit for bit after rounding to f32),
  reward [N] f64, flags {name: bool [N]}, decided {name: bool [N]}, margins {predicate: (margin [N], band [N])},
  reward_decided [N] (every flag the reward reads is decided).

A predicate `x <= t` has margin t - x and is undecided inside its band 8 * 2^-24 * (|x| + |t|): eight float32 unit
roundoffs of the two sides, the room a float32 evaluation of x may legitimately use. Compound flags are carried as
(lowest possible, highest possible) value pairs; a flag is decided where the two agree.
"""
import numpy as np

U = 2.0 ** -24  # float32 unit roundoff
BAND = 8 * U


# ---------------------------------------------------------------------------------------------------------------------
# three-valued predicates
class Tri:
    """a boolean per env known up to its band: lo = certainly true, hi = possibly true"""

    def __init__(self, lo, hi):
        self.lo, self.hi = np.asarray(lo, bool), np.asarray(hi, bool)

    def __and__(self, o):
        return Tri(self.lo & o.lo, self.hi & o.hi)

    def __invert__(self):
        return Tri(~self.hi, ~self.lo)

    @property
    def decided(self):
        return self.lo == self.hi

    @property
    def value(self):
        return self.hi  # (what exact arithmetic gives: set by the constructors below)


def _pred(margins, name, x, t, op):
    """x op t with op in '<=', '<', '>='; records the signed margin (positive = true) and the band"""
    x, t = np.asarray(x, np.float64), np.broadcast_to(np.asarray(t, np.float64), np.shape(x))
    m = (x - t) if op == ">=" else (t - x)
    band = BAND * (np.abs(x) + np.abs(t))
    margins[name] = (m, band)
    exact = (m > 0) if op == "<" else (m >= 0)
    und = np.abs(m) <= band
    tri = Tri(exact & ~und, exact | und)
    tri._exact = exact
    return tri


def _val(tri):
    return getattr(tri, "_exact", tri.hi)


def _and(a, b):
    r = a & b
    r._exact = _val(a) & _val(b)
    return r


def _not(a):
    r = ~a
    r._exact = ~_val(a)
    return r


# ---------------------------------------------------------------------------------------------------------------------
def _f64(S):
    return {k: (np.asarray(v, np.float64) if k in ("rigid", "qpos", "qvel", "imp") else v) for k, v in S.items()}


def _norm(v):
    return np.sqrt((v * v).sum(-1))


def finger_forces(S, obj_row, f1_row, f2_row):
    """force on each finger from the object during the last substep [N, 3] x 2: the raw per-pair impulses (on shape A)
    summed over the pairs whose two shapes belong to (finger, object), negated where the finger is shape B, over dt"""
    ps, sr = np.asarray(S["pair_shape"]).reshape(-1, 2), np.asarray(S["shape_row"])
    N = S["imp"].shape[1]
    out = {f1_row: np.zeros((N, 3)), f2_row: np.zeros((N, 3))}
    for p in range(len(ps)):
        ra, rb = int(sr[ps[p, 0]]), int(sr[ps[p, 1]])
        for fr in (f1_row, f2_row):
            if (ra, rb) == (fr, obj_row):
                sign = 1.0
            elif (ra, rb) == (obj_row, fr):
                sign = -1.0
            else:
                continue
            live = (np.asarray(S["cnt"])[p] > 0)[:, None]
            out[fr] = out[fr] + sign * np.where(live, S["imp"][p], 0.0)
    dt = float(S["dt"])
    return out[f1_row] / dt, out[f2_row] / dt


def _y_axis(q):
    q = q / _norm(q)[:, None]
    w, x, y, z = q.T
    return np.stack([2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x)], -1)


def _angle_deg(a, b):
    na, nb = _norm(a), _norm(b)
    a = a / np.where(na < 1e-6, 1.0, na)[:, None]
    b = b / np.where(nb < 1e-6, 1.0, nb)[:, None]
    return np.degrees(np.arccos(np.clip((a * b).sum(-1), -1.0, 1.0)))


def grasp(S, margins, obj_row, f1_row, f2_row, min_force, max_angle_deg):
    """Panda.is_grasping: each finger is pressed with >= min_force within max_angle of its closing axis (+y of the left
    finger's frame, -y of the right one's)"""
    lf, rf = finger_forces(S, obj_row, f1_row, f2_row)
    ldir, rdir = _y_axis(S["rigid"][f1_row][:, 3:7]), -_y_axis(S["rigid"][f2_row][:, 3:7])
    lflag = _and(_pred(margins, "left_force", _norm(lf), min_force, ">="), _pred(margins, "left_angle", _angle_deg(ldir, lf), max_angle_deg, "<="))
    rflag = _and(_pred(margins, "right_force", _norm(rf), min_force, ">="), _pred(margins, "right_angle", _angle_deg(rdir, rf), max_angle_deg, "<="))
    return _and(lflag, rflag), lflag, rflag, (_norm(lf), _norm(rf))


def _finish(obs, exact, reward, flags, margins, reads, extra=None):
    out = dict(obs=obs, exact=exact, reward=reward, margins=margins, flags={k: _val(v) for k, v in flags.items()},
               decided={k: v.decided for k, v in flags.items()})
    out["reward_decided"] = np.logical_and.reduce([flags[k].decided for k in reads]) if reads else np.ones(len(reward), bool)
    out.update(extra or {})
    return out


def _cols(D, spans):
    e = np.zeros(D, bool)
    for a, b in spans:
        e[a:b] = True
    return e


def time_limit(elapsed, limit):
    """(new elapsed_steps, truncated): the counter advances by one; truncated = new >= limit"""
    new = np.asarray(elapsed, np.int64) + 1
    return new, new >= int(limit)


# ---------------------------------------------------------------------------------------------------------------------
def pick(S, P):
    """PickCube: placed = |goal - obj| <= goal_thresh; robot static = max |qvel[:n_static]| <= static_thresh;
    success = placed & static. Reward: reach (1 - tanh 5 d_tcp); grasped: + 1 + (1 - tanh 5 d_goal);
    placed: + 1 - tanh(5 |qvel[:n_static]|); success: 5. Times reward_scale."""
    S = _f64(S)
    R, qpos, qvel = S["rigid"], S["qpos"], S["qvel"]
    n = qpos.shape[1]
    tcp, obj, goal = R[P["tcp_row"]], R[P["obj_row"]], R[P["goal_row"]]
    m = {}
    grasped, lflag, rflag, forces = grasp(S, m, P["obj_row"], P["finger1_row"], P["finger2_row"], P["min_force"], P["max_angle_deg"])
    d_goal = _norm(goal[:, :3] - obj[:, :3])
    placed = _pred(m, "placed", d_goal, P["goal_thresh"], "<=")
    qs = qvel[:, : P["n_static_dofs"]]
    static = _pred(m, "static", np.abs(qs).max(1), P["static_thresh"], "<=")
    success = _and(placed, static)
    obs = np.concatenate([qpos, qvel, _val(grasped)[:, None].astype(np.float64), tcp[:, :7], goal[:, :3], obj[:, :7],
                          obj[:, :3] - tcp[:, :3], goal[:, :3] - obj[:, :3]], 1)
    r = 1 - np.tanh(5 * _norm(obj[:, :3] - tcp[:, :3]))
    r = r + np.where(_val(grasped), 1 + (1 - np.tanh(5 * d_goal)), 0.0)
    r = r + np.where(_val(placed), 1 - np.tanh(5 * _norm(qs)), 0.0)
    r = np.where(_val(success), 5.0, r) * P["reward_scale"]
    flags = dict(success=success, is_obj_placed=placed, is_robot_static=static, is_grasped=grasped, left=lflag, right=rflag)
    return _finish(obs, np.ones(obs.shape[1], bool), r, flags, m, ("success", "is_obj_placed", "is_grasped"), dict(forces=forces))


def push(S, P):
    """PushCube: success = |obj - goal|_xy < goal_radius and obj_z < half + 5 mm. Reward: 1 - tanh 5 d with d the
    distance of the tcp to the push pose (obj - (half + 5 mm) x); d < 0.01: + 1 - tanh 5 |obj - goal|_xy; success: 3."""
    S = _f64(S)
    R, qpos, qvel = S["rigid"], S["qpos"], S["qvel"]
    tcp, obj, goal = R[P["tcp_row"]], R[P["obj_row"]], R[P["goal_row"]]
    m = {}
    half = float(P["cube_half_size"])
    d_xy = _norm(obj[:, :2] - goal[:, :2])
    inside = _pred(m, "inside", d_xy, P["goal_radius"], "<")
    low = _pred(m, "low", obj[:, 2], half + 5e-3, "<")
    success = _and(inside, low)
    push_p = obj[:, :3] + np.array([-half - 0.005, 0.0, 0.0])
    dist = _norm(push_p - tcp[:, :3])
    reached = _pred(m, "reached", dist, 0.01, "<")
    obs = np.concatenate([qpos, qvel, tcp[:, :7], goal[:, :3], obj[:, :7]], 1)
    r = 1 - np.tanh(5 * dist) + np.where(_val(reached), 1 - np.tanh(5 * d_xy), 0.0)
    r = np.where(_val(success), 3.0, r) * P["reward_scale"]
    return _finish(obs, np.ones(obs.shape[1], bool), r, dict(success=success, inside=inside, low=low, reached=reached), m, ("success", "reached"))


# ---- the Python Pose class' algebra: no renormalisation, product standardised to w >= 0 ----
def _qmul(a, b):
    aw, ax, ay, az = a.T
    bw, bx, by, bz = b.T
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def _qapply(q, p):
    v = q[:, 1:]
    t = 2 * np.cross(v, p)
    return p + q[:, :1] * t + np.cross(v, t)


def pose_mul(a, b):
    q = _qmul(a[1], b[1])
    q = np.where(q[:, :1] < 0, -q, q)
    return a[0] + _qapply(a[1], b[0]), q


def pose_inv(a):
    qc = a[1] * np.array([1.0, -1.0, -1.0, -1.0])
    return _qapply(qc, -a[0]), qc


def peg(S, P):
    """PegInsertionSide: head = peg * (half_x, 0, 0); hole = box * hole_offset; success = head_in_hole.x >= -0.015 and
    |y|, |z| <= hole radius. Reward: 1 - tanh 4 |tcp - peg * (-0.06, 0, 0)|; grasped (max angle of the struct): + 1 +
    3 (1 - tanh(0.5 (h + b) + 4.5 max(h, b))) with h, b the yz distances of head and centre in the goal frame
    (goal = hole * (-half_x, 0, 0)); grasped and h, b < 0.01: + 5 (1 - tanh 5 |head_in_hole|); success: 10."""
    S = _f64(S)
    R, qpos, qvel = S["rigid"], S["qpos"], S["qvel"]
    N = qpos.shape[0]
    hs, hoff, rad = (np.asarray(P[k], np.float64) for k in ("peg_half_sizes", "box_hole_offsets", "box_hole_radii"))
    tcp, pg, bx = R[P["tcp_row"]], R[P["peg_row"]], R[P["box_row"]]
    ident = np.tile([1.0, 0, 0, 0], (N, 1))
    off = lambda x: (np.stack([x, 0 * x, 0 * x], -1), ident)
    Ppeg, Pbox = (pg[:, :3], pg[:, 3:7]), (bx[:, :3], bx[:, 3:7])
    head = pose_mul(Ppeg, off(hs[:, 0]))
    hole = pose_mul(Pbox, (hoff, ident))
    hah = pose_mul(pose_inv(hole), head)[0]
    m = {}
    deep = _pred(m, "deep", hah[:, 0], -0.015, ">=")
    in_y = _pred(m, "in_y", np.abs(hah[:, 1]), rad, "<=")
    in_z = _pred(m, "in_z", np.abs(hah[:, 2]), rad, "<=")
    success = _and(_and(deep, in_y), in_z)
    grasped, lflag, rflag, forces = grasp(S, m, P["peg_row"], P["finger1_row"], P["finger2_row"], P["min_force"], P["max_angle_deg"])
    obs = np.concatenate([qpos, qvel, tcp[:, :7], pg[:, :7], hs, hole[0], hole[1], rad[:, None]], 1)
    n = qpos.shape[1]
    exact = np.ones(obs.shape[1], bool)
    exact[2 * n + 17 : 2 * n + 24] = False  # the hole pose is computed
    grasp_target = pose_mul(Ppeg, off(np.full(N, -0.06)))[0]
    r = 1 - np.tanh(4 * _norm(tcp[:, :3] - grasp_target))
    goal_inv = pose_inv(pose_mul(hole, off(-hs[:, 0])))
    hg, bg = pose_mul(goal_inv, head)[0], pose_mul(goal_inv, Ppeg)[0]
    head_yz, body_yz = _norm(hg[:, 1:]), _norm(bg[:, 1:])
    head_al = _pred(m, "head_aligned", head_yz, 0.01, "<")
    body_al = _pred(m, "body_aligned", body_yz, 0.01, "<")
    g = _val(grasped)
    r = r + np.where(g, 1 + 3 * (1 - np.tanh(0.5 * (head_yz + body_yz) + 4.5 * np.maximum(head_yz, body_yz))), 0.0)
    r = r + np.where(g & _val(head_al) & _val(body_al), 5 * (1 - np.tanh(5 * _norm(hah))), 0.0)
    r = np.where(_val(success), 10.0, r) * P["reward_scale"]
    # (ungrasped: the alignment tiers are not read)
    aligned = _and(head_al, body_al)
    reads_al = Tri(aligned.lo | ~grasped.hi, aligned.hi | ~grasped.hi)
    reads_al._exact = _val(aligned)
    flags = dict(success=success, deep=deep, in_y=in_y, in_z=in_z, is_grasped=grasped, left=lflag, right=rflag, head_aligned=head_al,
                 body_aligned=body_al, aligned_if_grasped=reads_al)
    return _finish(obs, exact, r, flags, m, ("success", "is_grasped", "aligned_if_grasped"), dict(head_at_hole=hah, forces=forces))


def stack(S, P):
    """StackCube: on = |A - B|_xy <= on_xy_thresh and | (A - B)_z - 2 half | <= on_z_thresh; static = |v_A| <= lin and
    |w_A| <= ang; success = on & static & ~grasped. Reward: 2 (1 - tanh 5 |tcp - A|); grasped: 4 + (1 - tanh 5 |B + 2 half
    z - A|); on: 6 + (ungrasp + 1 - tanh(10 |v| + |w|)) / 2 with ungrasp = (sum of the two finger joints) / gripper
    width if grasped, else 1; success: 8."""
    S = _f64(S)
    R, qpos, qvel = S["rigid"], S["qpos"], S["qvel"]
    tcp, A, B = R[P["tcp_row"]], R[P["cubeA_row"]], R[P["cubeB_row"]]
    m = {}
    grasped, lflag, rflag, forces = grasp(S, m, P["cubeA_row"], P["finger1_row"], P["finger2_row"], P["min_force"], P["max_angle_deg"])
    half = float(P["cube_half_size"])
    off = A[:, :3] - B[:, :3]
    on_xy = _pred(m, "on_xy", _norm(off[:, :2]), P["on_xy_thresh"], "<=")
    on_z = _pred(m, "on_z", np.abs(off[:, 2] - 2 * half), P["on_z_thresh"], "<=")
    # (the z predicate subtracts two lengths of 2 half: its band is that of the operands)
    m["on_z"] = (m["on_z"][0], BAND * (np.abs(off[:, 2]) + 2 * half + P["on_z_thresh"]))
    und = np.abs(m["on_z"][0]) <= m["on_z"][1]
    ex = _val(on_z)
    on_z = Tri(ex & ~und, ex | und)
    on_z._exact = ex
    on = _and(on_xy, on_z)
    v, av = _norm(A[:, 7:10]), _norm(A[:, 10:13])
    lin = _pred(m, "static_lin", v, P["static_lin_thresh"], "<=")
    ang = _pred(m, "static_ang", av, P["static_ang_thresh"], "<=")
    static = _and(lin, ang)
    success = _and(_and(on, static), _not(grasped))
    p_t, p_a, p_b = tcp[:, :3], A[:, :3], B[:, :3]
    obs = np.concatenate([qpos, qvel, tcp[:, :7], A[:, :7], B[:, :7], p_a - p_t, p_b - p_t, p_b - p_a], 1)
    g = _val(grasped)
    r = 2 * (1 - np.tanh(5 * _norm(p_t - p_a)))
    goal = p_b + np.array([0.0, 0.0, 2 * half])
    r = np.where(g, 4 + (1 - np.tanh(5 * _norm(goal - p_a))), r)
    ungrasp = np.where(g, (qpos[:, -2] + qpos[:, -1]) / P["gripper_width"], 1.0)
    r = np.where(_val(on), 6 + (ungrasp + (1 - np.tanh(10 * v + av))) / 2, r)
    r = np.where(_val(success), 8.0, r) * P["reward_scale"]
    flags = dict(success=success, is_cubeA_on_cubeB=on, is_cubeA_static=static, is_cubeA_grasped=grasped, left=lflag, right=rflag,
                 static_lin=lin, static_ang=ang)
    return _finish(obs, np.ones(obs.shape[1], bool), r, flags, m, ("success", "is_cubeA_on_cubeB", "is_cubeA_grasped"),
                   dict(forces=forces, gripper_width=float(P["gripper_width"]), velocity=A[:, 7:13]))


# ---------------------------------------------------------------------------------------------------------------------
PUSHT_SCALE = 64 / 2 / 0.15  # pixels per metre
PUSHT_LEVER = 0.14           # m, the template pixel farthest from the T's frame (end of the stem: (0.025, 0.1375))


def pusht_eps(px, py, w2g, coord=64.0):
    """Bound (pixels) on the float32 error of one image coordinate of the pseudo-render, against exact arithmetic on the
    same float32 inputs, for the chain  acosf -> cosf / sinf -> 3 x 3 product -> two FMAs -> divide -> scale + 32.
    With u = 2^-24:
      * yaw = 2 acosf(+-q_w): acosf within 2 ulp of a value in [0, pi], ulp <= 2^-22, the doubling exact:
        d_yaw <= 2 * 2 * 2^-22 = 9.6e-7 rad. A rotation error moves a pixel at distance <= 0.14 m (LEVER) from the T's
        frame by <= 0.14 d_yaw = 1.34e-7 m, whatever the orthogonal world-to-goal rotation that follows.
      * cosf / sinf themselves within 2 ulp of a value <= 1 (2^-23 each), times the goal rotation's row (|W0| + |W1| <=
        sqrt 2), plus the two roundings of the product row (2 u): the matrix entries T0, T1 carry <= sqrt 2 * 2^-23 + 2 u
        = 2.9e-7 beyond the rotation error; times |u| + |v| <= 0.14 sqrt 2 = 0.2 m: 5.8e-8 m.
      * translation column W0 px + W1 py + W2: three roundings of a value bounded by t = |W0 px| + |W1 py| + |W2|:
        3 u t (1.3e-7 m for t = 0.7 m).
      * the two FMAs and the sum h = T0 u + T1 v + T2: 3 u (|h| + 0.2) with |h| <= coord / SCALE (0.3 m at 64 px).
      * the third row of both matrices is (0, 0, 1) exactly: the divisor is 1 and the division exact.
      * times SCALE (its own float32 rounding u, the product's u: 2 u * 32 px = 3.8e-6 px), plus 32 (half an ulp of a
        value below 64: 2^-19 = 1.9e-6 px; of 2^k * 64: scaled with the coordinate).
    About 8e-5 px for a tee inside the image, a few 1e-5 more per metre of |p|. Callers use twice this bound."""
    w2g = np.asarray(w2g, np.float64).reshape(3, 3)
    t = np.maximum(np.abs(w2g[0, 0] * px) + np.abs(w2g[0, 1] * py) + np.abs(w2g[0, 2]),
                   np.abs(w2g[1, 0] * px) + np.abs(w2g[1, 1] * py) + np.abs(w2g[1, 2]))
    c = np.maximum(coord, 64.0)
    metres = PUSHT_LEVER * (8 * 2.0 ** -23) + 0.2 * (np.sqrt(2) * 2.0 ** -23 + 2 * U) + 3 * U * t + 3 * U * (c / PUSHT_SCALE + 0.2)
    return metres * PUSHT_SCALE + 2 * U * c + 2.0 ** -19 * (c / 64.0)


def pusht_count(tee, consts):
    """the pseudo-render's intersection count as an interval. tee [N, 13] rows; consts: dict(w2g [9], u [64], v [64],
    template [64, 64] bool). Every template pixel (i, j), at (u[j], v[i], 1), goes through world_to_goal @ tee_to_world,
    is scaled to pixels (+ 32) and truncated toward zero; an index outside [0, 64) sends it to (0, 0); index (x, y)
    lands on image row 63 - y, column x. Returns (count_min, count_max, undecided pixels [N])."""
    tee = np.asarray(tee, np.float64)
    N = tee.shape[0]
    W = np.asarray(consts["w2g"], np.float64).reshape(3, 3)
    tmpl = np.asarray(consts["template"], bool)
    ii, jj = np.nonzero(tmpl)
    uvec = np.stack([np.asarray(consts["u"], np.float64)[jj], np.asarray(consts["v"], np.float64)[ii], np.ones(len(ii))])  # [3, n]
    qw, qz = tee[:, 3], tee[:, 6]
    with np.errstate(invalid="ignore"):
        yaw = 2 * np.arccos(np.where(qz < 0, -qw, qw))
    cmin, cmax, nund = np.zeros(N, int), np.zeros(N, int), np.zeros(N, int)
    for e in range(N):
        T = np.eye(3)
        T[0, 0] = T[1, 1] = np.cos(yaw[e])
        T[0, 1], T[1, 0] = -np.sin(yaw[e]), np.sin(yaw[e])
        T[0, 2], T[1, 2] = tee[e, 0], tee[e, 1]
        h = W @ T @ uvec
        c = h[:2] / h[2] * PUSHT_SCALE + 32.0  # [2, n] image coordinates (x, y)
        if not np.all(np.isfinite(c)):
            continue  # (NaN compares false everywhere: every pixel goes to (0, 0))
        eps = 2 * pusht_eps(tee[e, 0], tee[e, 1], W, np.abs(c))
        lo, hi = np.trunc(c - eps), np.trunc(c + eps)  # truncation toward zero: (-1, 0) -> 0
        und = (lo != hi).any(0)
        nund[e] = und.sum()
        sure = np.zeros((64, 64), bool)
        maybe = np.zeros((64, 64), bool)
        for xs, ys, dst, sel in ((lo[0], lo[1], sure, ~und), (lo[0], lo[1], maybe, und), (lo[0], hi[1], maybe, und),
                                 (hi[0], lo[1], maybe, und), (hi[0], hi[1], maybe, und)):
            ok = sel & (xs >= 0) & (xs < 64) & (ys >= 0) & (ys < 64)
            dst[63 - ys[ok].astype(int), xs[ok].astype(int)] = True
        cmin[e] = (sure & tmpl).sum()
        cmax[e] = ((sure | maybe) & tmpl).sum()
    return cmin, cmax, nund


def pusht(S, P):
    """PushT: success = count / area >= intersection_thresh. Reward: ((cos(yaw - goal_z_rot) + 1) / 2)^2 / 2 +
    (1 - tanh 5 |tee - goal|_xy)^2 / 2 + sqrt(1 - tanh 5 |tee - tcp|) / 20; success: 3; divided by reward_div."""
    S = _f64(S)
    R, qpos, qvel = S["rigid"], S["qpos"], S["qvel"]
    tcp, tee, goal = R[P["tcp_row"]], R[P["tee_row"]], R[P["goal_row"]]
    cmin, cmax, nund = pusht_count(tee, P["consts"])
    area = int(np.asarray(P["consts"]["template"], bool).sum())
    m = {}
    s_lo = _pred(m, "covered_min", cmin / area, P["intersection_thresh"], ">=")
    s_hi = _pred(m, "covered_max", cmax / area, P["intersection_thresh"], ">=")
    success = Tri(s_lo.lo & s_hi.lo, s_lo.hi | s_hi.hi)
    success._exact = _val(s_lo)
    qw, qz = tee[:, 3], tee[:, 6]
    with np.errstate(invalid="ignore"):
        yaw = 2 * np.arccos(np.where(qz < 0, -qw, qw))
        rot = (np.cos(yaw - P["goal_z_rot"]) + 1) / 2
    r = rot ** 2 / 2 + (1 - np.tanh(5 * _norm(tee[:, :2] - goal[:, :2]))) ** 2 / 2
    r = r + np.sqrt(1 - np.tanh(5 * _norm(tee[:, :3] - tcp[:, :3]))) / 20
    r = np.where(_val(success), 3.0, r) / P["reward_div"]
    obs = np.concatenate([qpos, qvel, tcp[:, :7], goal[:, :3], tee[:, :7]], 1)
    return _finish(obs, np.ones(obs.shape[1], bool), r, dict(success=success), m, ("success",),
                   dict(count_min=cmin, count_max=cmax, undecided_pixels=nund, area=area, template=np.asarray(P["consts"]["template"], bool)))


TASKS = dict(pick=pick, push=push, peg=peg, stack=stack, pusht=pusht)
