"""A numpy float64 reference for the narrowphase manifolds (maniskill_amd/csrc/mssim_collide.h, the 16-lane routines of
mssim_solve16.h), written from the geometry and from the conventions stated in those headers and in include/mssim.h --
not from the kernels, and sharing no code with the oracle (oracle/oracle_collide.hpp).

What it knows:
  * the support VALUE h_S(d) = max_{x in S} d.x of a box, sphere, capsule, cylinder and hull (scalar closed forms: no
    support points, no case split by sign), and from it the directional gap g(n) = min_{a in A} n.a - max_{b in B} n.b
    and the mid plane between the two support planes
  * exact signed distances: sphere-sphere, sphere-capsule, capsule-capsule (non-parallel), sphere outside a box; the
    box-box gap as the best of the 15 separating axes
  * plane manifolds in closed form (plane normal = column 0 of the plane's frame, n = -normal, x = mid point, sep = gap)
  * a box-box manifold CHECKER that does not redo the clipping: it measures how far a manifold is from "normal = a best
    face axis, every point on the mid surface of the two faces and inside their overlap polygon, min(sep) = the lowest
    point of that polygon" -- the polygon being the intersection of 8 half planes, its vertices found by brute force

Contact convention: n points from shape B to shape A, sep = signed gap, x = mid point between the two surfaces.
A shape is a `Shape` built from exactly the float32 numbers the code under test is given.
"""
import itertools

import numpy as np

PLANE, BOX, SPHERE, CAPSULE, CYLINDER, CONVEX = range(6)
# include/mssim.h (float literals there: the value is the float32 one)
PATCH_SLACK = float(np.float32(4e-3))
PATCH_TIE_SEP = float(np.float32(1e-5))
PATCH_TIE_REL = float(np.float32(1e-3))
EDGE_AXIS_MIN_SQ = 1e-6  # a cross-product axis |a_i x b_j|^2 below this is skipped (parallel edges)
EDGE_OVER_FACE = 1e-3    # an edge axis is taken only when it beats the best face axis by this much
REF_FACE_TIE = 1e-5      # face of A is the reference face unless B's is better by more than this
SAT_GUARD = 1e-6         # added to every |a_i . b_j| of the axis search


class Shape:
    def __init__(self, type_, pose7, param, verts=None):
        self.type = int(type_)
        pose7 = np.asarray(pose7, dtype=np.float64)
        self.p = pose7[:3].copy()
        q = pose7[3:7] / np.sqrt(np.sum(pose7[3:7] ** 2))
        w, x, y, z = q
        self.R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                           [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                           [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        self.prm = np.asarray(param, dtype=np.float64)
        self.verts = None if verts is None else np.asarray(verts, dtype=np.float64).reshape(-1, 3)

    def world_verts(self):
        return self.p + self.verts @ self.R.T


def support_value(s, d):
    """h_S(d) = max over the shape of d . x"""
    d = np.asarray(d, dtype=np.float64)
    dl = s.R.T @ d
    base = float(d @ s.p)
    if s.type == BOX:
        return base + float(np.abs(dl) @ s.prm[:3])
    if s.type == SPHERE:
        return base + s.prm[0] * float(np.linalg.norm(dl))
    if s.type == CAPSULE:
        return base + s.prm[1] * abs(dl[0]) + s.prm[0] * float(np.linalg.norm(dl))
    if s.type == CYLINDER:
        return base + s.prm[1] * abs(dl[0]) + s.prm[0] * float(np.hypot(dl[1], dl[2]))
    if s.type == CONVEX:
        return base + float(np.max(s.verts @ dl))
    raise ValueError("no support value for shape type %d" % s.type)


def gap(A, B, n):
    """g(n): the gap between the support plane of A facing B and that of B facing A, n from B to A"""
    n = np.asarray(n, dtype=np.float64)
    return -support_value(A, -n) - support_value(B, n)


def mid_plane(A, B, n):
    """offset along n of the plane midway between the two support planes"""
    n = np.asarray(n, dtype=np.float64)
    return 0.5 * (-support_value(A, -n) + support_value(B, n))


# ------------------------------------------------------------------------------------------ exact distances
def _segment(s):
    ax = s.R[:, 0] * s.prm[1]
    return s.p - ax, s.p + ax


def point_segment_distance(p, a, b):
    ab = b - a
    t = np.clip(np.dot(p - a, ab) / np.dot(ab, ab), 0.0, 1.0)
    return float(np.linalg.norm(p - (a + t * ab)))


def segment_segment_distance(p1, q1, p2, q2):
    """two non-degenerate, non-parallel segments: the minimum is at an interior critical point or at an end point"""
    best = min(point_segment_distance(p1, p2, q2), point_segment_distance(q1, p2, q2),
               point_segment_distance(p2, p1, q1), point_segment_distance(q2, p1, q1))
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, b = d1 @ d1, d2 @ d2, d1 @ d2
    den = a * e - b * b
    if den > 1e-12 * a * e:
        s = (b * (d2 @ r) - (d1 @ r) * e) / den
        t = (a * (d2 @ r) - b * (d1 @ r)) / den
        if 0.0 <= s <= 1.0 and 0.0 <= t <= 1.0:
            best = min(best, float(np.linalg.norm(r + s * d1 - t * d2)))
    return best


def point_box_distance(p, box):
    """distance of a point OUTSIDE the box to it (None when inside)"""
    l = box.R.T @ (p - box.p)
    ex = np.maximum(np.abs(l) - box.prm[:3], 0.0)
    d = float(np.linalg.norm(ex))
    return d if d > 0.0 else None


def exact_distance(A, B):
    """signed distance of the pair where a closed form exists, else None"""
    t = (A.type, B.type)
    if t == (SPHERE, SPHERE):
        return float(np.linalg.norm(A.p - B.p)) - A.prm[0] - B.prm[0]
    if t in ((SPHERE, CAPSULE), (CAPSULE, SPHERE)):
        S, C = (A, B) if A.type == SPHERE else (B, A)
        return point_segment_distance(S.p, *_segment(C)) - S.prm[0] - C.prm[0]
    if t == (CAPSULE, CAPSULE):
        if np.linalg.norm(np.cross(A.R[:, 0], B.R[:, 0])) < 1e-3:
            return None
        return segment_segment_distance(*_segment(A), *_segment(B)) - A.prm[0] - B.prm[0]
    if t in ((SPHERE, BOX), (BOX, SPHERE)):
        S, X = (A, B) if A.type == SPHERE else (B, A)
        d = point_box_distance(S.p, X)
        return None if d is None else d - S.prm[0]
    return None


# ------------------------------------------------------------------------------------------ plane manifolds
def _deepest4(pts, seps):
    order = sorted(range(len(seps)), key=lambda i: (seps[i], i))[:4]
    return [pts[i] for i in order], [seps[i] for i in order]


def _extent4(pts, seps, nrm):
    """include/mssim.h, contact patches: the deepest, the farthest from it, the largest area on either side of that edge;
    every scan takes the first candidate within the tie tolerance of its extremum"""
    n = len(seps)
    smin = min(seps)
    cand = [i for i in range(n) if seps[i] <= smin + PATCH_SLACK]
    i0 = next(i for i in cand if seps[i] <= smin + PATCH_TIE_SEP)
    rest = [i for i in cand if i != i0]
    d2 = {i: float(np.sum((pts[i] - pts[i0]) ** 2)) for i in rest}
    mx = max(d2.values())
    i1 = next(i for i in rest if d2[i] >= mx - PATCH_TIE_REL * mx)
    e = pts[i1] - pts[i0]
    rest = [i for i in rest if i != i1]
    ar = {i: float(np.cross(e, pts[i] - pts[i0]) @ nrm) for i in rest}
    mx = max(abs(v) for v in ar.values())
    i2 = next(i for i in rest if abs(ar[i]) >= mx - PATCH_TIE_REL * mx)
    pick = [i0, i1, i2]
    rest = [i for i in rest if i != i2]
    other = {i: (-ar[i] if ar[i2] >= 0 else ar[i]) for i in rest}
    mx = max(other.values()) if other else 0.0
    if mx > PATCH_TIE_REL * abs(ar[i2]):
        pick.append(next(i for i in rest if other[i] >= mx - PATCH_TIE_REL * mx))
    return [pts[i] for i in pick], [seps[i] for i in pick]


def plane_manifold(P, B, offset):
    """(count, n, [count][4] x y z sep) of a plane P against B"""
    npl = P.R[:, 0]
    pts, seps = [], []
    by_extent = False

    def add(p, radius):
        s = float(npl @ (p - P.p)) - radius
        if s < offset:
            pts.append(p - npl * (radius + 0.5 * s))
            seps.append(s)

    if B.type == BOX:
        for i in range(8):
            l = np.array([B.prm[0] if i & 1 else -B.prm[0], B.prm[1] if i & 2 else -B.prm[1], B.prm[2] if i & 4 else -B.prm[2]])
            add(B.p + B.R @ l, 0.0)
    elif B.type == SPHERE:
        add(B.p, B.prm[0])
    elif B.type == CAPSULE:
        a, b = _segment(B)
        add(a, B.prm[0])
        add(b, B.prm[0])
    elif B.type == CYLINDER:
        ax = B.R[:, 0]
        side = npl - (npl @ ax) * ax
        ls = float(np.linalg.norm(side))
        # the lowest rim point; flat on its face (no lowest rim point): the centre of the face
        p = B.p - np.sign(npl @ ax) * B.prm[1] * ax
        if ls > 1e-12:
            p = p - B.prm[0] * side / ls
        add(p, 0.0)
    elif B.type == CONVEX:
        for v in B.world_verts()[:64]:
            add(v, 0.0)
        # a hull lying on a face (more than 4 vertices within the slack of the lowest): four by extent, not by depth
        if len(seps) > 4 and sum(s <= min(seps) + PATCH_SLACK for s in seps) > 4:
            pts, seps = _extent4(pts, seps, -npl)
            by_extent = True
    else:
        raise ValueError("plane against shape type %d" % B.type)
    if not by_extent:
        pts, seps = _deepest4(pts, seps)  # in order of depth, the lower index first among equals
    out = np.zeros((len(seps), 4))
    for k in range(len(seps)):
        out[k, :3], out[k, 3] = pts[k], seps[k]
    return len(seps), -npl, out


# ------------------------------------------------------------------------------------------ box-box
def sat_axes(A, B):
    """(faces, edges): faces = [(g, n, owner, axis index)] for the 6 face axes in both signs, edges = [(g, n, i, j)] for the
    cross-product axes that are long enough, n a unit vector from B to A and g = gap(A, B, n)"""
    faces, edges = [], []
    for owner, S in (("A", A), ("B", B)):
        for i in range(3):
            for sg in (1.0, -1.0):
                n = sg * S.R[:, i]
                faces.append((gap(A, B, n), n, owner, i))
    for i in range(3):
        for j in range(3):
            c = np.cross(A.R[:, i], B.R[:, j])
            l2 = float(c @ c)
            if l2 < EDGE_AXIS_MIN_SQ:
                continue
            for sg in (1.0, -1.0):
                n = sg * c / np.sqrt(l2)
                edges.append((gap(A, B, n), n, i, j))
    return faces, edges


def sat_gap(A, B):
    """the box-box gap by the best of the 15 axes (negative: the penetration depth along the best axis)"""
    faces, edges = sat_axes(A, B)
    return max(f[0] for f in faces + edges)


def sat_slack(A, B):
    """how much below the best face axis the chosen face axis may lie by the tie rules stated in mssim_collide.h: the
    reference-face tie plus the guard added to every |a_i . b_j| times the half extents it multiplies"""
    return REF_FACE_TIE + 2.0 * SAT_GUARD * float(np.sum(A.prm[:3]) + np.sum(B.prm[:3]))


def overlap_polygon(X, ir, a, Y, jinc, fc):
    """vertices (u, v, sep) of the incident face of Y cut to the side planes of the reference face `ir` of X: the
    intersection of 8 half planes in the incident face's own coordinates, every pair of boundary lines intersected and
    the points inside all 8 kept"""
    y1, y2 = Y.R[:, (jinc + 1) % 3], Y.R[:, (jinc + 2) % 3]
    hy1, hy2 = Y.prm[(jinc + 1) % 3], Y.prm[(jinc + 2) % 3]
    H = [((1.0, 0.0), hy1), ((-1.0, 0.0), hy1), ((0.0, 1.0), hy2), ((0.0, -1.0), hy2)]
    for k in ((ir + 1) % 3, (ir + 2) % 3):
        xk = X.R[:, k]
        c0 = float(xk @ (fc - X.p))
        cu, cv = float(xk @ y1), float(xk @ y2)
        H.append(((cu, cv), X.prm[k] - c0))
        H.append(((-cu, -cv), X.prm[k] + c0))
    scale = max(hy1, hy2, 1e-9)
    out = []
    for (n1, d1), (n2, d2) in itertools.combinations(H, 2):
        det = n1[0] * n2[1] - n1[1] * n2[0]
        if abs(det) < 1e-14:
            continue
        u = (d1 * n2[1] - d2 * n1[1]) / det
        v = (n1[0] * d2 - n2[0] * d1) / det
        if all(nn[0] * u + nn[1] * v <= dd + 1e-12 * scale for nn, dd in H):
            p = fc + u * y1 + v * y2
            out.append((u, v, float(a @ (p - X.p)) - X.prm[ir]))
    return out


def check_box_box(A, B, offset, count, n, pts):
    """Figures of merit of a box-box manifold (all lengths in metres, 0 = perfect), or raises AssertionError when the
    manifold is of the wrong kind. Keys:
      kind         'none' | 'edge' | 'face'
      unit         | |n| - 1 |
      axis         distance of n from the nearest SAT axis of its kind
      deficit      best admissible gap minus g(n), beyond the stated tie slack (<= 0 when inside it)
      depth        | min(sep) - expected | : the lowest point of the overlap polygon (face), g(n) (edge)
      surface      face: distance of a point from the mid surface of the two faces; edge: of n.x from the mid plane
      outside      face: how far a point lies outside the overlap polygon"""
    faces, edges = sat_axes(A, B)
    g_face = max(f[0] for f in faces)
    g_all = max([g_face] + [e[0] for e in edges])
    n = np.asarray(n, dtype=np.float64)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 4)[:count]
    if count == 0:
        return dict(kind="none", g_all=g_all, g_face=g_face)
    res = dict(unit=abs(float(np.linalg.norm(n)) - 1.0), g_all=g_all, g_face=g_face)
    gn = gap(A, B, n)
    d_face = min(float(np.linalg.norm(n - f[1])) for f in faces)
    d_edge = min([float(np.linalg.norm(n - e[1])) for e in edges] + [np.inf])
    if count == 1 and d_edge < d_face:
        res.update(kind="edge", axis=d_edge, deficit=g_all - gn, depth=abs(pts[0, 3] - gn),
                   surface=abs(float(n @ pts[0, :3]) - mid_plane(A, B, n)), outside=0.0)
        assert g_all > g_face + EDGE_OVER_FACE - 1e-4, "an edge contact where a face axis is as good"
        return res
    # face contact: which box owns the reference face is not known from n when faces are parallel: the better reading counts
    best = None
    for ref in ("A", "B"):
        X, Y = (A, B) if ref == "A" else (B, A)
        nref = -n if ref == "A" else n  # from X towards Y
        ir = int(np.argmax(np.abs(X.R.T @ nref)))
        a = X.R[:, ir] * np.sign(X.R[:, ir] @ nref)
        axis = float(np.linalg.norm(nref - a))
        if axis > 1e-3:
            continue
        jinc = int(np.argmax(np.abs(Y.R.T @ a)))
        ninc = -Y.R[:, jinc] * np.sign(Y.R[:, jinc] @ a)
        fc = Y.p + ninc * Y.prm[jinc]
        poly = overlap_polygon(X, ir, a, Y, jinc, fc)
        if not poly:
            continue
        y1, y2 = Y.R[:, (jinc + 1) % 3], Y.R[:, (jinc + 2) % 3]
        surface = outside = 0.0
        for x, s in zip(pts[:, :3], pts[:, 3]):
            p = x + a * (0.5 * s)  # the point of the incident face the contact stands for
            surface = max(surface, abs(float(ninc @ (p - fc))), abs(float(a @ (x - X.p)) - X.prm[ir] - 0.5 * s))
            outside = max(outside, abs(float(y1 @ (p - fc))) - Y.prm[(jinc + 1) % 3], abs(float(y2 @ (p - fc))) - Y.prm[(jinc + 2) % 3])
            for k in ((ir + 1) % 3, (ir + 2) % 3):
                outside = max(outside, abs(float(X.R[:, k] @ (p - X.p))) - X.prm[k])
        lowest = min(v[2] for v in poly)
        cand = dict(kind="face", ref=ref, axis=axis, deficit=g_face - gn - sat_slack(A, B), depth=abs(float(np.min(pts[:, 3])) - lowest),
                    surface=surface, outside=max(outside, 0.0), n_vertices=len(poly))
        score = lambda r: r["axis"] + r["depth"] + r["surface"] + r["outside"]
        if best is None or score(cand) < score(best):
            best = cand
    assert best is not None, "the normal is no face axis of either box, or the faces do not overlap"
    res.update(best)
    return res


# ------------------------------------------------------------------------------------------ single-point (MPR) manifolds
def check_point_manifold(A, B, offset, n, x, sep):
    """value checks of a one-point manifold of two convex shapes: | |n| - 1 |, | sep - g(n) |, | n.x - mid plane |, g(n)"""
    n = np.asarray(n, dtype=np.float64)
    gn = gap(A, B, n / np.linalg.norm(n))
    return dict(unit=abs(float(np.linalg.norm(n)) - 1.0), sep=abs(sep - gn), mid=abs(float(n @ np.asarray(x, dtype=np.float64)) - mid_plane(A, B, n)), g=gn)
