"""A numpy statement of the flat-shaded view (include/mssim_hip_tasks.h, "A flat-shaded view of the same scene"), written
from that definition and not from the kernel's header: which shape a ray enters first comes from the existing references
(tests/raycast_reference.py, raycast_mesh_reference.py: brute force over triangles, no BVH); this file adds the normal at
the entry point per shape type, the two lights, the checker and the rounding. Normals are carried into the ENV frame and
lit there with the light directions as the definition gives them (the kernel works in the camera frame instead). `dtype`
selects the arithmetic: float64 is the reference, float32 the same computation in the kernel's precision.

Colours are the dict of `maniskill_amd.model.compile.raycast_colours`: `shape_rgba` [S, 4] (r, g, b, checker cell size in
metres, 0 = none) and optionally `env_shape_rgba` [slots, N, 4].

`ambiguous` marks the pixels whose picture is not decided by the geometry to within a rounding: those of
raycast_mesh_reference.ambiguous (the id changes under a +-AMBIG_SHIFT sub-pixel shift, a second surface within
AMBIG_DIST, near / far), plus, under the same shifts, a change of the hit SHAPE, of the FACE, or of the checker cell.
"The face changes" reads: on a flat part (plane, box side, cylinder cap, hull face, triangle) the unit normals of the two
hits are more than FACE_TOL apart; on a curved part (sphere, cylinder side, a capsule's tube and balls), where the normal
moves with the ray, the part is another one.
"""
import numpy as np

from tests import raycast_mesh_reference as rmr
from tests import raycast_reference as rr

AMBIENT = 0.3
LIGHTS = (np.array([1.0, 1.0, -1.0]) / np.sqrt(3.0), np.array([0.0, 0.0, -1.0]))  # env frame, the way the light travels
CHECKER_DIM = 0.8
BACKGROUND = (44, 52, 66)
FACE_TOL = 1e-3
FLAT = -1  # `part` of a flat face; curved parts count from 0


def shape_in_env(scene, i, N, env):
    """(type, param[:3], (first plane, count)) of shape i as env `env` has it"""
    type_, param = int(scene["shape_type"][i]), np.asarray(scene["shape_param"][i][:3])
    planes2 = tuple(int(x) for x in np.asarray(scene["shape_planes"]).reshape(-1, 2)[i])
    n_es = int(scene.get("n_env_shape", 0))
    slot = int(scene["shape_env_slot"][i]) if n_es else -1
    if slot >= 0:
        ep = np.asarray(scene["env_shape_param"]).reshape(n_es, 4, N)[slot, :, env]
        if ep[3] > 0:
            type_ = int(ep[3]) - 1
        if type_ != rr.CONVEX:
            param = ep[:3]
        if scene.get("env_shape_planes") is not None and type_ == rr.CONVEX:
            planes2 = tuple(int(x) for x in np.asarray(scene["env_shape_planes"]).reshape(n_es, 2, N)[slot, :, env])
    return type_, param, planes2


def colour_in_env(scene, colours, i, N, env):
    n_es = int(scene.get("n_env_shape", 0))
    slot = int(scene["shape_env_slot"][i]) if n_es else -1
    if slot >= 0 and colours.get("env_shape_rgba") is not None:
        return np.asarray(colours["env_shape_rgba"], dtype=np.float64).reshape(n_es, N, 4)[slot, env]
    return np.asarray(colours["shape_rgba"], dtype=np.float64).reshape(-1, 4)[i]


def _unit(v):
    with np.errstate(divide="ignore", invalid="ignore"):
        return v / np.sqrt((v * v).sum(-1, keepdims=True))


def entry_normal(type_, param, planes, o, d, t, dt):
    """(n [..., 3] outward unit normal in the shape frame, part [...]) at the entry points p = o + t d of rays that enter
    the shape at t (anything where t is not finite)"""
    p = o + t[..., None] * d
    n = np.zeros(d.shape, dtype=dt)
    part = np.full(d.shape[:-1], FLAT, dtype=np.int64)
    against = np.where(d > 0, -1.0, 1.0).astype(dt)

    def slab_entries(axes, half):
        with np.errstate(divide="ignore", invalid="ignore"):
            lo = np.stack([np.minimum((-half[k] - o[k]) / d[..., k], (half[k] - o[k]) / d[..., k]) for k in axes], axis=-1)
        return np.where(np.stack([d[..., k] == 0 for k in axes], axis=-1), -np.inf, lo)

    def cylinder(o_, p_, r, h):
        """normal and part (FLAT on a cap, 0 on the side) of a cylinder about +x entered at p_ by rays from o_"""
        mask = np.array([0, 1, 1], dtype=dt)
        side_t, _ = rr._ball(o_ * mask, d * mask, r, dt)
        cap = slab_entries([0], [h])[..., 0] > side_t  # the cap slab raised the side's entry parameter
        nn = np.where(cap[..., None], np.stack([against[..., 0], 0 * t, 0 * t], axis=-1), p_ * mask / r)
        return nn.astype(dt), np.where(cap, FLAT, 0)

    if type_ == rr.PLANE:
        n[..., 0] = 1
    elif type_ == rr.BOX:
        k = np.argmax(slab_entries([0, 1, 2], param), axis=-1)  # the slab that set the entry; the lowest axis on a tie
        n = (np.eye(3, dtype=dt)[k] * against).astype(dt)
    elif type_ == rr.SPHERE:
        n, part = _unit(p), part * 0
    elif type_ == rr.CYLINDER:
        n, part = cylinder(o, p, param[0], param[1])
    elif type_ == rr.CAPSULE:
        r, h = param[0], param[1]
        tin, tout = rr._cylinder(o, d, r, h, dt)
        best = np.where(tin <= tout, tin, np.inf)
        n, part = cylinder(o, o + np.where(np.isfinite(best), best, 0)[..., None] * d, r, h)
        part = np.where(part == FLAT, 3, part)  # (a cap of the tube lies inside a ball: never the earliest but on the seam)
        for k, sx in enumerate((-1, 1)):
            c = np.array([sx * h, 0, 0], dtype=dt)
            bi, bo = rr._ball(o - c, d, r, dt)
            bi = np.where(bi <= bo, bi, np.inf)
            first = bi < best
            n = np.where(first[..., None], _unit(o - c + np.where(np.isfinite(bi), bi, 0)[..., None] * d), n)
            part, best = np.where(first, 1 + k, part), np.minimum(best, bi)
    elif type_ == rr.CONVEX:
        planes = np.asarray(planes).astype(dt)
        nd = d @ planes[:, :3].T
        dist = planes[:, 3] - planes[:, :3] @ o
        with np.errstate(divide="ignore", invalid="ignore"):
            tk = np.where(nd < 0, dist / nd, -np.inf)
        n = planes[np.argmax(tk, axis=-1), :3]  # the first plane, in index order, at the largest entry parameter
    return n.astype(dt), part


def triangle_normals(soup, tri, d, dt):
    """unit normals of triangles `tri` [...] of the soup (shape frame), turned against the rays d [..., 3]"""
    q = np.asarray(soup).astype(dt)[np.maximum(tri, 0)]
    n = _unit(np.cross(q[..., 6:9] - q[..., 3:6], q[..., 9:12] - q[..., 3:6]).astype(dt))
    return np.where(((n * d).sum(-1) > 0)[..., None], -n, n).astype(dt)


def render(scene, colours, camera, rigid, N, env, dtype=np.float64, du=0.0, dv=0.0):
    """one env's picture: dict(rgb [H, W, 3] int64; hit [H, W]; shape [H, W] (-1: nothing); part [H, W]; normal [H, W, 3]
    in the env frame; cell [H, W] checker cell parity (0 off a checkered shape); t [H, W])"""
    dt = np.dtype(dtype).type
    R = rmr.render(scene, camera, rigid, N, env, dtype, du, dv)
    H, W = R["hit"].shape
    u = (np.arange(W, dtype=dt) + dt(0.5) + dt(du) - dt(camera["cx"])) / dt(camera["fx"])
    v = (np.arange(H, dtype=dt) + dt(0.5) + dt(dv) - dt(camera["cy"])) / dt(camera["fy"])
    xcv, ycv = np.meshgrid(u, v)
    Rc, pc = rr.camera_pose(camera, rigid, N, env, dt)
    d_env = np.stack([np.ones_like(xcv), -xcv, -ycv], axis=-1) @ Rc.T
    normal = np.zeros((H, W, 3), dtype=dt)
    albedo = np.zeros((H, W, 3), dtype=dt)
    part = np.full((H, W), FLAT, dtype=np.int64)
    cell = np.zeros((H, W), dtype=np.int64)
    for i in np.unique(R["shape"][R["hit"]]):
        m = R["shape"] == i
        type_, param, (first, count) = shape_in_env(scene, i, N, env)
        Rs, ps = rmr.shape_pose(scene, i, rigid, N, env, dt)
        o, d = (Rs.T @ (pc - ps)).astype(dt), (d_env[m] @ Rs).astype(dt)
        t = R["t"][m].astype(dt)
        if type_ == rr.TRIMESH:
            n, pt = triangle_normals(scene["tri_soup"], R["tri"][m], d, dt), np.full(t.shape, FLAT)
        else:
            n, pt = entry_normal(type_, np.asarray(param, dtype=dt), np.asarray(scene["planes"])[first : first + count], o, d, t, dt)
        normal[m], part[m] = n @ Rs.T, pt
        rgba = colour_in_env(scene, colours, i, N, env).astype(dt)
        a = np.tile(rgba[:3], (len(t), 1))
        if rgba[3] > 0:
            p = o + t[:, None] * d
            if type_ == rr.PLANE:
                p[:, 0] = 0
            k = np.floor(p / rgba[3]).sum(-1).astype(np.int64)
            cell[m] = 1 + (k & 1)
            a = np.where(((k & 1) == 1)[:, None], dt(CHECKER_DIM) * a, a)
        albedo[m] = a
    lit = dt(AMBIENT) + sum(np.maximum(0, -(normal @ l.astype(dt))) for l in LIGHTS)
    c = albedo * np.minimum(1, lit)[..., None]
    rgb = np.floor(dt(255) * np.minimum(c, 1) + dt(0.5)).astype(np.int64)
    rgb[~R["hit"]] = BACKGROUND
    return dict(rgb=rgb, hit=R["hit"], shape=R["shape"], part=part, normal=normal, cell=cell, t=R["t"], c=c)


def ambiguous(scene, colours, camera, rigid, N, env):
    """([H, W] bool, the float64 render): see the head of this file"""
    amb, _ = rmr.ambiguous(scene, camera, rigid, N, env)
    amb = amb.copy()
    R = render(scene, colours, camera, rigid, N, env)
    for du, dv in ((rr.AMBIG_SHIFT, 0), (-rr.AMBIG_SHIFT, 0), (0, rr.AMBIG_SHIFT), (0, -rr.AMBIG_SHIFT)):
        r = render(scene, colours, camera, rigid, N, env, du=du, dv=dv)
        amb |= (r["shape"] != R["shape"]) | (r["part"] != R["part"]) | (r["cell"] != R["cell"])
        amb |= (R["part"] == FLAT) & R["hit"] & (np.abs(r["normal"] - R["normal"]).max(-1) > FACE_TOL)
    return amb, R
