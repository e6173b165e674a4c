"""The manifold routines of the control-step kernel, pair by pair, against the float64 reference.

`mssim_test_collide` (maniskill_amd/csrc/mssim_test_collide.h; a test hook, not part of the ABI) runs the device functions
that k_solve16 calls on a batch of explicit shape pairs. Every path is held to the checks of tests/test_narrowphase.py and
to the MEASURED_* constants of tests/narrowphase_cases.py, which come from the f32 ORACLE's error (never from these kernels).

Routine, the path of k_solve16 it runs on, and the asserted cases that reach it:
  collide_plane            per lane (stage A)        'plane': every primitive; capsule parallel; cylinder on rim and face
  collide_box_box<16>      per lane (stage A)        'boxbox' on path 0: dyadic, yaw 45, overhangs, edges, offsets, random families
  collide_box_box_coop     16 lanes (stage C)        'boxbox' on path 1: the same table, and case-by-case agreement with path 0
  collide_plane_hull_coop  16 lanes (stage C)        'plane_hull': 4..64 vertices, cup rims (extent rule), deepest vertex last
  collide_mpr_t/SupCoop16  16 lanes (stage B)        'mpr' on path 1: all type pairs, hull ties, hull sizes as A and as B
  collide_mpr_t/SupDirect  per lane (the hook only)  'mpr' on path 0, 'mpr_boxbox' on path 2, agreement with SupCoop16
Not covered here: the triangle stage, the persistent-manifold cache and its growth queries, the patch reduction.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from maniskill_amd import native
from tests import narrowphase_cases as nc
from tests import oracle_backend as ob

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hook():
    lib = C.CDLL(native.NATIVE_LIB_PATH)
    fn = lib.mssim_test_collide
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p]
    lib.mssim_last_error.restype = C.c_char_p
    lib.mssim_last_error.argtypes = [C.c_void_p]
    return lib


def launch(hook, type_, pose, param, hull, verts, offset, path, fill=0.0, n_verts=None):
    """(return code, message, out [n][20]) of one call of the hook on host arrays"""
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (type_, pose, param, hull, verts)]
    n = len(type_)
    out = torch.full((max(n, 1), 20), fill, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    rc = hook.mssim_test_collide(n, *(x.data_ptr() for x in t[:4]), t[4].data_ptr(), len(verts) if n_verts is None else n_verts, offset, path, out.data_ptr(),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, (hook.mssim_last_error(None) or b"").decode(), out.cpu().numpy()[:n]


def run(hook, batch, path):
    hull, verts = batch.packed_hulls()
    rc, msg, out = launch(hook, batch.type, batch.pose, batch.param, hull, verts, batch.offset, path)
    assert rc == 0, msg
    return out


@pytest.fixture(scope="module")
def f64():
    """the f64 oracle's manifolds of every class and the MPR stability masks, computed once"""
    lib = ob.load_oracle("f64")
    out = {}
    for b, force in ((nc.boxbox_batch(), False), (nc.plane_batch(), False), (nc.plane_hull_batch(), False), (nc.mpr_batch(), True), (nc.mpr_boxbox_batch(), True)):
        out[b.name] = nc.oracle_collide(lib, b, force_mpr=force)
    for b in (nc.mpr_batch(), nc.mpr_boxbox_batch()):
        out[b.name, "keep"] = nc.mpr_filter(lib, b, out[b.name])
    return out


def show(what, fig):
    print(what, {k: f"{v[0]:.2e}" for k, v in fig.items()})


@pytest.fixture(scope="module")
def boxbox(hook):
    b = nc.boxbox_batch()
    return {path: run(hook, b, path) for path in (0, 1)}


@pytest.mark.parametrize("path", [0, 1])
def test_box_box_manifolds(boxbox, f64, path):
    """collide_box_box<16> (path 0) and collide_box_box_coop (path 1): count and point order of the f64 oracle on every case,
    the reference's checks within the measured constants"""
    b, out, out64 = nc.boxbox_batch(), boxbox[path], f64["boxbox"]
    far = b.tagged("far")
    for mask, measured, what in ((~far, nc.MEASURED_BOXBOX, "box-box"), (far, nc.MEASURED_BOXBOX_FAR, "box-box, 10 m out")):
        fig = nc.eval_boxbox(b, out, out64, mask)
        show(f"path {path} {what}:", fig)
        nc.within(fig, measured, f"path {path}, {what}")
    print(f"path {path}: bitwise equal to the f64 oracle (cast to float32) on {nc.bitwise_share(out, out64):.1%} of {b.n} cases")


@pytest.mark.parametrize("path", [0, 1])
def test_box_box_dyadic_cases_equal_the_f64_oracle(boxbox, f64, path):
    """Cube of half 2^-6 on a 1 x 1 x 0.5 table and on an equal cube, every number dyadic, every frame axis-aligned: count,
    order and value of the f64 oracle, exactly (as numbers: the sign of a zero is not pinned).

    The 12 cases with the cube as shape A on the table are the sharp ones: by the tie rule the cube's face is the reference
    face and the 1 m table face is what gets clipped, the second clip plane cuts an edge that runs from x = 2^-6 to x = -0.5,
    and the interpolation weight is 0.03125 / 0.515625 = 2 / 33, not a dyadic number. They hold only because the clip
    interpolation (clip_cross, mssim_dev.h) is the oracle's IEEE sequence: with da * rcp(da - db) one coordinate of up to three
    points was 1.5e-8 to 8.9e-8 m (16 ulp) off on both paths."""
    b, out, out64 = nc.boxbox_batch(), boxbox[path], f64["boxbox"]
    d = b.tagged("dyadic")
    bad = [i for i in np.where(d)[0] if not np.array_equal(out[i], out64[i])]
    for i in bad[:3]:
        print(b.names[i], out[i], out64[i])
    worst = max([float(np.max(np.abs(out[i].astype(np.float64) - out64[i]))) for i in bad] + [0.0])
    assert not bad, f"path {path}: {len(bad)} of {d.sum()} dyadic cases differ from the f64 oracle by up to {worst:.3g}: {[b.names[i] for i in bad]}"


def test_box_box_per_lane_and_16_lane_routines_agree(boxbox):
    b = nc.boxbox_batch()
    (c0, n0, p0), (c1, n1, p1) = nc.split(boxbox[0]), nc.split(boxbox[1])
    bad = [b.names[i] for i in np.where(c0 != c1)[0]]
    assert not bad, f"count differs between collide_box_box<16> and collide_box_box_coop: {bad[:8]}"
    far = b.tagged("far")
    for mask, m in ((~far, nc.MEASURED_BOXBOX), (far, nc.MEASURED_BOXBOX_FAR)):
        # (same points in the same order: a swapped pair of points is an error of centimetres)
        assert np.max(np.abs(n0[mask] - n1[mask])) <= m["n_vs_f64"]
        assert np.max(np.abs(p0[mask][:, :, :3] - p1[mask][:, :, :3])) <= m["x_vs_f64"]
        assert np.max(np.abs(p0[mask][:, :, 3] - p1[mask][:, :, 3])) <= m["sep_vs_f64"]
    print(f"collide_box_box<16> and collide_box_box_coop bitwise equal on {nc.bitwise_share(boxbox[0], boxbox[1]):.1%} of {b.n} cases")


@pytest.mark.parametrize("cls", ["plane", "plane_hull"])
def test_plane_manifolds(hook, f64, cls):
    """collide_plane per lane on every primitive; collide_plane_hull_coop by 16 lanes on hulls of 4 to 64 vertices"""
    b = nc.plane_batch() if cls == "plane" else nc.plane_hull_batch()
    out = run(hook, b, 0 if cls == "plane" else 1)
    fig = nc.eval_plane(b, out, f64[cls])
    show(cls + ":", fig)
    nc.within(fig, nc.MEASURED_PLANE if cls == "plane" else nc.MEASURED_PLANE_HULL, cls)
    print(f"{cls}: bitwise equal to the f64 oracle (cast to float32) on {nc.bitwise_share(out, f64[cls]):.1%} of {b.n} cases")


@pytest.fixture(scope="module")
def mpr(hook):
    b = nc.mpr_batch()
    return {path: run(hook, b, path) for path in (0, 1, 2)}


@pytest.mark.parametrize("path", [0, 1, 2])
def test_mpr_manifolds(mpr, f64, path):
    """collide_mpr_t with SupDirect (paths 0 and 2) and with SupCoop16 (path 1)"""
    b = nc.mpr_batch()
    fig = nc.eval_mpr(b, mpr[path], f64["mpr"], f64["mpr", "keep"])
    show(f"path {path} mpr:", fig)
    nc.within(fig, nc.MEASURED_MPR, f"path {path}, mpr")
    print(f"path {path}: bitwise equal to the f64 oracle (cast to float32) on {nc.bitwise_share(mpr[path], f64['mpr']):.1%} of {b.n} cases")


def test_mpr_forced_on_box_box(hook, f64):
    b = nc.mpr_boxbox_batch()
    out = run(hook, b, 2)
    fig = nc.eval_mpr(b, out, f64["mpr_boxbox"], f64["mpr_boxbox", "keep"])
    show("path 2 mpr_boxbox:", fig)
    nc.within(fig, nc.MEASURED_MPR_BOXBOX, "path 2, forced box-box")


def test_mpr_support_policies_agree(mpr):
    """SupDirect against SupCoop16: the count on every case; sep within the constant"""
    b = nc.mpr_batch()
    print(f"paths 0 and 2 (no box-box pair in this batch: the same routine) bitwise equal on {nc.bitwise_share(mpr[0], mpr[2]):.1%}")
    (c0, n0, p0), (c1, n1, p1) = nc.split(mpr[0]), nc.split(mpr[1])
    bad = [b.names[i] for i in np.where(c0 != c1)[0]]
    assert not bad, f"count differs between SupDirect and SupCoop16: {bad[:8]}"
    assert np.max(np.abs(p0[:, 0, 3] - p1[:, 0, 3])) <= nc.MEASURED_MPR["sep_vs_f64"]
    tie = b.tagged("tie")
    assert np.max(np.abs(p0[tie, 0, :3] - p1[tie, 0, :3])) <= nc.MEASURED_MPR["tie_x"]
    print(f"SupDirect and SupCoop16 bitwise equal on {nc.bitwise_share(mpr[0], mpr[1]):.1%} of {b.n} cases; "
          f"largest difference in n {np.max(np.abs(n0 - n1)):.2e}, in x {np.max(np.abs(p0[:, 0, :3] - p1[:, 0, :3])):.2e}")


def test_hook_refuses_malformed_batches_without_launching(hook):
    verts = np.zeros((16, 3), dtype=np.float32)
    verts[:, 0] = np.arange(16)

    def call(ta, tb, hull_a=(0, 0), hull_b=(0, 0), path=0, offset=0.02, n_verts=None, vbuf=verts):
        type_ = np.array([[ta, tb]], dtype=np.int32)
        pose = np.array([[[0, 0, 1, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0]]], dtype=np.float32)
        param = np.full((1, 2, 4), 0.02, dtype=np.float32)
        hull = np.array([[hull_a, hull_b]], dtype=np.int32)
        return launch(hook, type_, pose, param, hull, vbuf, offset, path, fill=-7.0, n_verts=n_verts)

    rc, msg, out = call(nc.SPHERE, nc.CONVEX, hull_b=(8, 8), path=1)
    assert rc == 0 and out[0, 0] in (0.0, 1.0) and not np.any(out == -7.0)  # a well-formed batch runs and fills its row
    malformed = dict(
        type_above_range=dict(ta=nc.BOX, tb=6),
        trimesh=dict(ta=7, tb=nc.BOX),
        negative_type=dict(ta=-1, tb=nc.BOX),
        plane_as_b=dict(ta=nc.BOX, tb=nc.PLANE),
        no_vertices=dict(ta=nc.SPHERE, tb=nc.CONVEX, hull_b=(0, 0)),
        too_many_vertices=dict(ta=nc.SPHERE, tb=nc.CONVEX, hull_b=(0, 65)),
        unaligned_start=dict(ta=nc.CONVEX, tb=nc.SPHERE, hull_a=(4, 4)),
        negative_start=dict(ta=nc.CONVEX, tb=nc.SPHERE, hull_a=(-8, 4)),
        past_the_buffer=dict(ta=nc.SPHERE, tb=nc.CONVEX, hull_b=(8, 9)),
        padding_past_the_buffer=dict(ta=nc.SPHERE, tb=nc.CONVEX, hull_b=(8, 5), n_verts=14),
        plane_hull_per_lane=dict(ta=nc.PLANE, tb=nc.CONVEX, hull_b=(0, 8), path=0),
        plane_primitive_16_lanes=dict(ta=nc.PLANE, tb=nc.SPHERE, path=1),
        plane_forced_mpr=dict(ta=nc.PLANE, tb=nc.SPHERE, path=2),
        unknown_path=dict(ta=nc.BOX, tb=nc.BOX, path=3),
        negative_offset=dict(ta=nc.BOX, tb=nc.BOX, offset=-0.01),
        nan_offset=dict(ta=nc.BOX, tb=nc.BOX, offset=float("nan")),
    )
    for name, kw in malformed.items():
        rc, msg, out = call(**kw)
        assert rc != 0 and msg.startswith("mssim_test_collide:"), (name, rc, msg)
        assert np.all(out == -7.0), f"{name}: refused, but the output was written"
