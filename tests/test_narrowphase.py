"""The narrowphase reference (tests/narrowphase_reference.py) pinned by closed forms, and the f64 and f32 oracles held to it
on the whole case table (tests/narrowphase_cases.py). No GPU. tests/test_gpu_narrowphase.py holds the HIP routines to the
same checks and to the MEASURED_* constants, which come from the f32 oracle's figures here (python -m tests.narrowphase_cases).
"""
import numpy as np
import pytest

from tests import narrowphase_cases as nc
from tests import narrowphase_reference as ref
from tests.narrowphase_reference import BOX, CAPSULE, CONVEX, CYLINDER, PLANE, SPHERE, Shape

ID = (1, 0, 0, 0)


def P(p, q=ID):
    return list(p) + list(q)


# ------------------------------------------------------------------------------------------ the reference itself
def test_support_values_are_the_maximum_over_sampled_surface_points():
    """h_S(d) of every shape type against a brute-force maximum over points of the shape"""
    rng = np.random.default_rng(1)
    u = rng.normal(size=(20000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    for _ in range(5):
        q, p = nc._rand_q(rng), rng.uniform(-1, 1, size=3)
        hull = nc._hull(rng, 17)
        shapes = [
            (Shape(BOX, P(p, q), [0.03, 0.05, 0.02, 0]), np.sign(u) * [0.03, 0.05, 0.02]),
            (Shape(SPHERE, P(p, q), [0.04, 0, 0, 0]), u * 0.04),
            (Shape(CAPSULE, P(p, q), [0.02, 0.05, 0, 0]), u * 0.02 + np.sign(u[:, :1]) * [0.05, 0, 0]),
            (Shape(CYLINDER, P(p, q), [0.02, 0.05, 0, 0]), np.concatenate([np.sign(u[:, :1]) * 0.05, 0.02 * u[:, 1:] / np.linalg.norm(u[:, 1:], axis=1, keepdims=True)], axis=1)),
            (Shape(CONVEX, P(p, q), [0] * 4, hull), hull.astype(np.float64)),
        ]
        for s, local in shapes:
            world = s.p + local @ s.R.T
            for d in rng.normal(size=(6, 3)):
                d /= np.linalg.norm(d)
                h, brute = ref.support_value(s, d), float(np.max(world @ d))
                assert brute <= h + 1e-12
                assert h - brute < (1e-12 if s.type in (BOX, CONVEX) else 2e-5)  # (sampled curved surfaces: the sampling density)


def test_gap_and_exact_distances_on_hand_cases():
    a, b = Shape(SPHERE, P([0, 0, 0.1]), [0.03]), Shape(SPHERE, P([0, 0, 0]), [0.04])
    assert abs(ref.exact_distance(a, b) - 0.03) < 1e-15 and abs(ref.gap(a, b, [0, 0, 1]) - 0.03) < 1e-15
    assert ref.gap(a, b, [0, 0.6, 0.8]) < 0.03  # any other direction sees a smaller gap
    assert abs(ref.mid_plane(a, b, [0, 0, 1]) - 0.055) < 1e-15
    cap = Shape(CAPSULE, P([0, 0, 0]), [0.02, 0.05])  # axis x
    assert abs(ref.exact_distance(Shape(SPHERE, P([0.01, 0.06, 0]), [0.03]), cap) - 0.01) < 1e-15        # beside the shaft
    assert abs(ref.exact_distance(cap, Shape(SPHERE, P([0.09, 0.03, 0]), [0.01])) - 0.02) < 1e-15        # 3-4-5 beyond the end
    cap2 = Shape(CAPSULE, P([0.01, 0.02, 0.07], nc.Q_X_TO_Y), [0.01, 0.05])  # axis y, crossing above
    assert abs(ref.exact_distance(cap, cap2) - 0.04) < 1e-15
    assert ref.exact_distance(cap, Shape(CAPSULE, P([0, 0.1, 0]), [0.01, 0.05])) is None  # parallel: no closed form claimed
    box = Shape(BOX, P([0, 0, 0]), [0.1, 0.2, 0.3])
    assert abs(ref.exact_distance(Shape(SPHERE, P([0.13, 0.24, 0.1]), [0.01]), box) - 0.04) < 1e-15      # 3-4-5 off an edge
    assert abs(ref.exact_distance(box, Shape(SPHERE, P([0, 0, 0.35]), [0.02])) - 0.03) < 1e-15
    assert ref.exact_distance(box, Shape(SPHERE, P([0, 0, 0.1]), [0.02])) is None                        # centre inside
    # the SAT gap: face, and the crossed edges of tests/test_oracle_contacts.py (3 mm apart)
    assert abs(ref.sat_gap(Shape(BOX, P([0, 0, 0.35]), [0.02] * 3), box) - 0.03) < 1e-15
    h = 0.02 * np.sqrt(2)
    A = Shape(BOX, P([0, 0, 0], nc._q([np.pi / 4, 0, 0])), [0.02] * 3)
    B = Shape(BOX, P([0, 0, -2 * h - 0.003], nc._q([0, np.pi / 4, 0])), [0.02] * 3)
    assert abs(ref.sat_gap(A, B) - 0.003) < 1e-12
    assert max(f[0] for f in ref.sat_axes(A, B)[0]) < 0  # no face axis separates them: only the edge axis does


def test_plane_manifold_closed_forms():
    pl = Shape(PLANE, P([0, 0, 0], nc.Q_X_TO_Y), [0] * 4)  # the plane y = 0, normal +y
    c, n, p = ref.plane_manifold(pl, Shape(SPHERE, P([0.3, 0.035, 0.1]), [0.03]), 0.02)
    assert c == 1 and np.allclose(n, [0, -1, 0]) and np.allclose(p[0], [0.3, 0.0025, 0.1, 0.005], atol=1e-15)
    assert ref.plane_manifold(pl, Shape(SPHERE, P([0.3, 0.0501, 0.1]), [0.03]), 0.02)[0] == 0
    c, n, p = ref.plane_manifold(pl, Shape(CAPSULE, P([0.3, 0.021, 0.1]), [0.02, 0.05]), 0.02)  # parallel: both ends, the -x end first
    assert c == 2 and np.allclose(p, [[0.25, 0.0005, 0.1, 0.001], [0.35, 0.0005, 0.1, 0.001]], atol=1e-15)
    c, n, p = ref.plane_manifold(pl, Shape(CYLINDER, P([0.3, 0.049, 0.1], nc.Q_X_TO_Y), [0.02, 0.05]), 0.02)  # on its face: the centre
    assert c == 1 and np.allclose(p[0], [0.3, -0.0005, 0.1, -0.001], atol=1e-15)
    c, n, p = ref.plane_manifold(pl, Shape(CYLINDER, P([0.3, 0.021, 0.1]), [0.02, 0.05]), 0.02)  # on its side: its whole lowest line ties (the case table has no such case); the reference takes the middle
    assert c == 1 and abs(p[0, 3] - 0.001) < 1e-15 and abs(p[0, 0] - 0.3) < 1e-15
    c, n, p = ref.plane_manifold(pl, Shape(CYLINDER, P([0.3, 0.04, 0.1], nc._q([0, 0, 0.5])), [0.02, 0.05]), 0.1)  # on its rim
    low = np.array([0.3, 0.04, 0.1]) - 0.05 * np.array([np.cos(0.5), np.sin(0.5), 0]) - 0.02 * np.array([-np.sin(0.5), np.cos(0.5), 0])
    assert c == 1 and abs(p[0, 3] - low[1]) < 1e-15 and np.allclose(p[0, [0, 2]], low[[0, 2]], atol=1e-15)
    c, n, p = ref.plane_manifold(pl, Shape(BOX, P([0, 0.031, 0]), [0.02, 0.03, 0.04]), 0.02)  # flat: the 4 lower corners, index order
    assert c == 4 and np.allclose(p[:, 3], 0.001) and np.allclose(p[:, :3], [[-0.02, 0.0005, -0.04], [0.02, 0.0005, -0.04], [-0.02, 0.0005, 0.04], [0.02, 0.0005, 0.04]])
    # a 16-gon cup rim flat on the plane: the extent rule -- vertex 0, the opposite one, and the two at right angles
    cup = nc._cup()
    c, n, p = ref.plane_manifold(pl, Shape(CONVEX, P([0, 0.001, 0], (0.5, -0.5, -0.5, -0.5)), [0] * 4, cup), 0.02)
    assert c == 4 and np.allclose(p[:, 3], 0.001)
    r = np.linalg.norm(p[:, [0, 2]], axis=1)
    assert np.allclose(r, 0.04) and np.linalg.norm(p[0, :3] + p[1, :3] - [0, 0.001, 0]) < 1e-12 and abs(np.dot(p[0, [0, 2]], p[2, [0, 2]])) < 1e-12
    # tilted: only the corner region is inside the slack -> the 4 deepest, by depth
    q = nc._q([0.3, 0.2, 0.0])
    S = Shape(CONVEX, P([0, 0.06, 0], q), [0] * 4, cup)
    c, n, p = ref.plane_manifold(pl, S, 0.08)
    w = S.world_verts()[:, 1]
    assert c == 4 and np.allclose(p[:, 3], np.sort(w)[:4])


def test_box_box_checker_accepts_the_true_manifold_and_rejects_wrong_ones():
    A, B = Shape(BOX, P([0.98, 0.3, 0.021], nc._q([0, 0, 0.4])), [0.02] * 3), Shape(BOX, P([0, 0, -0.5]), [1, 1, 0.5])
    R = A.R
    corners = [A.p + R @ (np.array([sx, sy, -1]) * 0.02) for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1))]
    inside = [c for c in corners if c[0] <= 1.0]
    assert len(inside) == 3  # one corner hangs over the edge x = 1: the overlap polygon has 5 vertices
    pts = [[c[0], c[1], 0.0005, 0.001] for c in inside]
    lo = ref.check_box_box(A, B, 0.02, 3, [0, 0, 1], pts)
    assert lo["kind"] == "face" and lo["n_vertices"] == 5 and max(lo["axis"], lo["depth"], lo["surface"], lo["outside"]) < 1e-12 and lo["deficit"] <= 0
    hang = [c for c in corners if c[0] > 1.0][0]
    bad = ref.check_box_box(A, B, 0.02, 3, [0, 0, 1], [[hang[0], hang[1], 0.0005, 0.001]] + pts[1:])
    assert bad["outside"] > 1e-3  # a point beyond the table edge
    assert ref.check_box_box(A, B, 0.02, 3, [0, 0, 1], [[q[0], q[1], 0.001, 0.001] for q in pts])["surface"] > 4e-4  # off the mid surface
    assert ref.check_box_box(A, B, 0.02, 3, [0, 0, 1], [[q[0], q[1], 0.001, 0.002] for q in pts])["depth"] > 9e-4    # wrong depth
    assert ref.check_box_box(A, B, 0.02, 3, [0.001, 0, 1], pts)["axis"] > 9e-4                                        # tilted normal
    with pytest.raises(AssertionError):
        ref.check_box_box(A, B, 0.02, 3, [1, 0, 0], pts)  # a face axis whose faces do not overlap


# ------------------------------------------------------------------------------------------ the oracles on the whole table
@pytest.fixture(scope="module")
def results(oracle_lib, oracle_lib_f32):
    """the oracles' manifolds of every class, computed once: {(class, precision): out}"""
    out = {}
    for b, force in ((nc.boxbox_batch(), False), (nc.plane_batch(), False), (nc.plane_hull_batch(), False), (nc.mpr_batch(), True), (nc.mpr_boxbox_batch(), True)):
        out[b.name, "f64"] = nc.oracle_collide(oracle_lib, b, force_mpr=force)
        out[b.name, "f32"] = nc.oracle_collide(oracle_lib_f32, b, force_mpr=force)
    for b in (nc.mpr_batch(), nc.mpr_boxbox_batch()):
        out[b.name, "keep"] = nc.mpr_filter(oracle_lib, b, out[b.name, "f64"])
    return out


def test_natural_dispatch_is_the_forced_mpr_where_it_is_the_mpr(oracle_lib, results):
    b = nc.mpr_batch()
    assert np.array_equal(nc.oracle_collide(oracle_lib, b, force_mpr=False), results["mpr", "f64"])


def test_case_tables_cover_what_they_promise(results):
    bb = nc.boxbox_batch()
    c64, n64, p64 = nc.split(results["boxbox", "f64"])
    sizes = {}
    for i in np.where((c64 > 0) & ~bb.tagged("random"))[0]:
        A, B = bb.shapes(i)
        r = ref.check_box_box(A, B, bb.offset, int(c64[i]), n64[i], p64[i])
        if r["kind"] == "face":
            sizes.setdefault(bb.names[i].split()[0], set()).add(r["n_vertices"])
    assert {3, 5, 6} <= sizes["overhang"] and 8 in sizes["yaw45"]
    assert all(c64[i] == 1 for i in range(bb.n) if "crossed" in bb.tags[i])
    assert [int(c64[bb.names.index(f"inside offset {k}")]) for k in (0, 1)] == [4, 4] and [int(c64[bb.names.index(f"outside offset {k}")]) for k in (0, 1)] == [0, 0]
    assert all(c64[i] == 4 for i in range(bb.n) if bb.names[i].startswith("nearly parallel"))
    assert np.mean(c64[bb.tagged("random")] > 0) > 0.5
    ph, cph = nc.plane_hull_batch(), nc.split(results["plane_hull", "f64"])[0]
    assert {int(len(h[1])) for h in ph.hulls} >= set(nc.HULL_COUNTS) and np.mean(cph > 0) > 0.7
    for i in range(ph.n):  # every cup rim lies on its rim: more than 4 vertices within the slack, the extent rule decides
        if ph.names[i].startswith("cup"):
            A, B = ph.shapes(i)
            s = (B.world_verts() - A.p) @ A.R[:, 0]
            assert np.sum(s[s < ph.offset] <= s.min() + ref.PATCH_SLACK) > 4 and cph[i] == 4, ph.names[i]
    last = [i for i in range(ph.n) if ph.names[i].endswith("deepest last")]
    assert len(last) > 100 and all(np.argmin((ph.shapes(i)[1].world_verts() - ph.shapes(i)[0].p) @ ph.shapes(i)[0].R[:, 0]) == len(ph.hulls[i][1]) - 1 for i in last)
    m, cm = nc.mpr_batch(), nc.split(results["mpr", "f64"])[0]
    assert all(cm[i] == 1 for i in range(m.n) if "tie" in m.tags[i]) and 0.05 < np.mean(cm == 0) < 0.3


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_oracle_box_box_manifolds(results, precision):
    b = nc.boxbox_batch()
    far = b.tagged("far")
    out, out64 = results["boxbox", precision], results["boxbox", "f64"]
    for mask, measured in ((~far, nc.MEASURED_BOXBOX), (far, nc.MEASURED_BOXBOX_FAR)):
        fig = nc.eval_boxbox(b, out, out64, mask)
        print(precision, {k: f"{v[0]:.2e}" for k, v in fig.items()})
        if precision == "f64":  # the reference's own error: geometry in float64 on both sides (the oracle's output is cast to float32)
            tol = 16 * 2.0 ** -24 if mask is far else 2.0 ** -24
            assert all(fig[k][0] <= 2 * tol for k in ("unit", "axis", "depth", "surface", "outside", "deficit")), fig
        else:
            nc.within(fig, measured, "f32 oracle, box-box")
    d = b.tagged("dyadic")
    assert d.sum() >= 40 and np.array_equal(results["boxbox", "f32"][d], out64[d])  # exact in either precision
    c, n, p = nc.split(out64[d])
    assert np.all(c == 4) and np.all(np.abs(n[:, 2]) == 1.0)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("cls", ["plane", "plane_hull"])
def test_oracle_plane_manifolds(results, precision, cls):
    b = nc.plane_batch() if cls == "plane" else nc.plane_hull_batch()
    fig = nc.eval_plane(b, results[cls, precision], results[cls, "f64"])
    print(precision, {k: f"{v[0]:.2e}" for k, v in fig.items()})
    if precision == "f64":  # float64 geometry on both sides, output cast to float32: half an ulp of coordinates below 1 m
        assert all(fig[k][0] <= 2.0 ** -24 for k in ("n", "x", "sep")), fig
    else:
        nc.within(fig, nc.MEASURED_PLANE if cls == "plane" else nc.MEASURED_PLANE_HULL, "f32 oracle, " + cls)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("cls", ["mpr", "mpr_boxbox"])
def test_oracle_mpr_manifolds(results, precision, cls):
    b = nc.mpr_batch() if cls == "mpr" else nc.mpr_boxbox_batch()
    measured = nc.MEASURED_MPR if cls == "mpr" else nc.MEASURED_MPR_BOXBOX
    fig = nc.eval_mpr(b, results[cls, precision], results[cls, "f64"], results[cls, "keep"])
    print(precision, {k: f"{v[0]:.2e}" for k, v in fig.items()})
    nc.within(fig, measured, precision + " oracle, " + cls)  # (the f64 oracle carries the algorithm's own error: held to the same constants)
