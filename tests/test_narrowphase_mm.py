"""The millimetre-scale box-box rows of tests/narrowphase_mm_cases.py (a peg of PlugCharger's charger in a slot of its
receptacle: 0.5 mm clearance under a 20 mm contact offset) through the machinery of tests/test_narrowphase.py: the f64 and
the f32 oracle against the float64 reference, with the bounds of that file. No GPU; tests/test_gpu_narrowphase_mm.py holds
the HIP routines to the same checks."""
import numpy as np
import pytest

from tests import narrowphase_cases as nc
from tests import narrowphase_mm_cases as mm
from tests import narrowphase_reference as ref


@pytest.fixture(scope="module")
def results(oracle_lib, oracle_lib_f32):
    b = mm.mm_batch()
    return {"f64": nc.oracle_collide(oracle_lib, b), "f32": nc.oracle_collide(oracle_lib_f32, b)}


def test_slot_is_a_peg_plus_half_a_millimetre_per_side():
    W = mm.walls()
    lo = {k: np.array(c) - np.array(h) for k, (c, h) in W.items()}
    hi = {k: np.array(c) + np.array(h) for k, (c, h) in W.items()}
    assert abs((lo["outer block"][1] - hi["filler"][1]) - (2 * mm.PEG[1] + 1e-3)) < 1e-15 and abs(0.5 * (lo["outer block"][1] + hi["filler"][1]) - mm.GAP) < 1e-15
    assert abs((lo["top plate"][2] - hi["bottom plate"][2]) - (2 * mm.PEG[2] + 1e-3)) < 1e-15
    assert all(abs(hi[k][0]) < 1e-15 and abs(lo[k][0] + 2e-2) < 1e-15 for k in W)


def test_cases_are_what_their_names_say(results):
    """the reference's own gap of every row: 0.5 mm for the centred peg, 0 and -0.2 mm for the moved one (within the float32
    rounding of the poses), an overlap for the tilted ones, an edge-edge axis for the edge-on ones; every row is in contact
    range and gives a manifold"""
    b = mm.mm_batch()
    c64, n64, p64 = nc.split(results["f64"])
    assert b.n == 8 + 8 + 8 + 4 + 6 and np.all(c64 > 0)
    kinds = {}
    for i in range(b.n):
        A, B = b.shapes(i)
        g = ref.sat_gap(A, B)
        r = ref.check_box_box(A, B, b.offset, int(c64[i]), n64[i], p64[i])
        kinds[b.names[i]] = r["kind"]
        if "clear" in b.tags[i]:
            assert abs(g - 5e-4) < 2e-9 and r["kind"] == "face" and c64[i] == 4, (b.names[i], g)
        elif "0 gap" in b.tags[i]:
            assert abs(g) < 2e-9 and c64[i] == 4, (b.names[i], g)
        elif "0.2 mm penetration" in b.tags[i]:
            assert abs(g + 2e-4) < 2e-9 and c64[i] == 4, (b.names[i], g)
        elif "tilted" in b.tags[i]:
            # 8 mm x sin 0.1 = 0.8 mm at the peg's end, more than the clearance: every wall the peg turns toward is entered
            assert g < 0, (b.names[i], g)
        elif "edge" in b.tags[i]:
            assert abs(g - (3e-4 if b.names[i].endswith("off") else -1e-4)) < 2e-9 and r["kind"] == "edge" and c64[i] == 1, (b.names[i], g, r["kind"])
    assert sum(k == "edge" for k in kinds.values()) >= 6


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_oracle_manifolds_at_millimetre_scale(results, precision):
    b = mm.mm_batch()
    fig = nc.eval_boxbox(b, results[precision], results["f64"])
    print(precision, {k: f"{v[0]:.2e}" for k, v in fig.items()})
    if precision == "f64":  # the reference's own error, as in tests/test_narrowphase.py: float64 geometry, output cast to float32
        assert all(fig[k][0] <= 2 * 2.0 ** -24 for k in ("unit", "axis", "depth", "surface", "outside", "deficit")), fig
    else:
        nc.within(fig, nc.MEASURED_BOXBOX, "f32 oracle, box-box at millimetre scale")
