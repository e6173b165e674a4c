"""The millimetre-scale box-box rows of tests/narrowphase_mm_cases.py through `mssim_test_collide`, with the helpers and the
bounds of tests/test_gpu_narrowphase.py: collide_box_box<16> (path 0, per lane) and collide_box_box_coop (path 1, 16 lanes)
give the f64 oracle's count and point order on every row -- the peg 0.5 mm from a slot wall, touching it, 0.2 mm inside it,
tilted by 0.1 rad in the slot, edge-on at the slot's mouth -- and the float64 reference's checks within MEASURED_BOXBOX."""
import numpy as np
import pytest

from tests import narrowphase_cases as nc
from tests import narrowphase_mm_cases as mm
from tests import oracle_backend as ob
from tests.test_gpu_narrowphase import hook, run, show  # noqa: F401  (`hook` is that file's fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def f64():
    return nc.oracle_collide(ob.load_oracle("f64"), mm.mm_batch())


@pytest.fixture(scope="module")
def boxbox(hook):  # noqa: F811
    b = mm.mm_batch()
    return {path: run(hook, b, path) for path in (0, 1)}


@pytest.mark.parametrize("path", [0, 1])
def test_box_box_manifolds_at_millimetre_scale(boxbox, f64, path):
    b, out = mm.mm_batch(), boxbox[path]
    fig = nc.eval_boxbox(b, out, f64)
    show(f"path {path} box-box at millimetre scale:", fig)
    nc.within(fig, nc.MEASURED_BOXBOX, f"path {path}, box-box at millimetre scale")
    print(f"path {path}: bitwise equal to the f64 oracle (cast to float32) on {nc.bitwise_share(out, f64):.1%} of {b.n} cases")


def test_per_lane_and_16_lane_routines_agree_at_millimetre_scale(boxbox):
    b = mm.mm_batch()
    (c0, n0, p0), (c1, n1, p1) = nc.split(boxbox[0]), nc.split(boxbox[1])
    bad = [b.names[i] for i in np.where(c0 != c1)[0]]
    assert not bad, f"count differs between collide_box_box<16> and collide_box_box_coop: {bad[:8]}"
    m = nc.MEASURED_BOXBOX
    assert np.max(np.abs(n0 - n1)) <= m["n_vs_f64"] and np.max(np.abs(p0[:, :, :3] - p1[:, :, :3])) <= m["x_vs_f64"]
    assert np.max(np.abs(p0[:, :, 3] - p1[:, :, 3])) <= m["sep_vs_f64"]
