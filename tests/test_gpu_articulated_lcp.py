"""The HIP control-step kernel's ARTICULATED contact rows against a direct LCP solution -- an answer that does not come from the
oracle. The scenes of tests/articulated_lcp_cases.py (a pad on a slider pushing a cube, with and without its joint limit; a
three-joint arm pressing on a cube, alone and in the four-row layout; two pads holding / dropping a cube with free and with
saturated drives; a cube spinning on a turntable link; the Panda pinching a box, with and without the tendon, and with a second
cube on it in the two-row layout) run through the public step API: N = 5 envs, one substep, the sweeps allowed to converge.
Compared env by env with tests/indep_lcp.py::solve_substep_generalized under MEASURED_V / MEASURED_I -- four times the float32
ORACLE's error, measured on the CPU (tests/test_oracle_articulated_lcp.py) -- plus contact counts and no overflow.
"""
import pytest

from maniskill_amd.physx.system import MssimSystem
from tests import articulated_lcp_cases as cases
from tests.test_oracle_articulated_lcp import references

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(cases.SCENES))
def test_kernel_matches_direct_lcp_solution(name, tmp_path):
    sc = cases.make_scene(name, tmp_path)
    model = cases.compile_scene(sc)  # (asserts the (NDOF, NR) instance the scene is meant for)
    gpu = MssimSystem(device="cuda:0")
    gpu.gpu_init(model, cases.N)
    got = cases.run_solver(gpu, sc, model)
    assert gpu.overflow_count() == 0
    ev, ei = cases.errors(sc, model, got, references(sc))  # (contact counts = the reference's points per pair, asserted inside)
    print(f"\nGPU {name} instance {sc.instance}: velocity {ev:.3g} (bound {cases.MEASURED_V[name]:.3g}) impulse {ei:.3g} (bound {cases.MEASURED_I[name]:.3g})")
    assert ev <= cases.MEASURED_V[name] and ei <= cases.MEASURED_I[name], (ev, ei)
