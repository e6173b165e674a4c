"""The HIP control-step kernel's ARTICULATED contact rows against a direct LCP solution -- an answer that does not come from the
oracle -- on EVERY plain-step instance of k_solve16 (tests/test_dispatch.py holds the scene list to the instance list). The
scenes of tests/articulated_lcp_cases.py (a pad on a slider pushing a cube, with and without its joint limit; a three-joint arm
pressing on a cube, alone, in the four-row layout, and with an idle second branch and a second cube in the generic two-row
layout; two pads holding / dropping a cube with free and with saturated drives; a cube spinning on a turntable link; the Panda
pinching a box, with and without the tendon, and with a second cube on it in the two-row layout; the Fetch pinching a box, alone
and with a second cube, pressing a pad under its torso on the ground, and running three joints into their limits; panda_stick
pushing a floating cube that is dragged along its pad) and their mesh variants (one triangle far away: the TRI instance on the
same problem; the ground plane replaced by one triangle: the ground contacts out of the triangle stage) run through the public
step API: N = 5 envs, one substep, the sweeps allowed to converge. Compared env by env with
tests/indep_lcp.py::solve_substep_generalized under MEASURED_V / MEASURED_I -- four times the float32 ORACLE's error, measured on
the CPU (tests/test_oracle_articulated_lcp.py), for the scenes added with the Fetch never below the f64 oracle's allowance -- plus
contact counts and no overflow.
"""
import pytest

from maniskill_amd.physx.system import MssimSystem
from tests import articulated_lcp_cases as cases
from tests.test_oracle_articulated_lcp import references

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", cases.CASES)
def test_kernel_matches_direct_lcp_solution(name, tmp_path):
    sc = cases.make_scene(name, tmp_path)
    model = cases.compile_scene(sc)  # (asserts the (NDOF, NR, TRI) instance the scene is meant for)
    gpu = MssimSystem(device="cuda:0")
    gpu.gpu_init(model, cases.N)
    got = cases.run_solver(gpu, sc, model)
    assert gpu.overflow_count() == 0
    ev, ei = cases.errors(sc, model, got, references(sc))  # (contact counts = the reference's points per pair, asserted inside)
    bound_v, bound_i = cases.MEASURED_V[cases.bounds_name(name)], cases.MEASURED_I[cases.bounds_name(name)]
    print(f"\nGPU {name} instance {sc.instance}: velocity {ev:.3g} (bound {bound_v:.3g}) impulse {ei:.3g} (bound {bound_i:.3g})")
    assert ev <= bound_v and ei <= bound_i, (ev, ei)
