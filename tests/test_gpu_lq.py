"""-m gpu: the LQ blocks of ad_node_kernel + lq_node_kernel on the device against the numpy reference of one shooting node (lq_reference.py), which shares no
code with the oracle or the kernels.  The scenarios of lq_scenarios.py (all sixteen contact modes in motion, both quaternion branches and hemispheres, the relaxed
barriers on both sides of delta, an event-aligned grid over a whole swing), one SQP iteration each from the warm start with the LQ dump on; every block of every
checked node under the project's LQ-block bar, |got - ref|_inf <= 1e-10 max(1, |ref|_inf), and nc equal.  No oracle anywhere in this file.
The reference's share of each test (host time) is printed and recorded in profiles/lq_reference.md."""
import numpy as np
import pytest

import lq_reference as LR
import lq_scenarios as LS

pytestmark = pytest.mark.gpu


def _check(interface, name):
    import gpu_harness as G
    sc, ref, ref_seconds = LS.scenario(interface, name)
    sol = G.make_solver(LS.interface_of(interface, name), sc.B, sc.N)
    sol.enable_debug(True)
    mb = G.MpcBatch(sc.x0, sc.tt, sc.ts, sc.nev, sc.ev, sc.md, sc.N, **LS.solve_args(sc))
    sol.mpc(mb.args)
    out = mb.results()
    assert np.array_equal(out["T"], sc.grid) and (out["stats"][:, 7] == 0).all(), name
    for (i, k) in sc.checks:
        if k < sc.N:
            assert out["mode"][i, k] == LR.node_mode(sc.ev[i, :sc.nev[i]], sc.md[i], sc.grid[i, k]), (name, i, k)
    print(name, "nodes", len(sc.checks), f"reference {ref_seconds:.2f} s ({1e3 * ref_seconds / len(sc.checks):.0f} ms per node)")
    LS.assert_blocks(sc, ref, sol.debug_lq, "gpu")
    sol.close()


def test_all_sixteen_contact_modes_in_motion(interface):
    _check(interface, "all_modes")


def test_quaternion_branches_and_hemispheres(interface):
    _check(interface, "quaternion_branches")


def test_relaxed_barriers_on_both_sides_of_delta(interface):
    _check(interface, "barriers")


def test_event_aligned_grid_over_a_whole_swing(interface):
    _check(interface, "events")


def test_event_aligned_grid_with_the_position_error_gain_on(interface):
    _check(interface, "events_with_position_error_gain")
