"""CPU tier: the dual reference (dual_reference.py) on its own -- the three KKT identities on its refined solution, on oracle blocks of a trot at N = 7 with a
mode switch, and a hand-made two-node scalar problem whose multipliers are written out by hand."""
import numpy as np
import pytest

import dual_reference as DR
import kkt_reference as KR
import kkt_scenarios as KS
import support as S
from qm_door_amd import api


@pytest.fixture(scope="module")
def host():
    itf = api.QMInterface()
    return itf, S.Oracle(itf.problem)


def test_reference_satisfies_the_kkt_identities_on_a_trot(host):
    """Oracle blocks of a defect-laden trot iterate, N = 7 across the first switch (nc 12 and 14): every row of the three identities holds on the refined solution
    within TERMS eps of the sum of the magnitudes of its terms (one fp64 evaluation of an at most 78-term sum), the plain LU multipliers are close to the refined
    ones, and the primal part is the step of kkt_reference.solve bit for bit (the same factorisation and refinement)."""
    itf, orc = host
    sc = KS.unroll(itf, orc, "trot", 1, 7, 13, True, False)
    grid, nev, ev, md, tt, ts = sc.instance(0)
    blocks = KR.oracle_blocks(orc, grid, sc.X[0], sc.U[0], nev, ev, md, tt, ts)
    assert sorted({int(b["nc"]) for b in blocks[:-1]}) == [12, 14]
    ref = DR.solve(blocks)
    worst = DR.worst_identity(blocks, ref["dX"], ref["dU"], ref["lam"], ref["nu"])
    print("identities", worst, "e_lu", ref["e_lu"], "correction", ref["correction"], "refinements", ref["refinements"], "floor", DR.rounding_floor(blocks, ref))
    assert all(v <= DR.TERMS * DR.EPS for v in worst.values()), worst
    assert max(ref["e_lu"]) <= 1e-10 and max(ref["correction"]) <= 1e-2 * max(max(ref["e_lu"]), DR.EPS)
    step = KR.solve(blocks)
    assert np.array_equal(step["dX"], ref["dX"]) and np.array_equal(step["dU"], ref["dU"])
    assert [len(v) for v in ref["nu"]] == [int(b["nc"]) for b in blocks[:-1]] and ref["lam"].shape == (8, 30)
    # a wrong sign or a shifted node shows at the size of the terms
    bad = DR.worst_identity(blocks, ref["dX"], ref["dU"], -ref["lam"], ref["nu"])
    assert min(bad.values()) > 1e-3, bad


def test_reference_on_a_scalar_problem_solved_by_hand():
    """N = 1, one state, one input, one constraint row, dx_0 = 0:
        min  1/2 u^2 + u  +  1/2 * 2 x1^2 + 3 x1      s.t.  x1 = 2 x0 + u + 1,   0.5 x0 + 2 u + 1 = 0     (Q_0 = 1, q_0 = 4: they touch lambda_0 only)
    The constraint fixes u = -1/2, so x1 = 1/2.  By hand:
        lambda_1 = Q_1 x1 + q_1                      = 2 * 1/2 + 3          = 4
        0 = R u + r + B lambda_1 + D nu              = -1/2 + 1 + 4 + 2 nu  ->  nu = -9/4
        lambda_0 = Q_0 x0 + q_0 + A lambda_1 + C nu  = 0 + 4 + 8 - 9/8      = 87/8"""
    m = lambda v: np.array([[float(v)]])  # noqa: E731
    v = lambda s: np.array([float(s)])    # noqa: E731
    blocks = [dict(A=m(2), B=m(1), b=v(1), Q=m(1), R=m(1), q=v(4), r=v(1), C=m(0.5), D=m(2), e=v(1), nc=1), dict(Q=m(2), q=v(3))]
    ref = DR.solve(blocks)
    assert np.allclose(ref["dX"][:, 0], [0.0, 0.5], rtol=0, atol=4 * DR.EPS) and np.allclose(ref["dU"][:, 0], [-0.5], rtol=0, atol=4 * DR.EPS)
    assert np.allclose(ref["lam"][:, 0], [87.0 / 8.0, 4.0], rtol=8 * DR.EPS, atol=0), ref["lam"]
    assert np.allclose(ref["nu"][0], [-9.0 / 4.0], rtol=8 * DR.EPS, atol=0), ref["nu"]
    assert np.allclose(ref["lam_lu"][:, 0], [87.0 / 8.0, 4.0], rtol=64 * DR.EPS, atol=0)
    assert np.array_equal(DR.pad_nu(ref["nu"]), np.r_[[ref["nu"][0][0]], np.zeros(15)][None, :])
    # a nonzero dx_0 moves the multipliers as the identities say: x0 = 1 -> u = -3/4, x1 = 9/4, lambda_1 = 15/2, nu = -(-3/4 + 1 + 15/2) / 2 = -31/8
    ref = DR.solve(blocks, dx0=np.array([1.0]))
    assert np.allclose(ref["lam"][1], [7.5], rtol=8 * DR.EPS) and np.allclose(ref["nu"][0], [-31.0 / 8.0], rtol=8 * DR.EPS)
    assert np.allclose(ref["lam"][0], [1.0 + 4.0 + 2 * 7.5 + 0.5 * (-31.0 / 8.0)], rtol=8 * DR.EPS)
