"""CPU tier: the yardstick of the feedback-policy checks (feedback_reference.py) pinned against kkt_reference.py before any kernel is involved, on the oracle's LQ
blocks of kkt_scenarios.emu_scenarios()."""
import numpy as np
import pytest

import feedback_reference as FR
import kkt_reference as KR
import kkt_scenarios as KS
import support as S
from qm_door_amd import api


@pytest.fixture(scope="module")
def host():
    itf = api.QMInterface()
    return itf, S.Oracle(itf.problem)


@pytest.mark.parametrize("name", list(KS.emu_scenarios()))
def test_unit_right_hand_sides_give_the_sensitivity_of_the_first_input(host, name):
    """K_ref from the 30 unit right-hand sides equals, column by column, the difference of two kkt_reference.solve calls (dx0 = e_j minus dx0 = 0) on three
    nodes, and satisfies the linearised constraint C_k + D_k K_k = 0 on the nc live rows.  Tolerance: the rule of feedback_reference.py measured on these nodes;
    the difference of two full solutions additionally carries the rounding of both to fp64 and of the subtraction, 4 eps of the larger one (derived)."""
    itf, orc = host
    sc = KS.build(KS.emu_scenarios(), name, itf, orc)
    grid, nev, ev, md, tt, ts = sc.instance(0)
    blocks = KR.oracle_blocks(orc, grid, sc.X[0], sc.U[0], nev, ev, md, tt, ts)
    Knp = FR.numpy_gains(blocks)
    nodes = sorted({0, sc.N // 2, sc.N - 1})
    refs = {k: FR.reference_gain(blocks[k:]) for k in nodes}
    e_lu = max(KR.rel_err(r["K_lu"], r["K"]) for r in refs.values())
    e_np = max(KR.rel_err(Knp[k], r["K"]) for k, r in refs.items())
    tol = KS.FACTOR * max(e_lu, e_np)
    print(name, "e_lu", e_lu, "e_np", e_np, "tol", tol, "correction", [r["correction"] for r in refs.values()])
    for k, r in refs.items():
        K = r["K"]
        assert r["correction"] <= 1e-2 * tol, (name, k)
        base = KR.solve(blocks[k:], np.zeros(30))["dU"][0]
        for j in range(30):
            col = KR.solve(blocks[k:], np.eye(30)[j])["dU"][0]
            allow = tol * np.abs(K).max() + 4 * FR.EPS * max(np.abs(col).max(), np.abs(base).max())
            assert np.abs((col - base) - K[:, j]).max() <= allow, (name, k, j)
        nc = int(blocks[k]["nc"])
        C, D = blocks[k]["C"][:nc], blocks[k]["D"][:nc]
        assert (np.abs(C + D @ K) <= tol * (np.abs(C) + np.abs(D) @ np.abs(K))).all(), (name, k)


def test_checked_nodes_of_a_long_horizon():
    modes = np.r_[np.full(30, 15), np.full(40, 9), np.full(131, 6)]
    got = FR.checked_nodes(200, modes)
    assert {0, 1, 2, 197, 198, 199, 29, 30, 69, 70, 25, 50, 175} <= set(got) and max(got) == 199
    assert FR.checked_nodes(40, modes) == list(range(40))
