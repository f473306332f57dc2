"""CPU tier: the numpy reference of the SQP solution metrics (metrics_reference.py) against the references that already exist -- ls_reference.node_performance (the
dt-scaled cost and the two squared norms per node), lq_reference.lq_node (b and e at the same point) and ls_reference.performance (the totals).

Sign convention checked here: lq_reference's.  b = rk2(x, u, dt) - x_next and e = the VALUE of the equality row (the QP reads them as A dx + B du + b = dx_next and
C dx + D du + e = 0); defect and eq of the metrics are these two, with the same sign and the same row order."""
import numpy as np
import pytest

import lq_reference as LR
import ls_reference as LSR
import ls_scenarios as L
import metrics_reference as MR

REL = 1e-13   # two numpy evaluations of the same formulas in another order of summation


@pytest.fixture(scope="module")
def cases(interface):
    """infeasible iterates with O(0.1) defects and constraint values: N = 7 across the first switch of the trot (nc 12 -> 14), and a non-uniform grid with a far target"""
    P = L.base_params(interface)
    grid = np.array([0.0, 0.015, 0.02, 0.03, 0.045, 0.0525, 0.06])
    insts = [L.defect_instance(P, 7, 3, 0.05, None), L.defect_instance(P, len(grid) - 1, 4, 0.05, None, target_scale=0.5, grid=grid)]
    out = []
    for inst in insts:
        ev, md = inst.schedule
        out.append((inst, MR.trajectory_metrics(P, inst.grid, inst.X, inst.U, ev, md, inst.tt, inst.ts)))
    return P, out


def _close(a, b, scale=None):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= REL * max(1.0, np.abs(b).max() if scale is None else scale)


def test_nodes_equal_node_performance_and_lq_node(cases):
    P, both = cases
    seen = set()
    for inst, m in both:
        ev, md = inst.schedule
        N = len(inst.grid) - 1
        assert np.abs(m["defect"]).max() > 0.02 and np.abs(m["eq"]).max() > 0.1          # a wrong sign or row order would vanish on a converged trajectory
        for k in range(N + 1):
            a = LSR.node_args(inst.grid, inst.X, inst.U, ev, md, inst.tt, inst.ts, k)
            c, d, e = LSR.node_performance(P, **a)
            dt = a["dt"]
            if k == N:
                assert _close(m["node_cost"][k], c) and d == 0.0 and e == 0.0
                assert not m["cost_terms"][k][[0, 1, 3, 4, 5, 6, 7]].any() and m["cost_terms"][k][2] == m["node_cost"][k]
                continue
            assert _close(dt * m["node_cost"][k], c) and _close(dt * m["defect"][k] @ m["defect"][k], d) and _close(dt * m["eq"][k] @ m["eq"][k], e), (k,)
            o = LR.lq_node(P, **a)
            nc = int(o["nc"])
            seen.add(nc)
            assert m["nc"][k] == nc and not m["eq"][k, nc:].any()
            assert _close(m["defect"][k], o["b"]) and _close(m["eq"][k, :nc], o["e"]), (k,)
            assert _close(dt * m["node_cost"][k], o["cost"])
            t = m["cost_terms"][k]
            assert m["node_cost"][k] == ((((((t[0] + t[1]) + t[2]) + t[3]) + t[4]) + t[5]) + t[6]) and t[6] == 0.0 and t[7] == 0.0
            assert (m["mag"]["defect"][k] >= np.abs(m["defect"][k])).all() and (m["mag"]["eq"][k] >= np.abs(m["eq"][k])).all()
            assert (m["mag"]["cost_terms"][k] >= np.abs(t) * (1 - 1e-12)).all()
    assert {12, 14} <= seen, seen


def test_totals_equal_ls_reference_performance(cases):
    P, both = cases
    for inst, m in both:
        ev, md = inst.schedule
        merit, viol = LSR.performance(P, inst.grid, inst.X, inst.U, ev, md, inst.tt, inst.ts)
        p = m["performance"]
        assert _close(p[0], merit) and p[1] == p[0] and _close(np.sqrt(p[3] + p[4]), viol)
        assert not p[[2, 5, 6, 7]].any()
        # the initial-state term: |x0 - X_0|^2 on top of the dynamics SSE, nothing else moves
        x0 = inst.X[0] + 0.1
        q = MR.trajectory_metrics(P, inst.grid, inst.X, inst.U, ev, md, inst.tt, inst.ts, x0=x0)["performance"]
        assert _close(q[3] - p[3], 30 * 0.01, scale=1.0) and q[4] == p[4] and q[0] == p[0]
