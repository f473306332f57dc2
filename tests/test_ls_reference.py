"""CPU tier of the line-search pin: the numpy reference of the filter line search and the convergence test (ls_reference.py) against itself, its branches on
hand-made numbers, the coverage and margin conditions of every scenario of ls_scenarios.py, and then the oracle and the host-emulated kernels against it."""
import json
import os

import mpmath as mp
import numpy as np
import pytest

import lq_reference as LR
import lq_scenarios as LQS
import ls_reference as LSR
import ls_scenarios as L
import support as S
from qm_door_amd import abi, api

STEP_ERRORS = os.path.join(S.ROOT, "tests", "golden", "ls_oracle_step_errors.json")     # e_orc per case: the oracle's step error against the reference's direction


def _recorded():
    return json.load(open(STEP_ERRORS))


# ------------------------------------------------------------------------------------------------ (a) the reference against itself
@pytest.mark.parametrize("name", list(LQS.BUILDERS))
def test_node_performance_equals_the_lq_node_it_restates(interface, name):
    """cost, dt |b|^2 and dt |e|^2 of lq_reference.lq_node (the path pinned in 50 digits) at every checked node of the LQ scenarios"""
    sc, ref, _ = LQS.scenario(interface, name)
    P = LSR.Params(LQS.interface_of(interface, name).problem.settings)
    for (i, k), r in ref.items():
        a = sc.node(i, k)
        c, d, e = LSR.node_performance(P, **a)
        assert abs(c - r["cost"]) <= 1e-13 * max(1.0, abs(r["cost"])), (name, i, k, c, r["cost"])
        if not a["terminal"]:
            for got, want in ((d, a["dt"] * r["b"] @ r["b"]), (e, a["dt"] * r["e"] @ r["e"])):
                assert abs(got - want) <= 1e-13 * max(1.0, abs(want)), (name, i, k, got, want)


# ------------------------------------------------------------------------------------------------ (b) every branch and boundary on hand-made numbers
class _P:
    g_max, g_min, alpha_min, alpha_decay, gamma_c, armijo_factor, cost_tol, delta_tol, sqp_iterations = 1.0, 0.1, 0.2, 0.5, 0.25, 0.5, 0.5, 0.05, 3


def test_accept_step_branches_and_boundaries():
    A = lambda base, trial, aa, on=True: LSR.accept_step(_P, base, trial, aa, on)  # noqa: E731
    assert A((5.0, 4.0), (9.0, 2.9), -1.0) == (True, 1) and A((5.0, 4.0), (0.0, 3.0), -1.0) == (False, 1)          # type 1: v1 < (1 - gamma_c) v0 = 3, strict; the merit is not looked at
    assert A((5.0, 4.0), (0.0, 1.0), -1.0)[1] == 2                                                                   # v1 == g_max is not above it
    assert A((5.0, 0.05), (4.4, 0.05), -1.0) == (True, 3) and A((5.0, 0.05), (4.5, 0.05), -1.0) == (False, 3)        # type 3: m1 < m0 + armijo_factor alpha armijo = 4.5, strict
    assert A((5.0, 0.05), (4.4, 0.1), -1.0)[1] == 2 and A((5.0, 0.1), (4.4, 0.05), -1.0)[1] == 2                     # v == g_min is not below it
    assert A((5.0, 0.05), (4.4, 0.05), 0.0)[1] == 2 and A((5.0, 0.05), (4.4, 0.05), 1.0)[1] == 2                     # no descent: type 2
    assert A((5.0, 0.5), (4.87, 0.9), -1.0) == (True, 2) and A((5.0, 0.5), (4.875, 0.9), -1.0) == (False, 2)         # merit clause: m1 < m0 - gamma_c v0 = 4.875, strict
    assert A((5.0, 0.5), (9.0, 0.37), -1.0) == (True, 2) and A((5.0, 0.5), (9.0, 0.375), -1.0) == (False, 2)         # violation clause: v1 < 0.375, strict
    assert A((5.0, 0.4), (9.0, 9.0), 1.0, on=False) == (True, 0)
    log = []
    LSR.accept_step(_P, (5.0, 0.5), (4.0, 0.9), -1.0, True, log)
    assert log == [(1.0, 0.9), (0.9, 0.1), (4.0, 4.875), (0.9, 0.375)]                                   # what was evaluated, as (lhs, rhs) of lhs < rhs


def test_line_search_loop_and_its_end():
    base = (5.0, 4.0)
    perf = lambda a: (9.0, 8.0 if a > 0.3 else 2.0)  # noqa: E731
    r = LSR.line_search(_P, perf, base, -1.0)
    assert (r["alpha"], r["type"], r["merit"], r["violation"]) == (0.25, 1, 9.0, 2.0) and [t[:3] for t in r["trail"]] == [(1.0, 1, False), (0.5, 1, False), (0.25, 1, True)]
    r = LSR.line_search(_P, lambda a: (9.0, 8.0), base, -1.0)
    assert (r["alpha"], r["type"], r["merit"], r["violation"]) == (0.0, 4, 5.0, 4.0) and [t[0] for t in r["trail"]] == [1.0, 0.5, 0.25]   # 0.125 < alpha_min: not tried
    _P2 = type("P2", (_P,), dict(alpha_min=0.25))
    assert [t[0] for t in LSR.line_search(_P2, lambda a: (9.0, 8.0), base, -1.0)["trail"]] == [1.0, 0.5, 0.25]                             # alpha == alpha_min is tried
    _P3 = type("P3", (_P,), dict(alpha_min=0.6))
    assert LSR.line_search(_P3, perf, base, -1.0)["alpha"] == 0.0 and len(LSR.line_search(_P3, perf, base, -1.0)["trail"]) == 1
    assert LSR.line_search(_P, lambda a: (9.0, 8.0), base, -1.0, on=False)["type"] == 0


def test_check_convergence_reasons_precedence_and_boundaries():
    C = lambda it, al, m0, m1, v1, dx, du: LSR.check_convergence(_P, it, al, m0, m1, v1, dx, du)[0]  # noqa: E731
    assert C(2, 0.0, 5.0, 5.0, 0.0, 0.0, 0.0) == 1 and C(1, 1.0, 5.0, 4.0, 1.0, 1.0, 1.0) == 0          # iteration + 1 >= sqp_iterations
    assert C(0, 0.1, 5.0, 5.0, 0.0, 0.0, 0.0) == 2 and C(0, 0.2, 5.0, 4.0, 1.0, 1.0, 1.0) == 0          # 2 over 3 over 4; alpha == alpha_min is no stop
    assert C(0, 1.0, 5.0, 5.25, 0.05, 0.0, 0.0) == 3                                                   # 3 over 4
    assert C(0, 1.0, 5.0, 5.5, 0.05, 1.0, 1.0) == 0 and C(0, 1.0, 5.0, 5.25, 0.1, 1.0, 1.0) == 0      # both parts of 3 are strict
    assert C(0, 0.5, 5.0, 4.0, 1.0, 0.09, 0.09) == 4 and C(0, 0.5, 5.0, 4.0, 1.0, 0.1, 0.09) == 0 and C(0, 0.5, 5.0, 4.0, 1.0, 0.09, 0.1) == 0
    assert LSR.convergence_conditions(_P, 0, 0.1, 5.0, 5.0, 0.05, 0.0, 0.0) == {1: False, 2: True, 3: True, 4: True}
    assert LSR.margin([(1.0, 1.0 + 1e-7), (0.0, 1e-4)]) < 1e-6 <= LSR.margin([(1.0, 1.0 + 2e-6), (0.0, 1e-4)])


def test_projected_armijo_metric_equals_the_explicit_projection(interface):
    """ls_reference.armijo_metric(projected = True) against upstream's procedure carried out step by step on the reference's blocks of an infeasible trot iterate:
    QR of D' (qrConstraintProjection: Pu the null-space basis, Px = -D^+ C, Pe = -D^+ e), the projected cost q~ = q + Px'(r + R Pe), r~ = Pu'(r + R Pe)
    (changeOfInputVariables), the projected input step du~ = Pu'(du - Pe - Px dx), and sum q~.dx + r~.du~ (armijoDescentMetric before remapProjectedInput).
    The upstream solver's sources are not part of the reference tree this project was modelled on; the procedure is restated from its documented steps."""
    case = L.cases(interface, "backoff_two_trials")[0]
    inst, r = case.instances[1], L.references(interface, case)[1]
    blocks, dX, dU = L.reference_blocks(L.base_params(interface), inst), r["d"]["dX"], r["d"]["dU"]
    total = float(blocks[-1]["q"] @ dX[-1])
    for k, o in enumerate(blocks[:-1]):
        nc = o["nc"]
        Qf, Rf = np.linalg.qr(o["D"][:nc].T, mode="complete")
        Q1, Pu, R1 = Qf[:, :nc], Qf[:, nc:], Rf[:nc]
        Pe, Px = -Q1 @ np.linalg.solve(R1.T, o["e"][:nc]), -Q1 @ np.linalg.solve(R1.T, o["C"][:nc])
        assert np.abs(o["D"][:nc] @ Pe + o["e"][:nc]).max() <= 1e-12 and np.abs(o["D"][:nc] @ Pu).max() <= 1e-12
        dut = Pu.T @ (dU[k] - Pe - Px @ dX[k])
        assert np.abs(Pe + Px @ dX[k] + Pu @ dut - dU[k]).max() <= 1e-9 * max(1.0, np.abs(dU[k]).max())      # the step meets the linearised rows
        w = o["r"] + o["R"] @ Pe
        total += float((o["q"] + Px.T @ w) @ dX[k] + (Pu.T @ w) @ dut)
    assert abs(total - r["armijo"]) <= 1e-12 * abs(r["armijo"]), (total, r["armijo"])
    assert abs(r["armijo"] - r["armijo_unprojected"]) > 1e-4 * abs(r["armijo"])          # the two forms do differ here


# ------------------------------------------------------------------------------------------------ (c) coverage and margin of every scenario
CPU_SCENARIOS = [n for n in L.BUILDERS if n != "backoff_hbm_scratch"]      # (N = 300 takes its direction from the solver's dump: its conditions are asserted in (d), (e) and the GPU tier)


@pytest.mark.parametrize("name", CPU_SCENARIOS)
def test_scenario_reaches_its_branch_with_margin(interface, name):
    """on the reference alone: every instance reaches what it is named for, and no comparison of its filter and convergence test is within 1e-6 (fp32 leg: 1e-3)"""
    for case in L.cases(interface, name):
        refs = L.references(interface, case)
        print(case.name, f"reference {sum(r['seconds'] for r in refs):.1f} s", [(r["ls"]["alpha"], r["ls"]["type"], r["reason"]) for r in refs])
        L.assert_conditions(interface, case, refs, L.FP32_MARGIN if name in L.FP32_SCENARIOS else L.MARGIN)
    if name == "alpha_min_stops":       # what the two stopped instances would have taken: alpha 1/4 and alpha 1/2 (the same inputs in backoff_two_trials)
        ladder = L.references(interface, L.cases(interface, "backoff_two_trials")[0])
        assert ladder[2]["ls"]["alpha"] == 0.25 and ladder[1]["ls"]["alpha"] == 0.5
    if name == "line_search_off":
        assert not L.references(interface, L.cases(interface, "backoff_two_trials")[0])[2]["ls"]["trail"][0][2]


# ------------------------------------------------------------------------------------------------ the violation of the reference in 50 digits
def _violation_50_digits(P, inst, X, U):
    from test_lq_reference import MpModel

    class OneSided(MpModel):
        """MpModel differentiates the swing spline by a CENTRAL difference in time; on a node that lies ON an event time (t = 0.03 = 2 dt is the lift-off of these
        schedules) the backward point falls into the stance phase in front of it, where the leg has no swing reference (lq_reference.swing_z asserts).  The velocity
        reference of such a node is the derivative of the phase that STARTS there: a forward difference, step 1e-20 in 50 digits (error 1e-20 |z''|)."""
        def swing(self, a, leg):
            from test_lq_reference import _MpSettings
            f = lambda t: LR.swing_z(_MpSettings(self.P), [mp.mpf(float(e)) for e in a["events"]], a["modes"], leg, t)  # noqa: E731
            t = mp.mpf(float(a["t"]))
            return f(t), (f(t + self.STEP) - f(t)) / self.STEP
    M = OneSided(P)
    ev, md = inst.schedule
    total = mp.mpf(0)
    for k in range(len(inst.grid) - 1):
        a = LSR.node_args(inst.grid, X, U, ev, md, inst.tt, inst.ts, k)
        v = M.values(np.concatenate([M.vec(a["x"]), M.vec(a["u"])]), a)
        nc = len(v) - 36
        d = v[:30] - M.vec(a["xnext"])
        total += mp.mpf(float(a["dt"])) * (sum(x * x for x in d) + sum(x * x for x in v[30:30 + nc]))
    return mp.sqrt(total)


def test_violation_of_the_reference_in_50_digits(interface):
    """THE SLOW TEST of this file (about 10 s): the float64 violation of ls_reference.performance against the same sums in 50-digit mpmath (test_lq_reference.MpModel:
    flow map, RK2 map and equality rows restated), at the standing iterate of type3_armijo (where the violation is rounding and the defect b cancels) and at the
    accepted trial of backoff_two_trials' instance 1 (trot, a node on the lift-off event, swing rows).  The violation bound of the product
    (ls_scenarios.violation_bound) is 10 x these errors; the recorded figures must hold."""
    mp.mp.dps = 50
    case3, caseb = L.cases(interface, "type3_armijo")[2], L.cases(interface, "backoff_two_trials")[0]
    feas, r3 = case3.instances[0], L.references(interface, case3)[0]
    v64 = r3["base"][1]
    v50 = _violation_50_digits(L.case_params(interface, case3), feas, feas.X, feas.U)
    e_feas = abs(float(mp.mpf(v64) - v50))
    inst, r = caseb.instances[1], L.references(interface, caseb)[1]
    assert r["ls"]["alpha"] == 0.5
    w50 = _violation_50_digits(L.base_params(interface), inst, r["X"], r["U"])
    e_back = abs(float((mp.mpf(r["ls"]["violation"]) - w50) / w50))
    print(f"standing iterate: v64 {v64:.3e} v50 {float(v50):.3e} |v64 - v50| {e_feas:.1e};  backoff trial: v64 {r['ls']['violation']:.6e} relative error {e_back:.1e}")
    assert e_feas <= L.VIOLATION_ERRORS["feasible_abs"] and e_back <= L.VIOLATION_ERRORS["backoff_rel"], (e_feas, e_back)


# ------------------------------------------------------------------------------------------------ (d) the oracle, (e) the host-emulated kernels
def _oracle_outcome(interface, case, warm=None):
    orc = S.Oracle(L.interface_of(interface, case).problem)
    X, U = (case.X, case.U) if warm is None else warm
    uniq = {}
    for i, j in enumerate(case.layout):
        if j not in uniq or warm is not None:
            uniq[j] = orc.mpc_solve(case.N, 0.0, case.x0[i], case.tt[i], case.ts[i], int(case.nev[i]), case.ev[i], case.md[i], warm=(X[i], U[i]), line_search=case.line_search)
    each = [uniq[j] for j in case.layout]
    return {k: np.stack([r[k] for r in each]) for k in ("T", "X", "U", "mode", "stats")}, orc


def _oracle_blocks(orc, case):
    import kkt_reference as KR
    return lambda i: KR.oracle_blocks(orc, case.grid[i], case.X[i], case.U[i], int(case.nev[i]), case.ev[i], case.md[i], case.tt[i], case.ts[i])


def _step_error(case, refs, out):
    import kkt_reference as KR
    e = [0.0, 0.0]
    for i, j in enumerate(case.layout):
        a = refs[j]["ls"]["alpha"]
        if a > 0.0 and refs[j]["reason"] != 0:
            e = [max(e[0], KR.rel_err(out["X"][i] - case.X[i], a * refs[j]["d"]["dX"])), max(e[1], KR.rel_err(out["U"][i] - case.U[i], a * refs[j]["d"]["dU"]))]
    return e


@pytest.mark.parametrize("name", list(L.BUILDERS))
def test_oracle_equals_the_reference(interface, name):
    """the oracle's iteration of every scenario; its step error against the reference's direction is e_orc of the tolerance rule: measured here, and recorded in
    tests/golden/ls_oracle_step_errors.json for the GPU tier, which has no oracle (LS_RECORD=1 rewrites the record; otherwise what is measured must not exceed it)"""
    worst = {}
    rec = _recorded() if os.path.exists(STEP_ERRORS) else {}
    for case in L.cases(interface, name):
        out, orc = _oracle_outcome(interface, case)
        refs = L.references(interface, case, _oracle_blocks(orc, case))
        if case.direction == "dump":
            L.assert_conditions(interface, case, refs)
        e = _step_error(case, refs, out)
        if os.environ.get("LS_RECORD"):
            rec[case.name] = e
            json.dump(rec, open(STEP_ERRORS, "w"), indent=1, sort_keys=True)
        assert e[0] <= rec[case.name][0] and e[1] <= rec[case.name][1], (case.name, e, rec[case.name])
        L.check_outcome(case, refs, out, "oracle", e_orc=rec[case.name], worst=worst)
        if name == "across_calls":
            out_b, _ = _oracle_outcome(interface, case, warm=(out["X"], out["U"]))
            L.check_across_calls(case, refs, out, out_b, "oracle", worst)
    print("oracle", name, {k: f"{v:.1e}" for k, v in worst.items()}, "(in units of each bound)")


@pytest.fixture(scope="module")
def emu():
    return api.QMInterface(lib=abi.load_library(S.build_emu()))


@pytest.mark.parametrize("name", list(L.BUILDERS))
def test_emulated_kernels_equal_the_reference(interface, emu, name):
    """linesearch_kernel (and the chain in front of it) on host threads; the 300-instance cases cut to 8 instances (ls_scenarios.host_sized) with QMGPU_EMU_CUS = 2, so that the 128-thread launch is taken"""
    worst, worst32, rec = {}, {}, _recorded()
    for case in map(L.host_sized, L.cases(interface, name)):
        dump = case.direction == "dump"
        out, sol = L.solve_host(emu, case, debug=dump)
        refs = L.references(interface, case, L.dump_blocks(sol, case) if dump else None)
        if dump:
            L.assert_conditions(interface, case, refs)
        if name in L.FP32_SCENARIOS:
            out32, sol32 = L.solve_host(emu, case, dtype="f32")
            L.check_outcome(case, refs, out32, "emulation fp32", fp32=True, worst=worst32)
            sol32.close()
        L.check_outcome(case, refs, out, "emulation", e_orc=rec[case.name], worst=worst)
        if name == "across_calls":
            out_b, _ = L.solve_host(emu, case, warm=(out["X"], out["U"]))
            L.check_across_calls(case, refs, out, out_b, "emulation", worst)
        sol.close()
    print("emulation", name, {k: f"{v:.1e}" for k, v in worst.items()}, "fp32", {k: f"{v:.1e}" for k, v in worst32.items()}, "(in units of each bound)")
