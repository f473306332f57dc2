"""-m gpu: linesearch_kernel on the device against the numpy reference of the filter line search and the convergence test (ls_reference.py), which shares no code
with the oracle or the kernels, over the scenarios of ls_scenarios.py: alpha, step type, iteration count and convergence reason exactly, the step against alpha times
the reference's direction, merits, Armijo metric and violations under the bounds of ls_scenarios.check_outcome.  No oracle anywhere in this file: e_orc of the step
tolerance rule is the CPU tier's record (tests/golden/ls_oracle_step_errors.json).  The reference's share of each test (host time) is printed.
fp32 leg (backoff_two_trials, type1_constraint; 1e-3 margin asserted by the CPU tier): the discrete outcomes equal, merits and violations within 1e-4."""
import json
import os

import pytest

import ls_scenarios as L

pytestmark = pytest.mark.gpu
RECORD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ls_oracle_step_errors.json")))


def _check(interface, name):
    import gpu_harness as G
    worst, worst32, seconds = {}, {}, 0.0
    for case in L.cases(interface, name):
        dump = case.direction == "dump"
        out, sol = L.solve_device(G, interface, case, debug=dump)
        refs = L.references(interface, case, L.dump_blocks(sol, case) if dump else None)
        if dump:
            L.assert_conditions(interface, case, refs)
        if name in L.FP32_SCENARIOS:
            out32, sol32 = L.solve_device(G, interface, case, dtype="f32")
            L.check_outcome(case, refs, out32, "gpu fp32", fp32=True, worst=worst32)
            sol32.close()
        seconds += sum(r["seconds"] for r in refs)
        L.check_outcome(case, refs, out, "gpu", e_orc=RECORD[case.name], worst=worst)
        if name == "across_calls":
            out_b, sol_b = L.solve_device(G, interface, case, warm=(out["X"], out["U"]))
            L.check_across_calls(case, refs, out, out_b, "gpu", worst)
            sol_b.close()
        sol.close()
    print("gpu", name, f"reference {seconds:.1f} s;", {k: f"{v:.1e}" for k, v in worst.items()}, "fp32", {k: f"{v:.1e}" for k, v in worst32.items()}, "(in units of each bound)")


def test_backoff_two_trials(interface):
    _check(interface, "backoff_two_trials")


def test_backoff_one_trial(interface):
    _check(interface, "backoff_one_trial")


def test_backoff_hbm_scratch(interface):
    _check(interface, "backoff_hbm_scratch")


def test_backoff_128_threads(interface):
    _check(interface, "backoff_128_threads")


def test_type1_constraint(interface):
    _check(interface, "type1_constraint")


def test_type3_armijo(interface):
    _check(interface, "type3_armijo")


def test_type2_either_clause(interface):
    _check(interface, "type2_either_clause")


def test_alpha_min_stops(interface):
    _check(interface, "alpha_min_stops")


def test_dense_weights(interface):
    _check(interface, "dense_weights")


def test_line_search_off(interface):
    _check(interface, "line_search_off")


def test_convergence_reasons(interface):
    _check(interface, "convergence_reasons")


def test_across_calls(interface):
    _check(interface, "across_calls")
