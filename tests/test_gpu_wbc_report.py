"""GPU tier: wbc_report_kernel on the device through qmgpu_wbc_report_batch: the cases of wbc_report_cases.py against wbc_report_reference.py under its tolerance rule,
the oracle-free checks, the contracts, and the lock-step check (three ticks of qmgpu_cycle_batch for eight robots with a report of each tick's out, each tick compared on
its own).  Fails without the feature: the library has no qmgpu_wbc_report_batch."""
import numpy as np
import pytest

import support as S
import wbc_report_cases as WC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runner():
    import gpu_harness as G
    from qm_door_amd import api
    itf = api.QMInterface()
    to_host = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.array(t)  # noqa: E731
    make = lambda B, N=4, dtype="f64": G.make_solver(itf, B, N, dtype=dtype)  # noqa: E731
    return WC.Runner(itf, S.Oracle(itf.problem), "mi355x", to_dev=lambda a: G.dev(a), to_host=to_host, make_solver=make)


@pytest.mark.parametrize("case", list(WC.CASES))
def test_gpu_wbc_report_case(runner, case):
    WC.CASES[case](runner)


def test_gpu_wbc_report_lock_step(runner):
    WC.lock_step(runner)
