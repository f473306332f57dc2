"""GPU tier: plant_kernel on the device through qmgpu_plant_step_batch: the cases of plant_cases.py against plant_reference.py under its tolerance rule, the oracle-free
checks, the contracts, and the lock-step loop (MPC once, then policy evaluation -> WBC -> plant per tick, every tick compared on its own).  Fails without the feature:
the library has no qmgpu_plant_step_batch."""
import numpy as np
import pytest

import plant_cases as PC
import support as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runner():
    import torch
    import gpu_harness as G
    from qm_door_amd import api
    itf = api.QMInterface()
    to_host = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.array(t)  # noqa: E731
    make = lambda B, N=4, dtype="f64", itf_=None, **kw: G.make_solver(kw.get("itf") or itf_ or itf, B, N, dtype=dtype)  # noqa: E731
    return PC.Runner(itf, S.Oracle(itf.problem), "mi355x", to_dev=lambda a: G.dev(a), to_host=to_host, make_solver=make)


@pytest.mark.parametrize("case", list(PC.CASES))
def test_gpu_plant_case(runner, case):
    PC.CASES[case](runner)


def test_gpu_plant_lock_step(runner):
    PC.lock_step(runner)
