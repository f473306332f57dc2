"""CPU tier: wbc_report_kernel (kernels/wbc_report_kernel.h) on host threads (tests/emu) through qmgpu_wbc_report_batch: the cases of wbc_report_cases.py against
wbc_report_reference.py under its tolerance rule, the oracle-free checks and the contracts that need no GPU.  Fails without the feature: the emulated library has no
qmgpu_wbc_report_batch.  On this tier the x of a solved tick is the oracle's WBC solution of that tick (wbc_report_cases.Runner, own_solve: wbc_kernel on host threads
costs over a second per robot; the report is an evaluator and is compared at the x it was given); the solve - report - solve contract runs the library's own solve.
The GPU tier evaluates the library's own solutions.  The lock-step loop over qmgpu_cycle_batch runs on the GPU tier only."""
import ctypes
import os
import subprocess
import tempfile

import pytest

import support as S
import wbc_report_cases as WC
from qm_door_amd import abi, api


@pytest.fixture(scope="module")
def runner():
    itf = api.QMInterface(lib=abi.load_library(S.build_emu()))
    return WC.Runner(itf, S.Oracle(itf.problem), "emu", own_solve=False)


@pytest.mark.parametrize("case", list(WC.CASES))
def test_emu_wbc_report_case(runner, case):
    WC.CASES[case](runner)


def test_wbc_report_args_layout_matches_c():
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "qmgpu.h"
    int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(qmgpu_wbc_report_args), offsetof(qmgpu_wbc_report_args, x_stride),
                            offsetof(qmgpu_wbc_report_args, state_desired), offsetof(qmgpu_wbc_report_args, input_last), offsetof(qmgpu_wbc_report_args, x),
                            offsetof(qmgpu_wbc_report_args, active_tol), offsetof(qmgpu_wbc_report_args, eq_residual), offsetof(qmgpu_wbc_report_args, summary),
                            sizeof(qmgpu_wbc_task_rows), offsetof(qmgpu_wbc_task_rows, weight)); return 0; }
    '''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(S.ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        sizes = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).split()]
    T, R = abi.WbcReportArgs, abi.WbcTaskRows
    assert sizes == [ctypes.sizeof(T), T.x_stride.offset, T.state_desired.offset, T.input_last.offset, T.x.offset, T.active_tol.offset, T.eq_residual.offset,
                     T.summary.offset, ctypes.sizeof(R), R.weight.offset]
