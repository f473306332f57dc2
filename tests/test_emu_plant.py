"""CPU tier: plant_kernel (kernels/plant_kernel.h) on host threads (tests/emu) through qmgpu_plant_step_batch: the cases of plant_cases.py against plant_reference.py under
its tolerance rule, the oracle-free checks, and the contracts that need no GPU.  Fails without the feature: the emulated library has no qmgpu_plant_step_batch.
The lock-step loop runs on the GPU tier only (twenty ticks of MPC policy, WBC and plant on host threads do not fit this tier's seconds)."""
import ctypes
import os
import subprocess
import tempfile

import pytest

import plant_cases as PC
import support as S
from qm_door_amd import abi, api


@pytest.fixture(scope="module")
def runner():
    itf = api.QMInterface(lib=abi.load_library(S.build_emu()))
    return PC.Runner(itf, S.Oracle(itf.problem), "emu")


@pytest.mark.parametrize("case", list(PC.CASES))
def test_emu_plant_case(runner, case):
    PC.CASES[case](runner)


def test_plant_args_layout_matches_c():
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "qmgpu.h"
    int main(void) { printf("%zu %zu %zu %zu %zu\n", sizeof(qmgpu_plant_args), offsetof(qmgpu_plant_args, rbd), offsetof(qmgpu_plant_args, mode),
                            offsetof(qmgpu_plant_args, rbd_next), offsetof(qmgpu_plant_args, status)); return 0; }
    '''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(S.ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        sizes = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).split()]
    T = abi.PlantArgs
    assert sizes == [ctypes.sizeof(T), T.rbd.offset, T.mode.offset, T.rbd_next.offset, T.status.offset]
