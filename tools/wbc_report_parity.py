#!/usr/bin/env python3
"""Accuracy record of qmgpu_wbc_report_batch: runs the comparison cases of tests/wbc_report_cases.py (every contact mode, both variants, both task sets at the solver's
own x and at a random x; robots whose torque limits cannot hold; the lock-step ticks on the device) against tests/wbc_report_reference.py and records, per case and per
output, the kernel's worst error as a fraction of its bound, and the worst fraction overall.  Sections: "mi355x" on a machine with a GPU, "emu" (the host emulation
build) with --emu.  Writes --out (default profiles/wbc_report_parity.json); fails if a fraction exceeds 1."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--emu", action="store_true")
opt = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out = os.path.abspath(opt.out or os.path.join(ROOT, "profiles", "wbc_report_parity.json"))
os.environ["WBC_REPORT_RECORD"] = out
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import support as S  # noqa: E402
import wbc_report_cases as WC  # noqa: E402
from qm_door_amd import abi, api  # noqa: E402

if opt.emu:
    itf = api.QMInterface(lib=abi.load_library(S.build_emu()))
    runner = WC.Runner(itf, S.Oracle(itf.problem), "emu", own_solve=False)
else:
    import gpu_harness as G
    itf = api.QMInterface()
    runner = WC.Runner(itf, S.Oracle(itf.problem), "mi355x", to_dev=lambda a: G.dev(a), to_host=lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.array(t),
                       make_solver=lambda B, N=4, dtype="f64": G.make_solver(itf, B, N, dtype=dtype))
for case in ("modes_variants", "arbitrary_x", "binding_limits", "ee_force"):
    WC.CASES[case](runner)
if not opt.emu:
    WC.lock_step(runner)
rec = json.load(open(out))
print(json.dumps(dict(out=out, worst_fraction_of_bound=rec["worst_fraction_of_bound"])))
assert rec["worst_fraction_of_bound"] <= 1.0
