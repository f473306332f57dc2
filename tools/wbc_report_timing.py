#!/usr/bin/env python3
"""Device time of qmgpu_wbc_report_batch: 256 instances (the bench scenario's robots in the headline trot workload, the report of the WBC solution of one cycle), warm,
100 calls timed by a pair of events on the handle's stream (the call records nothing in the library's timing ring); qmgpu_wbc_solve_batch on the same inputs is timed
the same way in the same process.  The report does a strict subset of wbc_kernel's work (model, tasks, no QP): it has to come out cheaper, and the tool fails if it does not.
Prints one JSON line; --out FILE also writes it there (profiles/wbc_report_timing.json)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--calls", type=int, default=100)
opt = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import gpu_harness as G  # noqa: E402
from qm_door_amd import api  # noqa: E402
B, N = 256, 40


def stat(t):
    t = np.asarray(t)
    return dict(median=float(np.median(t)), min=float(t.min()), p90=float(np.percentile(t, 90)))


def timed(fn):
    """ms of each of opt.calls calls of fn, from event pairs on the current stream, after five warm-up calls"""
    for _ in range(5):
        fn()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(opt.calls)]
    for a, b in pairs:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return stat([a.elapsed_time(b) for a, b in pairs])


itf = api.QMInterface()
sc = bench.build_scenario(itf, B, 0)
sol = G.make_solver(itf, B, N)
mb = G.MpcBatch(sc["x0"], sc["tt"], sc["ts"], np.full(B, sc["nev"], dtype=np.int32), np.tile(sc["ev"], (B, 1)), np.tile(sc["md"], (B, 1)), N)
wb = G.WbcBatch(sc["rbd"], np.full(B, 0.002), np.full(B, 20.0), np.zeros((B, 30)))
t_eval = G.dev(np.zeros(B), torch.float64)
sol.cycle(mb.args, t_eval, wb.args)                       # one cycle: the plan whose policy the WBC tracks
torch.cuda.synchronize()
f64 = dict(dtype=torch.float64, device="cuda")
xd, ud, pm = torch.zeros((B, 30), **f64), torch.zeros((B, 30), **f64), torch.zeros(B, dtype=torch.int32, device="cuda")
sol.policy_eval(B, N, mb.oT, mb.oX, mb.oU, mb.oM, t_eval, xd, ud, pm)
il0 = torch.zeros((B, 30), **f64)                         # input_last of the tick: what the cycle's WBC started from
il = il0.clone()
wa = sol.wbc_args(B, wb.rbd, wb.period, wb.time, il, wb.out, wb.status, xd, ud, pm)


def solve():
    il.copy_(il0)                                         # every timed solve is the same tick (the copy is inside both the solve's and, below, the report's pair)
    sol.wbc(wa)


rec = dict(batch=B, calls=opt.calls, device=torch.cuda.get_device_name(0))
rec["wbc_solve_ms"] = timed(solve)
out = dict(eq_residual=torch.zeros((B, 3, 22), **f64), ineq_margin=torch.zeros((B, 56), **f64), tau=torch.zeros((B, 18), **f64),
           rows=torch.zeros((B, 4), dtype=torch.int32, device="cuda"), summary=torch.zeros((B, 12), **f64))
ra = sol.wbc_report_args(B, wb.rbd, wb.period, wb.time, il0, wb.out, xd, ud, pm, active_tol=1e-6, **out)


def report():
    il.copy_(il0)
    sol.wbc_report(ra)


rec["wbc_report_ms"] = timed(report)
rec["copy_ms"] = timed(lambda: il.copy_(il0))             # what both pairs contain besides their kernel
torch.cuda.synchronize()
assert bool(torch.isfinite(out["eq_residual"]).all()) and bool(torch.isfinite(out["tau"]).all())
assert float((out["tau"] - wb.out[:, 36:]).abs().max()) < 1e-9      # the report of the solve's own x commands the solve's torque
rec["level0_residual_inf_max"] = float(out["summary"][:, 3].max())
rec["min_margin"] = float(out["summary"][:, 6:8].min())
rec["report_over_solve"] = rec["wbc_report_ms"]["median"] / rec["wbc_solve_ms"]["median"]
print(json.dumps(rec))
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    json.dump(rec, open(opt.out, "w"), indent=1)
assert rec["report_over_solve"] < 1.0, "the report must be cheaper than the solve it reports on"
