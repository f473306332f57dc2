#!/usr/bin/env python3
"""HIP-event time of qmgpu_mpc_dual_batch on the bench workload (256 instances x N = 100, trot: bench.py configs[1] inputs), warm, median / min / p90 of repeated
calls, next to riccati_kernel's time (qmgpu_kernel_ms_mean[2]) measured in the same process.  costate_kernel is the call with the costates
alone; the call with nu and nc launches dual_multiplier_kernel behind it, whose time is reported as the difference of the two medians.
Prints one JSON line; --out FILE also writes it there (profiles/dual_timing.json)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import gpu_harness as G  # noqa: E402
from qm_door_amd import api  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--calls", type=int, default=100)
opt = ap.parse_args()

itf = api.QMInterface(); B, N = 256, 100
sc = bench.build_scenario(itf, B, 0)
sol = G.make_solver(itf, B, N)
sol.enable_debug(True)   # nu reads the LQ dump of the solve
mb = G.MpcBatch(sc["x0"], sc["tt"], sc["ts"], np.full(B, sc["nev"], dtype=np.int32), np.tile(sc["ev"], (B, 1)), np.tile(sc["md"], (B, 1)), N)
f64 = torch.float64
# the backward + forward sweep of the same workload, from the handle's own events
sol.enable_timing(True)
for _ in range(5 + opt.calls):
    sol.mpc(mb.args)
torch.cuda.synchronize()
hist = sol.kernel_ms_history(opt.calls)[:, 2]
sol.enable_timing(False)
sol.mpc(mb.args)
lam, nu = torch.zeros((B, N + 1, 30), dtype=f64, device="cuda"), torch.zeros((B, N, 16), dtype=f64, device="cuda")
nc, st = torch.zeros((B, N), dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")


def median_ms(call):
    for _ in range(5):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(opt.calls)]
    for a, b in ev:
        a.record(); call(); b.record()
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) for a, b in ev])
    return dict(median=float(np.median(t)), min=float(t.min()), p90=float(np.percentile(t, 90)))


cos = median_ms(lambda: sol.dual(B, N, lam, None, None, st))
both = median_ms(lambda: sol.dual(B, N, lam, nu, nc, st))
assert not st.cpu().numpy().any() and bool(torch.isfinite(lam).all()) and bool(torch.isfinite(nu).all()) and bool(lam.any()) and bool(nu.any())
# traffic per node, in doubles.  costate_kernel: the staged record, the gains and dx read, lambda written.  dual_multiplier_kernel: R, B, D, r of the dump, du and
# lambda_{k+1} read, nu written
cos_read, cos_written = 3316 + 560 + 30, 30
mul_read, mul_written = 900 + 900 + 480 + 30 + 30 + 30, 16
cos_bytes = (cos_read + cos_written) * 8 * B * N
rm = float(np.median(hist))
rec = dict(batch=B, N=N, calls=opt.calls, device=torch.cuda.get_device_name(0),
           costate_ms=cos, dual_ms=both, multiplier_ms_by_difference=both["median"] - cos["median"],
           riccati_ms=dict(median=rm, min=float(hist.min()), p90=float(np.percentile(hist, 90))),
           costate_over_riccati=cos["median"] / rm, dual_over_riccati=both["median"] / rm,
           costate_bytes_per_node=dict(read=cos_read * 8, written=cos_written * 8), costate_GB=cos_bytes / 1e9, costate_TBps=cos_bytes / (cos["median"] * 1e-3) / 1e12,
           multiplier_bytes_per_node=dict(read=mul_read * 8, written=mul_written * 8))
print(json.dumps(rec))
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    json.dump(rec, open(opt.out, "w"), indent=1)
