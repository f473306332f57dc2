#!/usr/bin/env python3
"""HIP-event time of qmgpu_mpc_value_function_batch and qmgpu_value_function_eval_batch on the bench workload (256 instances x N = 100, trot: bench.py configs[1]
inputs), warm, median / min / p90 of repeated calls, next to riccati_kernel's time (qmgpu_kernel_ms_mean[2]) measured in the same process: the value-function
kernel streams the same records through the same dependent chain without the factorisation.
Prints one JSON line; --out FILE also writes it there (profiles/value_function_timing.json)."""
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
z = lambda *shape: torch.zeros(shape, dtype=f64, device="cuda")  # noqa: E731
Sm, Sv, sl, xl = z(B, N + 1, 30, 30), z(B, N + 1, 30), z(B, N + 1, 30), z(B, N + 1, 30)
st = torch.zeros(B, dtype=torch.int32, device="cuda")
te = G.dev(np.full(B, 0.004), f64); xm = G.dev(sc["x0"], f64)
g, H = z(B, 30), z(B, 30, 30)


def median_ms(call):
    for _ in range(5):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(opt.calls)]
    for a, b in ev:
        a.record(); call(); b.record()
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) for a, b in ev])
    return dict(median=float(np.median(t)), min=float(t.min()), p90=float(np.percentile(t, 90)))


val = median_ms(lambda: sol.mpc_value_function(B, N, Sm, Sv, sl, xl, st))
evl = median_ms(lambda: sol.value_function_eval(B, N, mb.oT, Sm, Sv, te, xm, g, H))
assert not st.cpu().numpy().any() and bool(torch.isfinite(Sm).all()) and bool(Sm.any())
# traffic per node, in doubles: the staged record and the gains read, x_lin read, Sm + Sv + sv_lin + x_lin written
node_doubles_read, node_doubles_written = 3316 + 560 + 30, 900 + 3 * 30
val_bytes = (node_doubles_read + node_doubles_written) * 8 * B * N
rec = dict(batch=B, N=N, calls=opt.calls, device=torch.cuda.get_device_name(0),
           value_function_ms=val, riccati_ms=dict(median=float(np.median(hist)), min=float(hist.min()), p90=float(np.percentile(hist, 90))),
           value_function_over_riccati=val["median"] / float(np.median(hist)),
           value_function_bytes_per_node=dict(read=node_doubles_read * 8, written=node_doubles_written * 8), value_function_GB=val_bytes / 1e9,
           value_function_TBps=val_bytes / (val["median"] * 1e-3) / 1e12, value_function_eval_ms=evl)
print(json.dumps(rec))
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    json.dump(rec, open(opt.out, "w"), indent=1)
