#!/usr/bin/env python3
"""HIP-event time of qmgpu_mpc_feedback_batch and qmgpu_policy_eval_feedback_batch on the bench workload (256 instances x N = 100, trot: bench.py configs[1]
inputs), warm, median of 100 calls each, and the gain kernel's achieved bandwidth against its compulsory traffic.
Prints one JSON line; --out FILE also writes it there (profiles/feedback_policy_timing.json)."""
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
sol.mpc(mb.args)
f64 = torch.float64
K = torch.zeros((B, N + 1, 30, 30), dtype=f64, device="cuda"); uff = torch.zeros((B, N + 1, 30), dtype=f64, device="cuda")
st = torch.zeros(B, dtype=torch.int32, device="cuda")
te = G.dev(np.full(B, 0.004), f64); xm = G.dev(sc["x0"], f64)
xo, uo, mo = torch.zeros((B, 30), dtype=f64, device="cuda"), torch.zeros((B, 30), dtype=f64, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")


def median_ms(call):
    for _ in range(5):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(opt.calls)]
    for a, b in ev:
        a.record(); call(); b.record()
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) for a, b in ev])
    return float(np.median(t)), float(t.min()), float(np.percentile(t, 90))


gain = median_ms(lambda: sol.mpc_feedback(B, N, mb.oX, mb.oU, K, uff, st))
pol = median_ms(lambda: sol.policy_eval_feedback(B, N, mb.oT, mb.oX, uff, K, mb.oM, te, xm, xo, uo, mo))
assert not st.cpu().numpy().any() and bool(torch.isfinite(K).all()) and bool(K.any())
# compulsory traffic per node, in doubles: Px and Pu joint rows 18 x 30 + 18 x 18 = 864, K~ 18 x 30 = 540, x and u 60, written K and uff 930
node_bytes = (864 + 540 + 60 + 930) * 8
gain_bytes = node_bytes * B * N
pol_bytes = B * (2 * 930 + 2 * 30 + 30 + 60) * 8
rec = dict(batch=B, N=N, calls=opt.calls, device=torch.cuda.get_device_name(0),
           feedback_gain_ms=dict(median=gain[0], min=gain[1], p90=gain[2]), feedback_gain_compulsory_GB=gain_bytes / 1e9, feedback_gain_TBps=gain_bytes / (gain[0] * 1e-3) / 1e12,
           policy_eval_feedback_ms=dict(median=pol[0], min=pol[1], p90=pol[2]), policy_eval_feedback_GB=pol_bytes / 1e9, policy_eval_feedback_TBps=pol_bytes / (pol[0] * 1e-3) / 1e12)
print(json.dumps(rec))
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    json.dump(rec, open(opt.out, "w"), indent=1)
