#!/usr/bin/env python3
"""Device time of qmgpu_plant_step_batch: 256 instances (the bench scenario's robots, standing, under the torques of one WBC call), substeps 1 and 10, warm, 100 calls
each timed by a pair of events on the handle's stream (the call records nothing in the library's timing ring); wbc_kernel on the same robots is timed the same way in the
same process, for scale.  No threshold: nobody has measured this number before.
Prints one JSON line; --out FILE also writes it there (profiles/plant_timing.json)."""
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
sol.cycle(mb.args, t_eval, wb.args)                       # one cycle: the policy buffers, the contact modes and the torques the plant is driven with
torch.cuda.synchronize()
f64 = dict(dtype=torch.float64, device="cuda")
tau = wb.out[:, 36:].contiguous()
mode = mb.oM[:, 0].contiguous()
dt = torch.full((B,), 0.002, **f64)
out = dict(rbd_next=torch.zeros((B, 55), **f64), contact_force=torch.zeros((B, 12), **f64), tau_applied=torch.zeros((B, 18), **f64), status=torch.zeros(B, dtype=torch.int32, device="cuda"))
kd = torch.tensor(np.tile(np.r_[np.full(12, 3.0), np.full(6, 0.5)], (B, 1)), **f64)
vel_des = torch.zeros((B, 18), **f64)
rec = dict(batch=B, calls=opt.calls, device=torch.cuda.get_device_name(0))
for S in (1, 10):
    a = sol.plant_args(B, wb.rbd, tau, mode, dt, substeps=S, vel_des=vel_des, kd=kd, **out)
    rec["plant_substeps%d_ms" % S] = timed(lambda: sol.plant_step(a))
    assert bool(torch.isfinite(out["rbd_next"]).all()) and not bool((out["status"] & 1).any())
# wbc_kernel alone on the same robots (policy evaluation of the cycle above as its desired state and input)
xd, ud, pm = torch.zeros((B, 30), **f64), torch.zeros((B, 30), **f64), torch.zeros(B, dtype=torch.int32, device="cuda")
sol.policy_eval(B, N, mb.oT, mb.oX, mb.oU, mb.oM, t_eval, xd, ud, pm)
wa = sol.wbc_args(B, wb.rbd, wb.period, wb.time, wb.il, wb.out, wb.status, xd, ud, pm)
rec["wbc_ms_same_process"] = timed(lambda: sol.wbc(wa))
rec["plant_substep_ms"] = (rec["plant_substeps10_ms"]["median"] - rec["plant_substeps1_ms"]["median"]) / 9.0
rec["plant1_over_wbc"] = rec["plant_substeps1_ms"]["median"] / rec["wbc_ms_same_process"]["median"]
print(json.dumps(rec))
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    json.dump(rec, open(opt.out, "w"), indent=1)
