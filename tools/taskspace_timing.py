#!/usr/bin/env python3
"""Device time of qmgpu_mpc_taskspace_batch on the bench workload (256 instances x N = 100, trot: bench.py configs[1] inputs), at out_x / out_u of a solve.  The call
records nothing in the library's timing ring, so each call is timed by a pair of events on the handle's stream (the process's current stream); median / min / p90 of
repeated calls, with all nine outputs and with the four position outputs only (no U, no schedule: no velocity rows, no foothold phase), next to the metrics call's time
measured the same way in the same process.  No threshold: nobody has measured this number before.
Prints one JSON line; --out FILE also writes it there (profiles/taskspace_timing.json)."""
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
from qm_door_amd import abi, api  # noqa: E402
B, N, E = 256, 100, abi.MAX_EVENTS


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
sol.mpc(mb.args)
torch.cuda.synchronize()
f64 = dict(dtype=torch.float64, device="cuda")
pos = dict(feet_pos=torch.zeros((B, N + 1, 4, 3), **f64), ee_pos=torch.zeros((B, N + 1, 3), **f64), ee_quat=torch.zeros((B, N + 1, 4), **f64), com=torch.zeros((B, N + 1, 3), **f64))
rest = dict(feet_vel=torch.zeros((B, N, 4, 3), **f64), base_twist=torch.zeros((B, N, 6), **f64), cop=torch.zeros((B, N, 3), **f64),
            foothold_pos=torch.zeros((B, E, 4, 3), **f64), foothold_flag=torch.zeros((B, E, 4), dtype=torch.int32, device="cuda"))
every = sol.taskspace_args(B, N, mb.oT, mb.oX, U=mb.oU, sched_num=mb.sn, sched_times=mb.se, sched_modes=mb.sm, **pos, **rest)
positions = sol.taskspace_args(B, N, mb.oT, mb.oX, **pos)
mout = dict(node_cost=torch.zeros((B, N + 1), **f64), cost_terms=torch.zeros((B, N + 1, 8), **f64), defect=torch.zeros((B, N, 30), **f64), eq=torch.zeros((B, N, 16), **f64),
            nc=torch.zeros((B, N), dtype=torch.int32, device="cuda"), performance=torch.zeros((B, 8), **f64))
margs = sol.metrics_args(B, N, mb.oT, mb.oX, mb.oU, mb.tt, mb.ts, mb.sn, mb.se, mb.sm, x0=mb.x0, **mout)

t_every, t_pos, t_metrics = timed(lambda: sol.taskspace(every)), timed(lambda: sol.taskspace(positions)), timed(lambda: sol.metrics(margs))
assert all(bool(torch.isfinite(v).all()) for v in list(pos.values()) + [rest["feet_vel"], rest["base_twist"], rest["cop"], rest["foothold_pos"]])
landings = int(rest["foothold_flag"][0].sum())
# traffic per node, in doubles: x, u read; the 12 + 3 + 4 + 3 position entries and the 12 + 6 + 3 velocity entries written; per instance the 40 x 12 foothold entries and 40 x 4 flags
rec = dict(batch=B, N=N, calls=opt.calls, device=torch.cuda.get_device_name(0), taskspace_ms=t_every, taskspace_positions_only_ms=t_pos, metrics_ms_same_process=t_metrics,
           taskspace_over_metrics=t_every["median"] / t_metrics["median"], landings_per_instance=landings,
           bytes_per_node=dict(read=60 * 8, written=(22 + 21) * 8), bytes_per_instance_footholds=E * 12 * 8 + E * 4 * 4)
print(json.dumps(rec))
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    json.dump(rec, open(opt.out, "w"), indent=1)
