#!/usr/bin/env python3
"""Device time of qmgpu_mpc_metrics_batch on the bench workload (256 instances x N = 100, trot: bench.py configs[1] inputs), from the library's own HIP events
(qmgpu_enable_timing: a timed metrics call fills slot [5] of its six durations), median / min / p90 of repeated calls at out_x / out_u of a solve, next to
linesearch_kernel's time of the same batch (qmgpu_kernel_ms_mean[3]) measured in the same process, and -- with --parent-tree, a built checkout of the parent
commit -- the parent's linesearch_kernel time read the same way by a child process that imports that checkout (--root, --linesearch-only).
Prints one JSON line; --out FILE also writes it there (profiles/metrics_timing.json)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--parent-tree", help="a built checkout of the parent commit: its linesearch_kernel time is recorded too")
ap.add_argument("--root", help="the checkout to import (default: the one this file lies in)")
ap.add_argument("--linesearch-only", action="store_true", help="print linesearch_kernel's time as one JSON line and stop")
opt = ap.parse_args()

ROOT = os.path.abspath(opt.root) if opt.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import gpu_harness as G  # noqa: E402
from qm_door_amd import api  # noqa: E402
B, N = 256, 100


def stat(t):
    t = np.asarray(t)
    return dict(median=float(np.median(t)), min=float(t.min()), p90=float(np.percentile(t, 90)))


def solver_and_batch(itf):
    sc = bench.build_scenario(itf, B, 0)
    sol = G.make_solver(itf, B, N)
    return sc, sol, G.MpcBatch(sc["x0"], sc["tt"], sc["ts"], np.full(B, sc["nev"], dtype=np.int32), np.tile(sc["ev"], (B, 1)), np.tile(sc["md"], (B, 1)), N)


def linesearch_ms(sol, mb):
    sol.enable_timing(True)
    for _ in range(5 + opt.calls):
        sol.mpc(mb.args)
    torch.cuda.synchronize()
    mean = sol.kernel_ms_mean(opt.calls)[3]
    hist = sol.kernel_ms_history(opt.calls)[:, 3]
    sol.enable_timing(False)
    return dict(stat(hist), mean=float(mean))


itf = api.QMInterface()
sc, sol, mb = solver_and_batch(itf)
ls = linesearch_ms(sol, mb)
if opt.linesearch_only:
    print(json.dumps(ls))
    sys.exit(0)
f64 = torch.float64
out = dict(node_cost=torch.zeros((B, N + 1), dtype=f64, device="cuda"), cost_terms=torch.zeros((B, N + 1, 8), dtype=f64, device="cuda"),
           defect=torch.zeros((B, N, 30), dtype=f64, device="cuda"), eq=torch.zeros((B, N, 16), dtype=f64, device="cuda"),
           nc=torch.zeros((B, N), dtype=torch.int32, device="cuda"), performance=torch.zeros((B, 8), dtype=f64, device="cuda"))
args = sol.metrics_args(B, N, mb.oT, mb.oX, mb.oU, mb.tt, mb.ts, mb.sn, mb.se, mb.sm, x0=mb.x0, **out)
perf_only = sol.metrics_args(B, N, mb.oT, mb.oX, mb.oU, mb.tt, mb.ts, mb.sn, mb.se, mb.sm, x0=mb.x0, performance=out["performance"])


def metrics_ms(a):
    sol.enable_timing(True)
    for _ in range(5 + opt.calls):
        sol.metrics(a)
    torch.cuda.synchronize()
    hist = sol.kernel_ms_history(opt.calls)[:, 5]
    sol.enable_timing(False)
    return stat(hist)


every, sums = metrics_ms(args), metrics_ms(perf_only)
stats = mb.oS.cpu().numpy()
p = out["performance"].cpu().numpy()
assert np.isfinite(p).all() and np.allclose(p[:, 0], stats[:, 2], rtol=1e-10) and np.allclose(np.sqrt(p[:, 3] + p[:, 4]), stats[:, 3], rtol=1e-9)
# traffic per node, in doubles: x, u read (x_next is the neighbour's x); node_cost, the 8 terms, the defect, the 16 equality values written, nc as half a double
read, written = 60, 1 + 8 + 30 + 16 + 0.5
rec = dict(batch=B, N=N, calls=opt.calls, device=torch.cuda.get_device_name(0), metrics_ms=every, metrics_performance_only_ms=sums, linesearch_ms=ls,
           metrics_over_linesearch=every["median"] / ls["median"], bytes_per_node=dict(read=read * 8, written=written * 8))
if opt.parent_tree:
    tree = os.path.abspath(opt.parent_tree)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", tree, "--linesearch-only", "--calls", str(opt.calls)], capture_output=True, text=True, timeout=200, cwd=tree)
    assert child.returncode == 0, child.stderr[-2000:]
    rec["parent_linesearch_ms"] = json.loads(child.stdout.strip().splitlines()[-1])
    rec["metrics_over_parent_linesearch"] = every["median"] / rec["parent_linesearch_ms"]["median"]
print(json.dumps(rec))
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    json.dump(rec, open(opt.out, "w"), indent=1)
