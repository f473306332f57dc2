"""CPU tier: taskspace_kernel (kernels/taskspace_kernel.h) on host threads (tests/emu) against taskspace_reference.py -- every instance, every node and every event, on
the perturbed iterates of test_emu_metrics.perturbed --, the exact items (every entry written, the flags from the schedule alone, the zeros) and the contracts that need
no GPU.

Tolerance rule (taskspace_reference.py): |kernel - reference| <= C eps magnitude.  C per output class is the next power of two at or above 8 x the worst ratio measured
over all scenarios of this file on the host build (profiles/taskspace_parity.json, section "emu"; the factor 8 is test_emu_metrics.py's, for the device's fused
multiply-adds and its order inside the tree sweep, which the host build does not reproduce).  With TASKSPACE_RECORD set to a file path every comparison test adds its
measured ratios there."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import kkt_scenarios as KS
import support as S
import taskspace_reference as TR
import test_emu_metrics as EM
from qm_door_amd import abi, api

RECORD = os.environ.get("TASKSPACE_RECORD") or None
# measured worst ratios on the host build (profiles/taskspace_parity.json "emu_worst"): feet_pos 3.11, ee_pos 6.81, ee_quat 14.16, com 3.77, feet_vel 4.23, base_twist 5.72,
# cop 1.42, foothold_pos 1.20; times 8, next power of two
C = {"feet_pos": 32.0, "ee_pos": 64.0, "ee_quat": 128.0, "com": 32.0, "feet_vel": 64.0, "base_twist": 64.0, "cop": 16.0, "foothold_pos": 16.0}
OUTPUTS = ("feet_pos", "ee_pos", "ee_quat", "com", "feet_vel", "base_twist", "cop", "foothold_pos", "foothold_flag")
NEEDS_U = ("feet_vel", "base_twist", "cop")
NEEDS_SCHEDULE = ("foothold_pos", "foothold_flag")
EPS = TR.EPS
THREADS = 128   # TASKSPACE_THREADS (kernels/taskspace_lds.h)


@pytest.fixture(scope="module")
def emu():
    lib = abi.load_library(S.build_emu())
    itf = api.QMInterface(lib=lib)
    return itf, S.Oracle(itf.problem)


def zero_events(itf, orc):
    """no event at all: one stance phase"""
    md = np.zeros(abi.MAX_EVENTS + 1, dtype=np.int32)
    md[0] = abi.MODE_NAMES["STANCE"]
    return KS._batch("zero_events", itf, orc, [(0, np.zeros(abi.MAX_EVENTS), md)] * 2, 3, 41, True, False)


def strict_edges(itf, orc):
    """events exactly at t_0 and at t_N at which feet would land (both excluded: the comparisons are strict) around one inside the horizon that counts:
    LF_RH -> STANCE at t_0 = 0, -> RF_LH at 2 dt (no landing), -> LF_RH at 4 dt (LF and RH land), -> STANCE at t_N = 6 dt"""
    dt, N = itf.problem.settings.dt, 6
    grid = np.arange(N + 1) * dt
    ev, md = np.zeros(abi.MAX_EVENTS), np.zeros(abi.MAX_EVENTS + 1, dtype=np.int32)
    ev[:4] = [grid[0], grid[2], grid[4], grid[N]]
    md[:5] = [abi.MODE_NAMES[m] for m in ("LF_RH", "STANCE", "RF_LH", "LF_RH", "STANCE")]
    return KS._batch("strict_edges", itf, orc, [(4, ev, md)] * 2, N, 43, True, False)


def scenarios():
    """test_emu_metrics.scenarios() -- N = 1, N = 2, the trot across its first switch at batch 3, every gait, the event-aligned grid, N + 1 = THREADS + 1 at batch 1 (lane 0
    takes the terminal node in a second pass), the event-aligned grid over a longer horizon -- plus a schedule without events and one with events exactly on both ends of the grid"""
    sc = dict(EM.scenarios())
    sc["event_grid"] = lambda itf, orc: KS.event_grid(itf, orc, 0.45)       # (test_emu_metrics' 0.12 s ends before the first landing; 0.45 s holds the lift-off and a landing)
    sc["zero_events"] = zero_events
    sc["strict_edges"] = strict_edges
    return sc


def blank(B, N, xp=np, **kw):
    """the outputs, pre-filled with NaN (-1 for the flags): every entry must be written"""
    E = abi.MAX_EVENTS
    return dict(feet_pos=xp.full((B, N + 1, 4, 3), np.nan, **kw), ee_pos=xp.full((B, N + 1, 3), np.nan, **kw), ee_quat=xp.full((B, N + 1, 4), np.nan, **kw),
                com=xp.full((B, N + 1, 3), np.nan, **kw), feet_vel=xp.full((B, N, 4, 3), np.nan, **kw), base_twist=xp.full((B, N, 6), np.nan, **kw),
                cop=xp.full((B, N, 3), np.nan, **kw), foothold_pos=xp.full((B, E, 4, 3), np.nan, **kw))


def call(sol, sc, X, U, want=OUTPUTS, rows=None):
    """qmgpu_mpc_taskspace_batch through the emulated library on instances `rows` (default: all) of scenario sc at (X, U); numpy arrays are the device memory.  U and the
    schedule are passed only if an output in `want` needs them."""
    rows = list(range(sc.B)) if rows is None else rows
    B, N = len(rows), sc.N
    pick = lambda a: np.ascontiguousarray(a[rows])  # noqa: E731
    out = blank(B, N)
    out["foothold_flag"] = np.full((B, abi.MAX_EVENTS, 4), -1, dtype=np.int32)
    sched = dict(sched_num=pick(sc.nev), sched_times=pick(sc.ev), sched_modes=pick(sc.md)) if set(want) & set(NEEDS_SCHEDULE) else {}
    a = sol.taskspace_args(B, N, pick(sc.grid), pick(X), U=pick(U) if set(want) & set(NEEDS_U) else None, **sched, **{k: out[k] for k in want})
    sol.taskspace(a)
    return {k: out[k] for k in want}


def reference(itf, sc, X, U, i):
    grid, nev, ev, md, _, _ = sc.instance(i)
    return TR.trajectory_taskspace(itf.problem.settings.gravity, grid, X[i], U[i], ev[:nev], md[:nev + 1])


def schedule_flags(sc, i):
    """foothold_flag of instance i from the schedule alone"""
    grid, nev, ev, md, _, _ = sc.instance(i)
    flag = np.zeros((abi.MAX_EVENTS, 4), dtype=np.int32)
    for e in range(nev):
        if grid[0] < ev[e] < grid[-1]:
            flag[e] = [int(not S.contact_flags(md[e])[c] and S.contact_flags(md[e + 1])[c]) for c in range(4)]
    return flag


def assert_exact_items(name, sc, U, got):
    """what holds bit for bit whatever the arithmetic: nothing left unwritten, the flags, the zero entries"""
    for k, v in got.items():
        assert (v != -1).all() if k == "foothold_flag" else np.isfinite(v).all(), (name, k)
    for i in range(sc.B):
        flag = schedule_flags(sc, i)
        assert np.array_equal(got["foothold_flag"][i], flag), (name, i)
        assert not got["foothold_pos"][i][flag == 0].any(), (name, i)
    fz = U[:, :, [2, 5, 8, 11]]
    s = ((fz[..., 0] + fz[..., 1]) + fz[..., 2]) + fz[..., 3]
    assert not got["cop"][s <= 0].any(), name


def record(section, name, ratios):
    if not RECORD:
        return
    try:
        rec = json.load(open(RECORD))
    except (OSError, ValueError):
        rec = {}
    rec.setdefault(section, {})[name] = ratios
    rec[section + "_worst"] = {c: max(r[c] for r in rec[section].values()) for c in TR.CLASSES}
    rec["C"] = C
    json.dump(rec, open(RECORD, "w"), indent=1)


def compare(name, itf, sc, X, U, got, section, instances=None):
    """every instance (or `instances`), every node and every event against the reference under the tolerance rule; the worst ratios are printed and recorded before
    anything is asserted"""
    worst = {c: 0.0 for c in TR.CLASSES}
    for i in (range(sc.B) if instances is None else instances):
        ref = reference(itf, sc, X, U, i)
        assert np.array_equal(got["foothold_flag"][i], ref["foothold_flag"]), (name, i)
        for c, r in TR.ratios({k: v[i] for k, v in got.items()}, ref).items():
            worst[c] = max(worst[c], r)
    print(name, section, "worst |kernel - reference| / (eps magnitude):", json.dumps(worst))
    record(section, name, worst)
    for c in TR.CLASSES:
        assert worst[c] <= C[c], (name, c, worst[c], C[c])


def test_scenario_set_lands_every_foot_and_flies():
    """from the schedules alone: over the scenarios of this file each of the four feet lands at least once inside a horizon, and at least one node is a flight node"""
    lib = abi.load_library(S.build_emu())
    itf = api.QMInterface(lib=lib)
    orc = S.Oracle(itf.problem)
    landed, flight = np.zeros(4, dtype=bool), False
    for name in scenarios():
        sc = KS.build(scenarios(), name, itf, orc)
        for i in range(sc.B):
            grid, nev, ev, md, _, _ = sc.instance(i)
            landed |= schedule_flags(sc, i).any(axis=0)
            flight = flight or any(md[int(np.sum(ev[:nev] <= t))] == abi.MODE_NAMES["FLY"] for t in grid)
    assert landed.all() and flight, (landed, flight)


@pytest.mark.parametrize("name", list(scenarios()))
def test_emu_taskspace_equals_the_reference(emu, name):
    itf, orc = emu
    sc = KS.build(scenarios(), name, itf, orc)
    X, U = EM.perturbed(sc)
    sol = api.GpuSolver(itf, max_batch=sc.B, max_nodes=sc.N)                 # a handle that never solved
    got = call(sol, sc, X, U)
    assert_exact_items(name, sc, U, got)
    compare(name, itf, sc, X, U, got, "emu")
    flags = got["foothold_flag"]
    if name == "two_passes_N128":
        assert sc.N + 1 == THREADS + 1 and sc.B == 1 and flags.any(axis=(0, 1)).all()                 # every foot lands somewhere in 1.9 s of trot
    if name == "trot_N7":
        assert sc.B == 3
    if name == "mixed_gaits":
        fz = U[:, :, [2, 5, 8, 11]]
        assert ((((fz[..., 0] + fz[..., 1]) + fz[..., 2]) + fz[..., 3]) <= 0).any()                     # cop's zero branch is taken
    if name == "event_grid":                                                                           # every event inside the horizon is a node: the weight sits at its edge
        for i in range(sc.B):
            inside = [t for t in sc.ev[i, :sc.nev[i]] if sc.grid[i, 0] < t < sc.grid[i, -1]]
            assert inside and all(t in sc.grid[i] for t in inside) and flags[i].any()
    if name == "zero_events":
        assert not sc.nev.any() and not flags.any() and not got["foothold_pos"].any()
    if name == "strict_edges":
        for i in range(sc.B):
            assert sc.ev[i, 0] == sc.grid[i, 0] and sc.ev[i, 3] == sc.grid[i, -1]
            assert flags[i].tolist()[:4] == [[0, 0, 0, 0], [0, 0, 0, 0], [1, 0, 0, 1], [0, 0, 0, 0]] and not flags[i, 4:].any()


def test_emu_taskspace_contracts(emu):
    """a repeated call; each output alone; batch 1 against batch 3; refused arguments; the struct's size"""
    itf, orc = emu
    sc = KS.build(scenarios(), "trot_N7", itf, orc)
    X, U = EM.perturbed(sc)
    B, N = sc.B, sc.N
    sol = api.GpuSolver(itf, max_batch=B, max_nodes=N)
    full = call(sol, sc, X, U)
    again = call(sol, sc, X, U)
    for k in OUTPUTS:
        assert np.array_equal(full[k], again[k]), k
    for k in OUTPUTS:                                                        # each output alone (U and the schedule passed only where it needs them): the same bits
        assert np.array_equal(call(sol, sc, X, U, want=(k,))[k], full[k]), k
    for i in range(B):                                                       # an instance alone: the same bits as inside the batch
        one = call(sol, sc, X, U, rows=[i])
        for k in OUTPUTS:
            assert np.array_equal(one[k][0], full[k][i]), (i, k)

    def refused(s, **change):
        out = blank(B, N)
        kw = dict(batch=B, num_nodes=N, time_grid=sc.grid, X=X, U=U, sched_num=sc.nev, sched_times=sc.ev, sched_modes=sc.md, feet_pos=out["feet_pos"])
        kw.update(change)
        with pytest.raises(abi.QmGpuError) as e:
            s.taskspace(s.taskspace_args(**kw))
        assert e.value.status == abi.ERR_INVALID_ARGUMENT and str(e.value), change
    out = blank(B, N)
    flag = np.zeros((B, abi.MAX_EVENTS, 4), dtype=np.int32)
    refused(sol, batch=B + 1); refused(sol, num_nodes=N + 1); refused(sol, batch=0); refused(sol, num_nodes=0)
    refused(sol, time_grid=None); refused(sol, X=None)
    for k in NEEDS_U:
        refused(sol, U=None, **{k: out[k]})
    for missing in ("sched_num", "sched_times", "sched_modes"):
        refused(sol, foothold_pos=out["foothold_pos"], **{missing: None})
        refused(sol, foothold_flag=flag, **{missing: None})
    refused(api.GpuSolver(itf, max_batch=B, max_nodes=N, dtype="f32"))
    assert itf.lib.qmgpu_mpc_taskspace_batch(sol.handle, None) == abi.ERR_INVALID_ARGUMENT            # a null argument struct
    sol.taskspace(sol.taskspace_args(B, N, sc.grid, X, feet_pos=out["feet_pos"]))                      # positions need neither U nor the schedule
    assert np.array_equal(out["feet_pos"], full["feet_pos"])


def test_taskspace_args_layout_matches_c():
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "qmgpu.h"
    int main(void) { printf("%zu %zu %zu %zu\n", sizeof(qmgpu_taskspace_args), offsetof(qmgpu_taskspace_args, time_grid), offsetof(qmgpu_taskspace_args, feet_pos),
                            offsetof(qmgpu_taskspace_args, foothold_flag)); return 0; }
    '''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(S.ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        sizes = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).split()]
    T = abi.TaskspaceArgs
    assert sizes == [ctypes.sizeof(T), T.time_grid.offset, T.feet_pos.offset, T.foothold_flag.offset]
