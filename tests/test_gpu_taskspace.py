"""-m gpu: the planned task-space trajectories (qmgpu_mpc_taskspace_batch) on the device.

The comparisons of the emulation tier (test_emu_taskspace.py: its tolerance rule and its C, set from the host build's ratios and not from the device's) on the scenarios
of kkt_scenarios.gpu_scenarios() that test_gpu_metrics.py uses: against taskspace_reference.py at a perturbed iterate -- every instance, node and event, except
horizon_N200 (the reference on instance 0; the flags and the zeros on all) --, on a handle that never solved; product against product, the stance rows of eq from
qmgpu_mpc_metrics_batch; the solves around the call untouched; poisoned scratch; a WBC pending on the overlap stream; an F32 handle; the timing ring.  With
TASKSPACE_RECORD set to a file path the measured ratios are added there under "gpu" (the record of profiles/taskspace_parity.json)."""
import numpy as np
import pytest

import kkt_scenarios as KS
import support as S
import taskspace_reference as TR
import test_emu_metrics as EM
import test_emu_taskspace as ET
import test_gpu_metrics as GM

pytestmark = pytest.mark.gpu

SCENARIOS = GM.SCENARIOS
REDUCED = GM.REDUCED


def _call(G, sol, sc, X, U, want=ET.OUTPUTS, rows=None):
    """qmgpu_mpc_taskspace_batch on instances `rows` (default: all) of scenario sc at (X, U); the outputs (numpy) start as NaN / -1"""
    import torch
    rows = list(range(sc.B)) if rows is None else rows
    B, N = len(rows), sc.N
    f64, i32 = torch.float64, torch.int32
    d = lambda a, t=f64: G.dev(np.ascontiguousarray(a[rows]), t)  # noqa: E731
    out = ET.blank(B, N, xp=torch, dtype=f64, device="cuda")
    out["foothold_flag"] = torch.full((B, TR.MAX_EVENTS, 4), -1, dtype=i32, device="cuda")
    sched = dict(sched_num=d(sc.nev, i32), sched_times=d(sc.ev), sched_modes=d(sc.md, i32)) if set(want) & set(ET.NEEDS_SCHEDULE) else {}
    a = sol.taskspace_args(B, N, d(sc.grid), d(X), U=d(U) if set(want) & set(ET.NEEDS_U) else None, **sched, **{k: out[k] for k in want})
    sol.taskspace(a)
    sol.synchronize()
    return {k: out[k].cpu().numpy() for k in want}


@pytest.mark.parametrize("name", SCENARIOS)
def test_taskspace_equals_the_reference(interface, oracle, name):
    import gpu_harness as G
    sc = KS.build(KS.gpu_scenarios(), name, interface, oracle)
    X, U = EM.perturbed(sc)
    sol = G.make_solver(interface, sc.B, sc.N)                               # a handle that never solved
    got = _call(G, sol, sc, X, U)
    ET.assert_exact_items(name, sc, U, got)                                  # every instance: nothing unwritten, the flags from the schedule alone, the zeros
    ET.compare(name, interface, sc, X, U, got, "gpu", instances=REDUCED.get(name))
    if name in ("mixed_gaits", "horizon_N200"):
        assert got["foothold_flag"].any(axis=(0, 1)).all(), name             # every foot lands somewhere
    again = _call(G, sol, sc, X, U)                                          # two calls in a row: the same bits
    for k in ET.OUTPUTS:
        assert np.array_equal(again[k], got[k]), (name, k)
    sol.close()


def test_stance_foot_velocities_are_the_stance_rows_of_the_metrics(interface, oracle):
    """Product against product: feet_vel of a stance foot against the three rows that foot contributes to eq of qmgpu_mpc_metrics_batch at the same point, with
    position_error_gain = 0 (the z row is then the velocity alone).  The two kernels run the same sweep on the same inputs; the allowance is the rule's, C eps magnitude
    with the reference's magnitude of the foot velocity and the larger of the two classes' C."""
    import gpu_harness as G
    from qm_door_amd import api
    itf = api.QMInterface()                                                  # an interface of its own: the session's keeps its gain
    itf.problem.settings.position_error_gain = 0.0
    sc = KS.build(KS.gpu_scenarios(), "mixed_gaits", interface, oracle)
    X, U = EM.perturbed(sc)
    sol = G.make_solver(itf, sc.B, sc.N)
    ts = _call(G, sol, sc, X, U, want=("feet_vel",))
    mt = GM._call(G, sol, sc, X, U, want=("eq", "nc"))
    c = max(ET.C["feet_vel"], EM.C["eq"])
    worst, rows_seen = 0.0, 0
    for i in range(sc.B):
        grid, nev, ev, md, _, _ = sc.instance(i)
        mag = TR.trajectory_taskspace(itf.problem.settings.gravity, grid, X[i], U[i])["mag"]["feet_vel"]
        for k in range(sc.N):
            flags = S.contact_flags(md[int(np.sum(ev[:nev] <= grid[k]))])
            row = 0
            for foot in range(4):
                if flags[foot]:
                    gap = np.abs(ts["feet_vel"][i, k, foot] - mt["eq"][i, k, row:row + 3])
                    worst = max(worst, float((gap / (c * TR.EPS * mag[k, foot])).max()))
                    rows_seen += 3
                row += 3 if flags[foot] else 4
            assert row == mt["nc"][i, k]
    print("stance rows compared:", rows_seen, "worst gap / allowance:", worst)
    assert rows_seen > 0 and worst <= 1.0
    sol.close()


def test_solves_around_the_call_are_bit_identical(interface, oracle):
    """a solve, the call, the same solve again, on one handle: T, X, U, mode and stats of both solves equal those of a handle that never made the call"""
    import gpu_harness as G
    sc = KS.build(KS.gpu_scenarios(), "horizon_N2", interface, oracle)
    plain_sol = G.make_solver(interface, sc.B, sc.N)
    _, plain = GM._solve(G, plain_sol, sc)
    plain_sol.close()
    sol = G.make_solver(interface, sc.B, sc.N)
    _, before = GM._solve(G, sol, sc)
    got = _call(G, sol, sc, before["X"], before["U"])
    assert all(np.isfinite(v).all() for k, v in got.items() if k != "foothold_flag")
    _, after = GM._solve(G, sol, sc)
    for key in ("T", "X", "U", "mode", "stats"):
        assert np.array_equal(before[key], plain[key]) and np.array_equal(after[key], plain[key]), key
    sol.close()


def test_taskspace_reads_nothing_a_solve_leaves_behind(interface, oracle):
    """qmgpu_debug_poison (every scratch buffer and the LDS filled with NaN) before the call: every output finite, the same bits"""
    import gpu_harness as G
    sc = KS.build(KS.gpu_scenarios(), "trot_cold", interface, oracle)
    X, U = EM.perturbed(sc)
    sol = G.make_solver(interface, sc.B, sc.N)
    clean = _call(G, sol, sc, X, U)
    sol.debug_poison()
    poisoned = _call(G, sol, sc, X, U)
    for k in ET.OUTPUTS:
        assert np.isfinite(poisoned[k]).all() and np.array_equal(clean[k], poisoned[k]), k
    sol.close()


def test_taskspace_next_to_a_pending_wbc(interface, oracle):
    """qmgpu_set_overlap(1), a WBC pending from qmgpu_cycle_batch: the call does not join it, returns the bits it returns without overlap, and the WBC outputs after
    qmgpu_synchronize are those of a cycle without the call"""
    import torch
    import gpu_harness as G
    sc = KS.build(KS.gpu_scenarios(), "trot_cold", interface, oracle)
    X, U = EM.perturbed(sc)
    B, N = sc.B, sc.N
    rbd = np.array([S.rbd_from_state(oracle, sc.x0[i]) for i in range(B)])
    res = {}
    for overlap in (False, True):
        sol = G.make_solver(interface, B, N)
        sol.set_overlap(overlap)
        mb = G.MpcBatch(sc.x0, sc.tt, sc.ts, sc.nev, sc.ev, sc.md, N)
        wb = G.WbcBatch(rbd, np.full(B, 0.002), np.full(B, 20.0), np.zeros((B, 30)))
        sol.cycle(mb.args, G.dev(np.zeros(B), torch.float64), wb.args)
        m = _call(G, sol, sc, X, U) if overlap else None
        sol.synchronize()
        res[overlap] = (m, wb.results())
        if not overlap:
            res["plain"] = _call(G, sol, sc, X, U)
        sol.close()
    for k in ET.OUTPUTS:
        assert np.array_equal(res[True][0][k], res["plain"][k]), k
    for k in ("out", "status", "input_last"):
        assert np.array_equal(res[True][1][k], res[False][1][k]), k


def test_taskspace_contracts_and_determinism(interface, oracle):
    """an F32 handle and arguments beyond the capacity are refused; an instance alone gives the bits it gives inside a batch of 3; positions without U and schedule"""
    import gpu_harness as G
    from qm_door_amd import abi
    sc = KS.unroll(interface, oracle, "trot", 3, 7, 13, True, False)
    X, U = EM.perturbed(sc)
    B, N = sc.B, sc.N
    sol = G.make_solver(interface, B, N)
    full = _call(G, sol, sc, X, U)
    one = _call(G, sol, sc, X, U, rows=[1])
    for k in ET.OUTPUTS:
        assert np.array_equal(one[k][0], full[k][1]), k
    pos_only = _call(G, sol, sc, X, U, want=TR.NODE_OUTPUTS)
    for k in TR.NODE_OUTPUTS:
        assert np.array_equal(pos_only[k], full[k]), k
    f32 = G.make_solver(interface, B, N, dtype="f32")
    small = G.make_solver(interface, B - 1, N - 1)
    for s in (f32, small):
        with pytest.raises(abi.QmGpuError) as e:
            _call(G, s, sc, X, U)
        assert e.value.status == abi.ERR_INVALID_ARGUMENT and str(e.value)
    for s in (sol, f32, small):
        s.close()


def test_taskspace_calls_leave_the_timing_ring_alone(interface, oracle):
    """with timing on, qmgpu_last_kernel_ms, qmgpu_kernel_ms_mean and qmgpu_kernel_ms_history are the same before and after the call"""
    import gpu_harness as G
    sc = KS.build(KS.gpu_scenarios(), "horizon_N2", interface, oracle)
    sol = G.make_solver(interface, sc.B, sc.N)
    sol.enable_timing(True)
    GM._solve(G, sol, sc)
    GM._solve(G, sol, sc)
    before = (sol.last_kernel_ms(), sol.kernel_ms_mean(2), sol.kernel_ms_history(2))
    _call(G, sol, sc, sc.X, sc.U)
    after = (sol.last_kernel_ms(), sol.kernel_ms_mean(2), sol.kernel_ms_history(2))
    assert before[0] == after[0] and before[1] == after[1] and np.array_equal(before[2], after[2]) and before[0][5] > 0
    sol.close()
