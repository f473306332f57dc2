"""-m gpu: the SQP solution metrics (qmgpu_mpc_metrics_batch) on the device.

The comparisons of the emulation tier (test_emu_metrics.py: its tolerance rule and its C, set from the host build's ratios and not from the device's) on scenarios of
kkt_scenarios.gpu_scenarios(): against metrics_reference.py at a perturbed iterate -- every instance and node, except horizon_N200 (the reference on instance 0; nc
and the padding on all) --, against the product's own LQ dump and solve statistics at the warm start and at out_x / out_u, force tracking (product against
product), poisoned scratch, a WBC pending on the overlap stream, an F32 handle, determinism.  With METRICS_RECORD set to a file path the measured ratios are added
there under "gpu" (the record of profiles/metrics_parity.json)."""
import numpy as np
import pytest

import kkt_scenarios as KS
import ls_reference as LSR
import metrics_reference as MR
import support as S
import test_emu_metrics as EM

pytestmark = pytest.mark.gpu

SCENARIOS = ["horizon_N1", "horizon_N2", "trot_cold", "mixed_gaits", "event_grid", "horizon_N200"]
REDUCED = {"horizon_N200": [0]}


@pytest.fixture(scope="module")
def params(interface):
    return LSR.Params(interface.problem.settings)


def _call(G, sol, sc, X, U, x0=None, want=EM.OUTPUTS, rows=None, contact=None):
    """qmgpu_mpc_metrics_batch on instances `rows` (default: all) of scenario sc at (X, U); the outputs (numpy) start as NaN / -1"""
    import torch
    rows = list(range(sc.B)) if rows is None else rows
    B, N = len(rows), sc.N
    f64, i32 = torch.float64, torch.int32
    d = lambda a, t=f64: None if a is None else G.dev(np.ascontiguousarray(a[rows]), t)  # noqa: E731
    out = EM.blank(B, N, xp=torch, dtype=f64, device="cuda")
    out["nc"] = torch.full((B, N), -1, dtype=i32, device="cuda")
    a = sol.metrics_args(B, N, d(sc.grid), d(X), d(U), d(sc.tt), d(sc.ts), d(sc.nev, i32), d(sc.ev), d(sc.md, i32), x0=d(x0), ee_contact_ref=d(contact), **{k: out[k] for k in want})
    sol.metrics(a)
    sol.synchronize()
    return {k: out[k].cpu().numpy() for k in want}


def _solve(G, sol, sc):
    import torch
    mb = G.MpcBatch(sc.x0, sc.tt, sc.ts, sc.nev, sc.ev, sc.md, sc.N, warm=(sc.X, sc.U) if sc.warm else None, line_search=sc.line_search, time_grid=None if sc.uniform else sc.grid)
    if sc.contact is not None:
        mb.contact = G.dev(sc.contact, torch.float64)
        mb.args.ee_contact_ref = mb.contact.data_ptr()
    sol.mpc(mb.args)
    return mb, mb.results()


@pytest.mark.parametrize("name", SCENARIOS)
def test_metrics_equal_the_reference(interface, oracle, params, name):
    import gpu_harness as G
    sc = KS.build(KS.gpu_scenarios(), name, interface, oracle)
    X, U = EM.perturbed(sc)
    sol = G.make_solver(interface, sc.B, sc.N)                               # a handle that never solved
    got = _call(G, sol, sc, X, U)
    EM.assert_exact_items(name, got)
    nc_seen, _ = EM.compare(name, params, sc, X, U, got, "gpu", instances=REDUCED.get(name))
    assert np.abs(got["defect"]).max() > 0.1 and np.abs(got["eq"]).max() > 0.1
    if name == "mixed_gaits":
        assert {12, 13, 14, 16} <= set(got["nc"].ravel().tolist())
    if name == "horizon_N200":                                               # nc of every instance: the mode of the node's time, from the schedule alone
        for i in range(sc.B):
            grid, nev, ev, md, _, _ = sc.instance(i)
            want = [sum(3 if f else 4 for f in S.contact_flags(md[int(np.sum(ev[:nev] <= t))])) for t in grid[:-1]]
            assert got["nc"][i].tolist() == want, i
    withx0 = _call(G, sol, sc, X, U, x0=sc.x0)
    grow = ((sc.x0 - X[:, 0]) ** 2).sum(axis=1)
    # the kernel forms fl(SSE + s), s its tree sum of the 30 squares (7 levels, each square rounded once: <= 9 eps s); the difference taken here is exact or rounded once,
    # numpy's own sum of the squares carries <= 31 eps s: together below eps SSE' + 41 eps s <= 64 eps SSE' (SSE' the value with x0, s <= SSE')
    d = withx0["performance"][:, 3] - got["performance"][:, 3]
    assert (np.abs(d - grow) <= 64 * EM.EPS * withx0["performance"][:, 3]).all() and np.array_equal(np.delete(withx0["performance"], 3, axis=1), np.delete(got["performance"], 3, axis=1))
    for i in (range(sc.B) if name not in REDUCED else REDUCED[name]):         # with x0: every output against the reference again
        assert not MR.within({k: v[i] for k, v in withx0.items()}, EM.reference(params, sc, X, U, i, sc.x0), EM.C), (name, i)
    again = _call(G, sol, sc, X, U)                                          # two calls in a row: the same bits
    for k in EM.OUTPUTS:
        assert np.array_equal(again[k], got[k]), (name, k)
    sol.close()


@pytest.mark.parametrize("name", ["horizon_N2", "mixed_gaits", "event_grid"])
def test_metrics_equal_the_solve_they_restate(interface, oracle, params, name):
    """the warm-started solve with the LQ dump on: b, e of the dump and out_stats[0..1] at the warm start, out_stats[2..3] at out_x / out_u; and the solves untouched"""
    import gpu_harness as G
    sc = KS.build(KS.gpu_scenarios(), name, interface, oracle)
    plain_sol = G.make_solver(interface, sc.B, sc.N)
    _, plain = _solve(G, plain_sol, sc)
    plain_sol.close()
    sol = G.make_solver(interface, sc.B, sc.N)
    sol.enable_debug(True)
    _, out = _solve(G, sol, sc)
    EM.check_against_solve(name, params, sc, sol, out, lambda X, U: _call(G, sol, sc, X, U), range(sc.B))
    _, again = _solve(G, sol, sc)
    for key in ("T", "X", "U", "mode", "stats"):
        assert np.array_equal(out[key], plain[key]) and np.array_equal(again[key], plain[key]), (name, key)
    sol.close()


def test_force_tracking_term_product_against_product():
    """Product against product (the reference leaves force tracking out): slot 6 is non-zero with the contact reference and exactly 0 without it on the same handle;
    performance at out_x / out_u matches out_stats[2..3] of that solve under the sum rule, the magnitudes taken from the call's own terms."""
    import gpu_harness as G
    itf = KS.force_tracking_interface()
    orc = S.Oracle(itf.problem)
    sc = KS.force_tracking(itf, orc, B=2, N=2)
    sol = G.make_solver(itf, sc.B, sc.N)
    _, out = _solve(G, sol, sc)
    sc.grid = out["T"]
    on = _call(G, sol, sc, out["X"], out["U"], contact=sc.contact)
    off = _call(G, sol, sc, out["X"], out["U"])
    EM.assert_exact_items("force_tracking", on, force_tracking=True)
    EM.assert_exact_items("force_tracking", off)
    assert (on["cost_terms"][:, :-1, 6] > 0).all() and not on["cost_terms"][:, -1, 6].any()
    dts = np.diff(out["T"], axis=1)
    P = LSR.Params(itf.problem.settings)
    for i in range(sc.B):
        # the magnitudes of everything but the force term come from the reference at the same point; the force term's own summands are added to both parts of the rule
        ref = EM.reference(P, sc, out["X"], out["U"], i)
        m, ms = ref["mag"]["performance"].copy(), ref["mag"]["performance_sum"].copy()
        force = float(dts[i] @ on["cost_terms"][i, :-1, 6])
        m[0] += force; ms[0] += (sc.N + 2) * force
        allow = EM.C["performance"] * EM.EPS * m + EM.EPS * ms
        p = on["performance"][i]
        merit, viol = out["stats"][i, 2], out["stats"][i, 3]
        assert abs(p[0] - merit) <= allow[0], (i, p[0], merit, allow[0])
        assert abs((p[3] + p[4]) - viol * viol) <= allow[3] + allow[4], (i, p[3] + p[4], viol * viol)
    sol.close()


def test_metrics_read_nothing_a_solve_leaves_behind(interface, oracle):
    """qmgpu_debug_poison (every scratch buffer and the LDS filled with NaN) before the call: no NaN, the same bits"""
    import gpu_harness as G
    sc = KS.build(KS.gpu_scenarios(), "trot_cold", interface, oracle)
    X, U = EM.perturbed(sc)
    sol = G.make_solver(interface, sc.B, sc.N)
    clean = _call(G, sol, sc, X, U, x0=sc.x0)
    sol.debug_poison()
    poisoned = _call(G, sol, sc, X, U, x0=sc.x0)
    for k in EM.OUTPUTS:
        assert np.isfinite(poisoned[k]).all() and np.array_equal(clean[k], poisoned[k]), k
    sol.close()


def test_metrics_next_to_a_pending_wbc(interface, oracle):
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
    for k in EM.OUTPUTS:
        assert np.array_equal(res[True][0][k], res["plain"][k]), k
    for k in ("out", "status", "input_last"):
        assert np.array_equal(res[True][1][k], res[False][1][k]), k


def test_metrics_contracts_and_determinism(interface, oracle):
    """an F32 handle and arguments beyond the capacity are refused; an instance alone gives the bits it gives inside a batch of 3"""
    import gpu_harness as G
    from qm_door_amd import abi
    sc = KS.unroll(interface, oracle, "trot", 3, 7, 13, True, False)
    X, U = EM.perturbed(sc)
    B, N = sc.B, sc.N
    sol = G.make_solver(interface, B, N)
    full = _call(G, sol, sc, X, U, x0=sc.x0)
    one = _call(G, sol, sc, X, U, x0=sc.x0, rows=[1])
    for k in EM.OUTPUTS:
        assert np.array_equal(one[k][0], full[k][1]), k
    perf_only = _call(G, sol, sc, X, U, x0=sc.x0, want=("performance",))
    assert np.array_equal(perf_only["performance"], full["performance"])
    f32 = G.make_solver(interface, B, N, dtype="f32")
    small = G.make_solver(interface, B - 1, N - 1)
    for s in (f32, small):
        with pytest.raises(abi.QmGpuError) as e:
            _call(G, s, sc, X, U)
        assert e.value.status == abi.ERR_INVALID_ARGUMENT and str(e.value)
    for s in (sol, f32, small):
        s.close()


def test_timed_metrics_calls_stay_out_of_the_kernel_means(interface, oracle):
    """with timing on, a metrics call is one row of the history ([5] only) and is left out of qmgpu_kernel_ms_mean: the per-kernel times of the solves stay the solves'"""
    import gpu_harness as G
    sc = KS.build(KS.gpu_scenarios(), "horizon_N2", interface, oracle)
    sol = G.make_solver(interface, sc.B, sc.N)
    sol.enable_timing(True)
    _solve(G, sol, sc)
    _call(G, sol, sc, sc.X, sc.U)
    hist, mean = sol.kernel_ms_history(2), np.array(sol.kernel_ms_mean(2))
    assert not hist[1, :5].any() and hist[1, 5] > 0 and (hist[0, :4] > 0).all()
    assert np.array_equal(mean, hist[0]), (mean, hist)
    _call(G, sol, sc, sc.X, sc.U)
    only = np.array(sol.kernel_ms_mean(2))                                   # a window of metrics calls alone: their mean in [5]
    h2 = sol.kernel_ms_history(2)
    assert not only[:5].any() and abs(only[5] - h2[:, 5].mean()) <= 1e-12
    sol.close()
