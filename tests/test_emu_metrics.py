"""CPU tier: metrics_kernel (kernels/metrics_kernel.h) on host threads (tests/emu) against metrics_reference.py -- every instance, every node, on iterates with O(0.1)
defects and constraint values --, against the emulated library's OWN LQ dump and solve statistics, the exact items (nc, the zero padding, node_cost as the stated sum,
the zero slots) and the contracts that need no GPU.

Tolerance rule (metrics_reference.py): |kernel - reference| <= C eps magnitude, the sums with (N + 2) eps sum |summand| on top.  C per output class is the next power
of two at or above 8 x the worst ratio measured over all scenarios of this file on the host build (profiles/metrics_parity.json, section "emu"; the factor 8 is for
the device's fused multiply-adds and its order inside the tree sweep, which the host build does not reproduce).  With METRICS_RECORD set to a file path every
comparison test adds its measured ratios there."""
import json
import os

import numpy as np
import pytest

import kkt_scenarios as KS
import ls_reference as LSR
import metrics_reference as MR
import support as S
from qm_door_amd import abi, api
from test_kkt_reference import emu_solve

RECORD = os.environ.get("METRICS_RECORD") or None
# measured worst ratios on the host build (profiles/metrics_parity.json "emu_worst"): defect 1.80, eq 5.40, cost_terms 0.52, performance 1.42; times 8, next power of two
C = {"defect": 16.0, "eq": 64.0, "cost_terms": 8.0, "performance": 16.0}
OUTPUTS = ("node_cost", "cost_terms", "defect", "eq", "nc", "performance")
EPS = MR.EPS


@pytest.fixture(scope="module")
def emu():
    lib = abi.load_library(S.build_emu())
    itf = api.QMInterface(lib=lib)
    return itf, S.Oracle(itf.problem), LSR.Params(itf.problem.settings)


def scenarios():
    """N = 1, N = 2, N = 7 across the first switch of the trot (nc 12 -> 14, batch 3), every gait (nc 13 and 16 among them), the event-aligned grid, and N + 1 = 129 at
    batch 1: one node more than the workgroup has lanes, so lane 0 takes a second node (the terminal one) in a second pass"""
    return {
        "horizon_N1": lambda itf, orc: KS.horizon(itf, orc, 1, True, False),
        "horizon_N2": lambda itf, orc: KS.horizon(itf, orc, 2, True, False),
        "trot_N7": lambda itf, orc: KS.unroll(itf, orc, "trot", 3, 7, 13, True, False),
        "mixed_gaits": lambda itf, orc: KS.mixed_gaits(itf, orc, 4, 8),
        "event_grid": lambda itf, orc: KS.event_grid(itf, orc, 0.12),
        "two_passes_N128": lambda itf, orc: KS.horizon(itf, orc, 128, True, False, B=1),
    }


def perturbed(sc, seed=5):
    """(X, U) of the scenario's warm start pushed off the dynamics and off the constraints: states (row 0 included: X_0 != x0) by 0.1, forces by 5 N, joint rates by 0.5"""
    rng = np.random.default_rng(seed)
    X = sc.X + 0.1 * rng.standard_normal(sc.X.shape)
    U = sc.U + rng.standard_normal(sc.U.shape) * np.r_[np.full(12, 5.0), np.full(18, 0.5)]
    return np.ascontiguousarray(X), np.ascontiguousarray(U)


def blank(B, N, xp=np, **kw):
    """the outputs, pre-filled with NaN (-1 for nc): every entry must be written"""
    return dict(node_cost=xp.full((B, N + 1), np.nan, **kw), cost_terms=xp.full((B, N + 1, 8), np.nan, **kw), defect=xp.full((B, N, 30), np.nan, **kw),
                eq=xp.full((B, N, 16), np.nan, **kw), performance=xp.full((B, 8), np.nan, **kw))


def call(sol, sc, X, U, x0=None, want=OUTPUTS, rows=None, contact=None):
    """qmgpu_mpc_metrics_batch through the emulated library on instances `rows` (default: all) of scenario sc at (X, U); numpy arrays are the device memory"""
    rows = list(range(sc.B)) if rows is None else rows
    B, N = len(rows), sc.N
    pick = lambda a: None if a is None else np.ascontiguousarray(a[rows])  # noqa: E731
    out = blank(B, N)
    out["nc"] = np.full((B, N), -1, dtype=np.int32)
    a = sol.metrics_args(B, N, pick(sc.grid), pick(X), pick(U), pick(sc.tt), pick(sc.ts), pick(sc.nev), pick(sc.ev), pick(sc.md), x0=pick(x0), ee_contact_ref=pick(contact),
                         **{k: out[k] for k in want})
    sol.metrics(a)
    return {k: out[k] for k in want}


def reference(P, sc, X, U, i, x0=None):
    grid, nev, ev, md, tt, ts = sc.instance(i)
    return MR.trajectory_metrics(P, grid, X[i], U[i], ev[:nev], md[:nev + 1], tt, ts, x0=None if x0 is None else x0[i])


def assert_exact_items(name, got, force_tracking=False):
    """what holds bit for bit whatever the arithmetic: nothing left unwritten, the zero padding, node_cost as the stated sum, the zero slots"""
    for k, v in got.items():
        assert (v != -1).all() if k == "nc" else np.isfinite(v).all(), (name, k)
    t = got["cost_terms"]
    assert np.array_equal(got["node_cost"], ((((((t[..., 0] + t[..., 1]) + t[..., 2]) + t[..., 3]) + t[..., 4]) + t[..., 5]) + t[..., 6])), name
    assert not t[..., 7].any() and (force_tracking or not t[..., 6].any()), name
    assert not t[:, -1, [0, 1, 3, 4, 5, 6, 7]].any(), name                                   # terminal node: slot 2 only
    assert not got["performance"][:, [2, 5, 6, 7]].any() and np.array_equal(got["performance"][:, 0], got["performance"][:, 1]), name
    pad = np.arange(16)[None, None, :] >= got["nc"][:, :, None]
    assert not got["eq"][pad].any() and ((got["nc"] >= 12) & (got["nc"] <= 16)).all(), name


def record(section, name, ratios):
    if not RECORD:
        return
    try:
        rec = json.load(open(RECORD))
    except (OSError, ValueError):
        rec = {}
    rec.setdefault(section, {})[name] = ratios
    rec[section + "_worst"] = {c: max(r[c] for r in rec[section].values()) for c in MR.CLASSES}
    rec["C"] = C
    json.dump(rec, open(RECORD, "w"), indent=1)


def compare(name, P, sc, X, U, got, section, x0=None, instances=None):
    """every instance (or `instances`) and every node against the reference: nc exact, the rest under the tolerance rule; the worst ratios are printed and recorded
    before anything is asserted"""
    worst, nc_seen, refs = {c: 0.0 for c in MR.CLASSES}, set(), {}
    for i in (range(sc.B) if instances is None else instances):
        refs[i] = ref = reference(P, sc, X, U, i, x0)
        gi = {k: v[i] for k, v in got.items()}
        assert np.array_equal(gi["nc"], ref["nc"]), (name, i, gi["nc"], ref["nc"])
        nc_seen |= set(ref["nc"].tolist())
        for c, r in MR.ratios(gi, ref).items():
            worst[c] = max(worst[c], r)
        cm = ref["mag"]["node_cost"]
        worst["cost_terms"] = max(worst["cost_terms"], float((np.abs(gi["node_cost"] - ref["node_cost"]) / (EPS * cm)).max()))
    print(name, section, "worst |kernel - reference| / (eps magnitude):", json.dumps(worst), "nc", sorted(nc_seen))
    record(section, name, worst)
    for c in MR.CLASSES:
        assert worst[c] <= C[c], (name, c, worst[c], C[c])
    return nc_seen, refs


@pytest.mark.parametrize("name", list(scenarios()))
def test_emu_metrics_equal_the_reference(emu, name):
    itf, orc, P = emu
    sc = KS.build(scenarios(), name, itf, orc)
    X, U = perturbed(sc)
    sol = api.GpuSolver(itf, max_batch=sc.B, max_nodes=sc.N)                 # a handle that never solved
    got = call(sol, sc, X, U)
    assert_exact_items(name, got)
    nc_seen, refs = compare(name, P, sc, X, U, got, "emu")
    assert np.abs(got["defect"]).max() > 0.1 and np.abs(got["eq"]).max() > 0.1
    if name == "trot_N7":
        assert nc_seen == {12, 14}
    if name == "mixed_gaits":
        assert {13, 16} <= nc_seen
    if name == "event_grid":
        assert (np.diff(sc.grid[0]) < 0.25 * itf.problem.settings.dt).any()
    # the initial-state term: with x0 given, performance[3] grows by |x0 - X_0|^2 and nothing else moves
    withx0 = call(sol, sc, X, U, x0=sc.x0)
    for k in OUTPUTS:
        if k != "performance":
            assert np.array_equal(withx0[k], got[k]), (name, k)
    grow = ((sc.x0 - X[:, 0]) ** 2).sum(axis=1)
    assert (grow > 0.05).all() and np.array_equal(np.delete(withx0["performance"], 3, axis=1), np.delete(got["performance"], 3, axis=1))
    # the kernel forms fl(SSE + s), s its tree sum of the 30 squares (7 levels, each square rounded once: <= 9 eps s); the difference taken here is exact or rounded once,
    # numpy's own sum of the squares carries <= 31 eps s: together below eps SSE' + 41 eps s <= 64 eps SSE' (SSE' the value with x0, s <= SSE')
    d = withx0["performance"][:, 3] - got["performance"][:, 3]
    assert (np.abs(d - grow) <= 64 * EPS * withx0["performance"][:, 3]).all(), (name, d, grow)
    for i in range(sc.B):
        ref = reference(P, sc, X, U, i, sc.x0)
        assert not MR.within({k: v[i] for k, v in withx0.items()}, ref, C), (name, i)


@pytest.mark.parametrize("name", ["horizon_N2", "trot_N7", "event_grid"])
def test_emu_metrics_equal_the_solve_they_restate(emu, name):
    """A warm-started solve with the LQ dump on.  At the warm start (row 0 = x0): defect and eq against the b and e of the dump, performance against out_stats[0..1];
    at out_x / out_u: performance against out_stats[2..3].  Product against product: the two sides differ in the order of their operations only; the allowance is
    the rule's, C eps magnitude (the sums: plus (N + 2) eps sum |summand|), with the reference's magnitudes at the same point.  The solve reports the violation as
    sqrt(dynamics SSE + equality SSE); it is compared squared, under the sum of the two allowances."""
    itf, orc, P = emu
    sc = KS.build(scenarios(), name, itf, orc)
    _, plain = emu_solve(itf, sc, False)                                      # a handle that never makes the call
    sol, out = emu_solve(itf, sc, True)
    check_against_solve(name, P, sc, sol, out, lambda X, U, **kw: call(sol, sc, X, U, **kw), range(sc.B))
    # a solve after the call: bit-identical to one on a handle that never called
    again_sol = sol
    B, N = sc.B, sc.N
    oT, oX, oU, oM, oS = np.zeros((B, N + 1)), np.zeros((B, N + 1, 30)), np.zeros((B, N, 30)), np.zeros((B, N + 1), dtype=np.int32), np.zeros((B, abi.NSTATS))
    a = again_sol.mpc_args(B, N, sc.x0, sc.tt, sc.ts, sc.nev, sc.ev, sc.md, oT, oX, oU, oM, oS, t0=np.zeros(B) if sc.uniform else None,
                           time_grid=None if sc.uniform else sc.grid, warm_x=sc.X, warm_u=sc.U, line_search=sc.line_search)
    again_sol.mpc(a)
    for key, got in (("T", oT), ("X", oX), ("U", oU), ("mode", oM), ("stats", oS)):
        assert np.array_equal(got, plain[key]) and np.array_equal(out[key], plain[key]), (name, key)


def check_against_solve(name, P, sc, sol, out, metrics, instances):
    """shared with the GPU tier: metrics(X, U) -> the call's outputs at (X, U) on the solve's grid"""
    assert sc.warm and np.array_equal(sc.X[:, 0], sc.x0) and (out["stats"][:, 7] == 0).all()
    at_warm, at_out = metrics(sc.X, sc.U), metrics(out["X"], out["U"])
    worst = dict(b=0.0, e=0.0, stats=0.0)
    for i in instances:
        ref = reference(P, sc, sc.X, sc.U, i)
        for k in range(sc.N):
            g = sol.debug_lq(i, k)
            nc = g["nc"]
            assert nc == at_warm["nc"][i, k] == ref["nc"][k], (name, i, k)
            for key, mine, dump, mag, c in (("b", at_warm["defect"][i, k], g["b"], ref["mag"]["defect"][k], C["defect"]), ("e", at_warm["eq"][i, k, :nc], g["e"], ref["mag"]["eq"][k, :nc], C["eq"])):
                gap = np.abs(mine - dump)
                assert (gap[mag == 0] == 0).all()
                worst[key] = max(worst[key], float((gap[mag > 0] / (c * EPS * mag[mag > 0])).max()))
        for which, got, rf in ((0, at_warm, ref), (2, at_out, reference(P, sc, out["X"], out["U"], i))):
            m, ms = rf["mag"]["performance"], rf["mag"]["performance_sum"]
            allow = C["performance"] * EPS * m + EPS * ms
            merit, viol = out["stats"][i, which], out["stats"][i, which + 1]
            p = got["performance"][i]
            worst["stats"] = max(worst["stats"], abs(p[0] - merit) / allow[0], abs((p[3] + p[4]) - viol * viol) / (allow[3] + allow[4]))
    print(name, "against the solve's own dump and statistics: worst gap / allowance", json.dumps(worst))
    assert max(worst.values()) <= 1.0, (name, worst)


def test_emu_metrics_contracts(emu):
    """refused arguments; optional outputs left out; batch 1 against batch 3; a repeated call"""
    itf, orc, P = emu
    sc = KS.build(scenarios(), "trot_N7", itf, orc)
    X, U = perturbed(sc)
    B, N = sc.B, sc.N
    sol = api.GpuSolver(itf, max_batch=B, max_nodes=N)
    full = call(sol, sc, X, U, x0=sc.x0)
    again = call(sol, sc, X, U, x0=sc.x0)
    for k in OUTPUTS:
        assert np.array_equal(full[k], again[k]), k
    for k in OUTPUTS:                                                        # each output alone: the same bits
        assert np.array_equal(call(sol, sc, X, U, x0=sc.x0, want=(k,))[k], full[k]), k
    for i in range(B):                                                       # an instance alone: the same bits as inside the batch
        one = call(sol, sc, X, U, x0=sc.x0, rows=[i])
        for k in OUTPUTS:
            assert np.array_equal(one[k][0], full[k][i]), (i, k)

    def refused(s, **change):
        out = blank(B, N)
        kw = dict(batch=B, num_nodes=N, time_grid=sc.grid, X=X, U=U, target_times=sc.tt, target_states=sc.ts, sched_num=sc.nev, sched_times=sc.ev, sched_modes=sc.md,
                  performance=out["performance"])
        kw.update(change)
        with pytest.raises(abi.QmGpuError) as e:
            s.metrics(s.metrics_args(**kw))
        assert e.value.status == abi.ERR_INVALID_ARGUMENT and str(e.value), change
    refused(sol, batch=B + 1); refused(sol, num_nodes=N + 1); refused(sol, batch=0); refused(sol, num_nodes=0)
    for missing in ("time_grid", "X", "U", "target_times", "target_states", "sched_num", "sched_times", "sched_modes"):
        refused(sol, **{missing: None})
    refused(api.GpuSolver(itf, max_batch=B, max_nodes=N, dtype="f32"))
    assert interface_status(itf, sol) == abi.ERR_INVALID_ARGUMENT


def interface_status(itf, sol):
    """a null argument struct"""
    return itf.lib.qmgpu_mpc_metrics_batch(sol.handle, None)
