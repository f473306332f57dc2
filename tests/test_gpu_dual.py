"""-m gpu: the SQP dual solution (qmgpu_mpc_dual_batch) on the device.

On scenarios of kkt_scenarios.gpu_scenarios() with the line search off (so that out - iterate IS the full step): costates and nu per instance against the KKT
multipliers solved in high precision from the product's OWN LQ blocks (dual_reference.py) under that module's tolerance rule -- every instance, except
horizon_N200 (the reference on instance 0; nc and the padding on both) --, nc and the zero padding exact, the three KKT identities and
lambda_k = Sm_k dx_k + sv_lin_k on the product's own outputs, and the solves untouched by the call.  Every scenario prints its measured figures; with DUAL_RECORD
set to a file path they are collected there as JSON (the record of profiles/dual_kkt.json).  Then the contracts: nu without the dump, calls that do not match the
last solve, a flagged instance, several SQP iterations per call, poisoned scratch."""
import ctypes as C
import os

import numpy as np
import pytest

import dual_reference as DR
import kkt_scenarios as KS
import support as S
from test_emu_dual import check_identities

pytestmark = pytest.mark.gpu

RECORD = os.environ.get("DUAL_RECORD") or None
# N = 1 and 2; a trot with switches (nc 12 and 14: a swing foot's force rows appear); every gait (nc 12 .. 16); the event-aligned grid; force tracking; N = 200
SCENARIOS = ["horizon_N1", "horizon_N2", "trot_cold", "mixed_gaits", "event_grid", "force_tracking", "horizon_N200"]
REDUCED = {"horizon_N200": [0]}


@pytest.fixture(scope="module")
def force_tracking_setup():
    itf = KS.force_tracking_interface()
    return itf, S.Oracle(itf.problem)


def _scenario(name, itf, orc):
    sc = KS.build(KS.gpu_scenarios(), name, itf, orc)
    sc.line_search = False
    return sc


def _solve(G, sol, sc):
    import torch
    mb = G.MpcBatch(sc.x0, sc.tt, sc.ts, sc.nev, sc.ev, sc.md, sc.N, warm=(sc.X, sc.U) if sc.warm else None, line_search=sc.line_search,
                    time_grid=None if sc.uniform else sc.grid)
    if sc.contact is not None:
        mb.contact = G.dev(sc.contact, torch.float64)
        mb.args.ee_contact_ref = mb.contact.data_ptr()
    sol.mpc(mb.args)
    return mb, mb.results()


def _dual(sol, B, N, want_nu=True):
    """costate, nu, nc, status (numpy) of the last solve of `sol` (the outputs start as NaN / -1: every entry must be written)"""
    import torch
    lam = torch.full((B, N + 1, 30), float("nan"), dtype=torch.float64, device="cuda")
    nu = torch.full((B, N, 16), float("nan"), dtype=torch.float64, device="cuda")
    nc = torch.full((B, N), -1, dtype=torch.int32, device="cuda")
    st = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    sol.dual(B, N, lam, nu if want_nu else None, nc, st)
    torch.cuda.synchronize()
    return lam.cpu().numpy(), nu.cpu().numpy(), nc.cpu().numpy(), st.cpu().numpy()


def _value(sol, B, N):
    import torch
    Sm = torch.zeros((B, N + 1, 30, 30), dtype=torch.float64, device="cuda")
    Sv, sl = torch.zeros((B, N + 1, 30), dtype=torch.float64, device="cuda"), torch.zeros((B, N + 1, 30), dtype=torch.float64, device="cuda")
    sol.mpc_value_function(B, N, Sm, Sv, sl)
    torch.cuda.synchronize()
    return Sm.cpu().numpy(), sl.cpu().numpy()


@pytest.mark.parametrize("name", SCENARIOS)
def test_dual_equals_kkt_multipliers(interface, oracle, force_tracking_setup, name):
    import gpu_harness as G
    itf, orc = force_tracking_setup if name == "force_tracking" else (interface, oracle)
    sc = _scenario(name, itf, orc)
    B, N = sc.B, sc.N
    plain_sol = G.make_solver(itf, B, N)
    _, plain = _solve(G, plain_sol, sc)                                  # a handle that never makes the call, dump off
    plain_sol.close()
    sol = G.make_solver(itf, B, N)
    sol.enable_debug(True)
    mb, out = _solve(G, sol, sc)
    lam, nu, nc, st = _dual(sol, B, N)
    assert not st.any() and (out["stats"][:, 7] == 0).all() and (out["stats"][:, 4] == 1.0).all(), (name, st)
    rec, kept = DR.check_dual(sc, lam, nu, nc, sol.debug_lq, instances=REDUCED.get(name), record_path=RECORD)
    if name in ("trot_cold", "mixed_gaits"):
        assert {12, 14} <= set(rec["nc"]), rec["nc"]
    check_identities(name, sc, out, lam, nu, kept)
    # lambda_k = Sm_k dx_k + sv_lin_k (lambda_0 = sv_lin_0: dx_0 = 0), the value function of the same solve.  Both sides are fp64 routes to the same number, each
    # allowed tol_costate |lambda|_inf; the product formed here adds 64 eps (|Sm||dx| + |sv_lin|), and Sm's own relative error (the same rule) rides on |Sm||dx|
    Sm, sl = _value(sol, B, N)
    worst = 0.0
    for i, (blocks, ref, tol) in kept.items():
        dX = out["X"][i] - sc.X[i]
        assert not dX[0].any()
        L = np.abs(ref["lam"]).max()
        for k in range(N + 1):
            size = np.abs(Sm[i, k]) @ np.abs(dX[k]) + np.abs(sl[i, k])
            allow = 2 * tol[0] * L + (64 * DR.EPS + tol[0]) * size
            gap = np.abs(lam[i, k] - (Sm[i, k] @ dX[k] + sl[i, k]))
            worst = max(worst, float((gap / allow).max()))
            assert (gap <= allow).all(), (name, i, k, float(gap.max()))
        assert np.abs(lam[i, 0] - sl[i, 0]).max() <= 2 * tol[0] * L, (name, i)
    print(name, "costate against the value function: worst gap / allowance", worst)
    lam2, _, nc2, _ = _dual(sol, B, N, want_nu=False)                    # the optional output left out: the same costates
    assert np.array_equal(lam2, lam) and np.array_equal(nc2, nc)
    _, again = _solve(G, sol, sc)                                        # the next solve on the handle that made the calls
    for key in ("T", "X", "U", "mode", "stats"):
        assert np.array_equal(out[key], plain[key]), (name, key)
        assert np.array_equal(again[key], plain[key]), (name, key)
    sol.close()


def test_dual_needs_a_matching_sqp_solve_and_nu_needs_the_dump(interface, oracle):
    import torch
    import gpu_harness as G
    from qm_door_amd import abi
    sc = _scenario("horizon_N2", interface, oracle)
    B, N = sc.B, sc.N
    sol = G.make_solver(interface, B, N)
    lam = torch.zeros((B, N + 1, 30), dtype=torch.float64, device="cuda"); nu = torch.zeros((B, N, 16), dtype=torch.float64, device="cuda")

    def refused(s, b, n, with_nu=False):
        with pytest.raises(abi.QmGpuError) as e:
            s.dual(b, n, lam, nu if with_nu else None)
        assert e.value.status == abi.ERR_INVALID_ARGUMENT and str(e.value)
    refused(sol, B, N)                                                   # before any solve
    mb, _ = _solve(G, sol, sc)
    refused(sol, B - 1, N); refused(sol, B, N - 1); refused(sol, B, N + 1)
    refused(sol, B, N, with_nu=True)                                     # the solve wrote no dump
    sol.dual(B, N, lam)                                                  # the costates alone need none
    sol.enable_debug(True)
    refused(sol, B, N, with_nu=True)                                     # switched on after the solve: still not that solve's dump
    sol.mpc(mb.args)
    sol.dual(B, N, lam, nu)
    torch.cuda.synchronize()
    assert lam.cpu().numpy().any() and nu.cpu().numpy().any()
    mb.args.algorithm = 1                                                # QMGPU_ALG_DDP: the dual solution is the SQP solver's
    sol.mpc(mb.args)
    refused(sol, B, N); refused(sol, B, N, with_nu=True)
    f32 = G.make_solver(interface, B, N, dtype="f32")
    mb.args.algorithm = 0
    f32.mpc(mb.args)
    refused(f32, B, N)
    torch.cuda.synchronize()
    sol.close(); f32.close()


def test_a_flagged_instance_gets_a_zero_dual_solution(interface, oracle):
    """The construction of test_gpu_edges (the input weights negated through qmgpu_update_settings: the backward sweep's Cholesky fails, the instance is flagged):
    costate = nu = 0, nc still the node's, status non-zero, everything finite; the handle recovers once the settings are restored."""
    import gpu_harness as G
    from qm_door_amd import abi
    from test_gpu_edges import _batch
    B, N = 3, 8
    sol = G.make_solver(interface, B, N)
    sol.enable_debug(True)
    mb, _ = _batch(G, interface, oracle, B, N, seed=23)
    P2 = type(interface.problem).from_buffer_copy(interface.problem)
    for k in range(900):
        P2.settings.R_task[k] = -P2.settings.R_task[k]
    abi.check(interface.lib, interface.lib.qmgpu_update_settings(sol.handle, C.byref(P2.settings)))
    sol.mpc(mb.args)
    assert (mb.results()["stats"][:, 7] != 0).all()
    lam, nu, nc, st = _dual(sol, B, N)
    assert (st != 0).all(), st
    assert np.isfinite(lam).all() and np.isfinite(nu).all() and not lam.any() and not nu.any()
    assert ((nc >= 12) & (nc <= 16)).all(), nc
    abi.check(interface.lib, interface.lib.qmgpu_update_settings(sol.handle, C.byref(interface.problem.settings)))
    sol.mpc(mb.args)
    assert (mb.results()["stats"][:, 7] == 0).all()
    lam, nu, nc2, st = _dual(sol, B, N)
    assert not st.any() and lam.any() and nu.any() and np.isfinite(lam).all() and np.isfinite(nu).all() and np.array_equal(nc2, nc)
    sol.close()


def test_dual_of_several_sqp_iterations_belongs_to_the_last_one_performed(oracle):
    """sqp.sqpIteration = 3 in one call against three chained calls with sqp.sqpIteration = 1, each warm-started from the previous outputs (the batch of
    test_gpu_value_function.py): an instance that performed i iterations (out_stats[8]) has costates, nu and nc bit-identical to those taken after the i-th
    chained call."""
    import gpu_harness as G
    from qm_door_amd import api
    three, one = api.QMInterface(), api.QMInterface()
    three.problem.settings.sqp_iterations = 3
    for itf in (three, one):
        itf.problem.settings.delta_tol = 20.0
    B, N = 8, 30
    x0 = S.perturbed_states(three.initial_state, B, seed=11)
    x0[::2] = three.initial_state + 0.1 * (x0[::2] - three.initial_state)
    tgt = S.nominal_target(oracle, three.initial_state)
    tt = np.zeros((B, 1)); ts = np.tile(tgt, (B, 1, 1)).copy()
    nev, ev, md = S.trot_schedule(2.0, phase0=0.1)
    sn, se, sm = np.full(B, nev, dtype=np.int32), np.tile(ev, (B, 1)), np.tile(md, (B, 1))
    sol3 = G.make_solver(three, B, N)
    sol3.enable_debug(True)
    mb3 = G.MpcBatch(x0, tt, ts, sn, se, sm, N)
    sol3.mpc(mb3.args)
    r3 = mb3.results()
    lam3, nu3, nc3, st3 = _dual(sol3, B, N)
    its = r3["stats"][:, 8].astype(int)
    print("iterations performed", its.tolist())
    assert not st3.any() and its.max() == 3 and its.min() < 3, its
    sol1 = G.make_solver(one, B, N)
    sol1.enable_debug(True)
    warm = None
    for call in (1, 2, 3):
        mb = G.MpcBatch(x0, tt, ts, sn, se, sm, N, warm=warm)
        sol1.mpc(mb.args)
        r = mb.results()
        lam, nu, nc, _ = _dual(sol1, B, N)
        for i in np.nonzero(its == call)[0]:
            assert np.array_equal(r["X"][i], r3["X"][i]), (call, i)
            assert np.array_equal(lam[i], lam3[i]) and np.array_equal(nu[i], nu3[i]) and np.array_equal(nc[i], nc3[i]), (call, i)
        warm = (r["X"], r["U"])
    assert lam3.any() and nu3.any()
    sol3.close(); sol1.close()


def test_dual_reads_nothing_a_solve_leaves_unwritten(interface, oracle):
    """qmgpu_debug_poison (every scratch buffer and the LDS filled with NaN) before the solve: no NaN in the outputs, and the same bits as without it -- what the
    kernels read beyond the written rows (rows >= m~ of the records, rows >= nc of the dump) is masked."""
    import gpu_harness as G
    sc = _scenario("trot_cold", interface, oracle)
    B, N = sc.B, sc.N
    res = []
    for poison in (False, True):
        sol = G.make_solver(interface, B, N)
        sol.enable_debug(True)
        if poison:
            sol.debug_poison()
        _solve(G, sol, sc)
        res.append(_dual(sol, B, N))
        sol.close()
    for clean, poisoned in zip(*res):
        assert np.isfinite(poisoned).all()
        assert np.array_equal(clean, poisoned)
    assert res[1][0].any() and res[1][1].any() and not res[1][3].any()
