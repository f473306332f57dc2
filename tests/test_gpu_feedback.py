"""-m gpu: the SQP feedback policy (qmgpu_mpc_feedback_batch, qmgpu_policy_eval_feedback_batch) on the device.

Gains: on every scenario of kkt_scenarios.gpu_scenarios(), K_k against the sensitivity of the first input of the QP over nodes k .. N to its initial state, solved
in high precision from the product's OWN LQ blocks (feedback_reference.py), under that module's tolerance rule; all nodes except for N = 200, 300, where the
nodes of feedback_reference.checked_nodes are compared.  The structural checks (uff_k + K_k X_k = U_k, the last entry a copy, zero force rows of swing feet) run on
every node of every instance.  Every scenario prints its measured figures; with FEEDBACK_RECORD set to a file path they are collected there as JSON (the record
of profiles/feedback_policy_kkt.json).  Then the policy evaluation against the plain statement of its formula, and the edges: a flagged instance, several SQP
iterations per call, calls that do not match the last solve, and a feedback call next to a WBC pending on the overlap stream."""
import ctypes as C
import os

import numpy as np
import pytest

import feedback_reference as FR
import kkt_scenarios as KS
import support as S

pytestmark = pytest.mark.gpu

RECORD = os.environ.get("FEEDBACK_RECORD") or None


@pytest.fixture(scope="module")
def force_tracking_setup():
    itf = KS.force_tracking_interface()
    return itf, S.Oracle(itf.problem)


def _solve(G, sol, sc):
    import torch
    mb = G.MpcBatch(sc.x0, sc.tt, sc.ts, sc.nev, sc.ev, sc.md, sc.N, warm=(sc.X, sc.U) if sc.warm else None, line_search=sc.line_search,
                    time_grid=None if sc.uniform else sc.grid)
    if sc.contact is not None:
        mb.contact = G.dev(sc.contact, torch.float64)
        mb.args.ee_contact_ref = mb.contact.data_ptr()
    sol.mpc(mb.args)
    return mb, mb.results()


def _feedback(sol, mb, X=None, U=None):
    """K, uff, status of the last solve of `sol` as numpy arrays (the outputs start as NaN / -1: every entry must be written)"""
    import torch
    B, N = mb.B, mb.N
    K = torch.full((B, N + 1, 30, 30), float("nan"), dtype=torch.float64, device="cuda")
    uff = torch.full((B, N + 1, 30), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    sol.mpc_feedback(B, N, mb.oX if X is None else X, mb.oU if U is None else U, K, uff, st)
    torch.cuda.synchronize()
    return K, uff, st.cpu().numpy()


@pytest.mark.parametrize("name", list(KS.gpu_scenarios()))
def test_gains_equal_kkt_sensitivities(interface, oracle, force_tracking_setup, name):
    import gpu_harness as G
    itf, orc = force_tracking_setup if name == "force_tracking" else (interface, oracle)
    sc = KS.build(KS.gpu_scenarios(), name, itf, orc)
    plain_sol = G.make_solver(itf, sc.B, sc.N)
    _, plain = _solve(G, plain_sol, sc)                                  # a handle that never makes the feedback call
    plain_sol.close()
    sol = G.make_solver(itf, sc.B, sc.N)
    sol.enable_debug(True)
    mb, out = _solve(G, sol, sc)
    K, uff, st = _feedback(sol, mb)
    K, uff = K.cpu().numpy(), uff.cpu().numpy()
    assert not st.any(), (name, st)
    FR.check_structure(name, out, K, uff)
    FR.check_gains(sc, out, K, sol.debug_lq, record_path=RECORD)
    _, again = _solve(G, sol, sc)                                        # the next solve on the handle that made the call
    for key in ("T", "X", "U", "mode", "stats"):
        assert np.array_equal(out[key], plain[key]), (name, key)
        assert np.array_equal(again[key], plain[key]), (name, key)
    sol.close()


@pytest.mark.parametrize("name", ["mixed_gaits", "event_grid", "horizon_N1", "horizon_N200"])
def test_policy_evaluation_with_feedback(interface, oracle, name):
    """u = uff(t) + K(t) x_measured on a node, inside an interval, before t_0 and beyond t_N for a random x_measured against the numpy statement: row by row within
    64 eps (|uff(t)| + |K(t)||x_measured|) (two 31-term accumulations, the kernel's and numpy's, each below 31 eps times that sum); x_out / mode_out
    bit-identical to qmgpu_policy_eval_batch; x_measured = X_k at t = T_k returns U_k to the fixed-point bound."""
    import torch
    import gpu_harness as G
    sc = KS.build(KS.gpu_scenarios(), name, interface, oracle)
    sol = G.make_solver(interface, sc.B, sc.N)
    mb, out = _solve(G, sol, sc)
    K, uff, _ = _feedback(sol, mb)
    Kh, fh = K.cpu().numpy(), uff.cpu().numpy()
    B, N, f64 = sc.B, sc.N, torch.float64
    z = lambda *shape, dtype=f64: torch.zeros(shape, dtype=dtype, device="cuda")  # noqa: E731
    x_ff, u_ff, m_ff, x_fb, u_fb, m_fb = z(B, 30), z(B, 30), z(B, dtype=torch.int32), z(B, 30), z(B, 30), z(B, dtype=torch.int32)
    rng = np.random.default_rng(3)
    for t in FR.policy_cases(out["T"], rng):
        xm = out["X"][:, 0] + 0.05 * rng.standard_normal((B, 30))
        td, xd = G.dev(t, f64), G.dev(xm, f64)
        sol.policy_eval(B, N, mb.oT, mb.oX, mb.oU, mb.oM, td, x_ff, u_ff, m_ff)
        sol.policy_eval_feedback(B, N, mb.oT, mb.oX, uff, K, mb.oM, td, xd, x_fb, u_fb, m_fb)
        torch.cuda.synchronize()
        u, bound = FR.policy_reference(out["T"], out["X"], fh, Kh, t, xm)
        err = np.abs(u_fb.cpu().numpy() - u)
        print(name, "policy: worst error / bound", float((err / np.where(bound > 0, bound, 1.0)).max()))
        assert (err <= bound).all(), name
        assert torch.equal(x_fb, x_ff) and torch.equal(m_fb, m_ff), name
    for k in sorted({0, N // 2, N - 1}):
        xm = np.ascontiguousarray(out["X"][:, k])
        sol.policy_eval_feedback(B, N, mb.oT, mb.oX, uff, K, mb.oM, G.dev(out["T"][:, k], f64), G.dev(xm, f64), x_fb, u_fb, m_fb)
        got = u_fb.cpu().numpy()
        for i in range(B):
            assert (np.abs(got[i] - out["U"][i, k]) <= FR.fixed_point_bound(Kh[i, k], xm[i], out["U"][i, k])).all(), (name, i, k)
    sol.close()


def test_a_flagged_instance_gets_the_feed_forward_policy(interface, oracle):
    """The scenario of test_gpu_edges.py::test_a_failed_factorisation_flags_the_instance_and_leaves_the_iterate (the input weights negated through
    qmgpu_update_settings: the backward sweep's Cholesky fails, the instance is flagged, nothing faults): K = 0, uff = U, status non-zero, everything finite."""
    import gpu_harness as G
    from qm_door_amd import abi
    from test_gpu_edges import _batch
    B, N = 3, 8
    sol = G.make_solver(interface, B, N)
    mb, _ = _batch(G, interface, oracle, B, N, seed=23)
    P2 = type(interface.problem).from_buffer_copy(interface.problem)
    for k in range(900):
        P2.settings.R_task[k] = -P2.settings.R_task[k]
    abi.check(interface.lib, interface.lib.qmgpu_update_settings(sol.handle, C.byref(P2.settings)))
    sol.mpc(mb.args)
    bad = mb.results()
    assert (bad["stats"][:, 7] != 0).all()
    K, uff, st = _feedback(sol, mb)
    K, uff = K.cpu().numpy(), uff.cpu().numpy()
    assert (st != 0).all(), st
    assert np.isfinite(K).all() and np.isfinite(uff).all()
    assert not K.any()
    assert np.array_equal(uff[:, :N], bad["U"]) and np.array_equal(uff[:, N], bad["U"][:, N - 1])
    abi.check(interface.lib, interface.lib.qmgpu_update_settings(sol.handle, C.byref(interface.problem.settings)))
    sol.mpc(mb.args)
    assert (mb.results()["stats"][:, 7] == 0).all()
    K, uff, st = _feedback(sol, mb)
    assert not st.any() and K.cpu().numpy().any()
    sol.close()


def test_gains_of_several_sqp_iterations_belong_to_the_last_one_performed(oracle):
    """sqp.sqpIteration = 3 in one call against three chained calls with sqp.sqpIteration = 1, each warm-started from the previous outputs: an instance that
    performed i iterations (out_stats[8]) has K, uff bit-identical to those taken after the i-th chained call.  The batch of
    test_gpu_mpc.py::test_sqp_convergence_test_per_instance with deltaTol 20 instead of 5: with three iterations at most, six instances stop after the second
    (primal step below deltaTol) and two run all three."""
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
    mb3 = G.MpcBatch(x0, tt, ts, sn, se, sm, N)
    sol3.mpc(mb3.args)
    r3 = mb3.results()
    K3, f3, st3 = _feedback(sol3, mb3)
    K3, f3 = K3.cpu().numpy(), f3.cpu().numpy()
    its = r3["stats"][:, 8].astype(int)
    print("iterations performed", its.tolist())
    assert not st3.any() and its.max() == 3 and its.min() < 3, its
    sol1 = G.make_solver(one, B, N)
    warm = None
    for call in (1, 2, 3):
        mb = G.MpcBatch(x0, tt, ts, sn, se, sm, N, warm=warm)
        sol1.mpc(mb.args)
        r = mb.results()
        K, f, _ = _feedback(sol1, mb)
        K, f = K.cpu().numpy(), f.cpu().numpy()
        for i in np.nonzero(its == call)[0]:
            assert np.array_equal(r["X"][i], r3["X"][i]) and np.array_equal(r["U"][i], r3["U"][i]), (call, i)
            assert np.array_equal(K[i], K3[i]) and np.array_equal(f[i], f3[i]), (call, i)
        warm = (r["X"], r["U"])
    sol3.close(); sol1.close()


def test_feedback_needs_a_matching_sqp_solve(interface, oracle):
    import torch
    import gpu_harness as G
    from qm_door_amd import abi
    sc = KS.build(KS.gpu_scenarios(), "horizon_N2", interface, oracle)
    B, N = sc.B, sc.N
    sol = G.make_solver(interface, B, N)
    K = torch.zeros((B, N + 1, 30, 30), dtype=torch.float64, device="cuda"); uff = torch.zeros((B, N + 1, 30), dtype=torch.float64, device="cuda")
    X, U = G.dev(sc.X, torch.float64), G.dev(sc.U, torch.float64)

    def refused(b, n):
        with pytest.raises(abi.QmGpuError) as e:
            sol.mpc_feedback(b, n, X, U, K, uff)
        assert e.value.status == abi.ERR_INVALID_ARGUMENT and str(e.value)
    refused(B, N)                                                        # before any solve
    mb, _ = _solve(G, sol, sc)
    refused(B - 1, N); refused(B, N - 1); refused(B, N + 1)
    sol.mpc_feedback(B, N, mb.oX, mb.oU, K, uff)
    mb.args.algorithm = 1                                                # QMGPU_ALG_DDP: the feedback policy is the SQP solver's
    sol.mpc(mb.args)
    refused(B, N)
    f32 = G.make_solver(interface, B, N, dtype="f32")
    mb.args.algorithm = 0
    f32.mpc(mb.args)
    with pytest.raises(abi.QmGpuError) as e:
        f32.mpc_feedback(B, N, mb.oX, mb.oU, K, uff)
    assert e.value.status == abi.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    sol.close(); f32.close()


def test_feedback_runs_next_to_a_pending_overlap_wbc(interface, oracle):
    """With qmgpu_set_overlap on, a feedback call behind qmgpu_cycle_batch does not join the WBC pending on the overlap stream and disturbs nothing: the gains
    and the WBC outputs are bit-identical to the serial order (overlap off)."""
    import torch
    import gpu_harness as G
    from test_gpu_edges import _batch
    B, N = 6, 20
    res = []
    for overlap in (False, True):
        sol = G.make_solver(interface, B, N)
        sol.set_overlap(overlap)
        mb, (x0, *_rest) = _batch(G, interface, oracle, B, N, seed=29)
        rbd = np.array([S.rbd_from_state(oracle, x0[i]) for i in range(B)])
        wb = G.WbcBatch(rbd, np.full(B, 0.002), np.full(B, 20.0), np.zeros((B, 30)))
        sol.cycle(mb.args, G.dev(np.full(B, 0.004), torch.float64), wb.args)
        K, uff, st = _feedback(sol, mb)
        sol.synchronize()
        res.append((K.cpu().numpy(), uff.cpu().numpy(), st, wb.results(), mb.results()))
        sol.close()
    (Ka, fa, sa, wa, ma), (Kb, fb, sb, wbr, mbr) = res
    assert np.array_equal(Ka, Kb) and np.array_equal(fa, fb) and np.array_equal(sa, sb) and Ka.any()
    assert np.array_equal(wa["out"], wbr["out"]) and np.array_equal(wa["status"], wbr["status"]) and np.array_equal(wa["input_last"], wbr["input_last"])
    assert np.array_equal(ma["X"], mbr["X"]) and np.array_equal(ma["U"], mbr["U"])
