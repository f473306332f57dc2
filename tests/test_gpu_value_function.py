"""-m gpu: the SQP value function (qmgpu_mpc_value_function_batch, qmgpu_value_function_eval_batch) on the device.

On the scenarios of kkt_scenarios.gpu_scenarios(): Sm_k and sv_lin_k against the Hessian and the gradient of the optimal cost of the QP over nodes k .. N as a
function of its initial state, solved in high precision from the product's OWN LQ blocks (value_reference.py), under that module's tolerance rule -- all nodes of
all instances, except batch_beyond_cus (the reference on instances 0, 255, 256, 299) and horizon_N200 (the reference at nodes 0, N-3, N-2, N-1 of instance 0),
where the structural checks still run on every node of every instance.  Every scenario prints its measured figures; with VALUE_RECORD set to a file path they are
collected there as JSON (the record of profiles/value_function_kkt.json).  Then the evaluation against the plain statement of its formula, and the edges: a
flagged instance, several SQP iterations per call, calls that do not match the last solve, and a call next to a WBC pending on the overlap stream."""
import ctypes as C
import os

import numpy as np
import pytest

import kkt_scenarios as KS
import support as S
import value_reference as VR
from test_emu_value_function import check_evaluation

pytestmark = pytest.mark.gpu

RECORD = os.environ.get("VALUE_RECORD") or None
SCENARIOS = ["stance", "static_walk", "trot_cold", "flying_trot", "mixed_gaits", "event_grid", "barrier", "force_tracking", "horizon_N1", "horizon_N2", "batch_beyond_cus",
             "horizon_N200"]
# where the reference is NOT built on every node of every instance: (instances, nodes(N))
REDUCED = {"batch_beyond_cus": ([0, 255, 256, 299], lambda N: None), "horizon_N200": ([0], lambda N: [0, N - 3, N - 2, N - 1])}


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


def _value(sol, B, N):
    """Sm, Sv, sv_lin, x_lin (device tensors) and status (numpy) of the last solve of `sol` (the outputs start as NaN / -1: every entry must be written)"""
    import torch
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")  # noqa: E731
    Sm, Sv, sl, xl = nan(B, N + 1, 30, 30), nan(B, N + 1, 30), nan(B, N + 1, 30), nan(B, N + 1, 30)
    st = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    sol.mpc_value_function(B, N, Sm, Sv, sl, xl, st)
    torch.cuda.synchronize()
    return Sm, Sv, sl, xl, st.cpu().numpy()


def _host(*tensors):
    return tuple(t.cpu().numpy() for t in tensors)


@pytest.mark.parametrize("name", SCENARIOS)
def test_value_function_equals_kkt_cost_to_go(interface, oracle, force_tracking_setup, name):
    import gpu_harness as G
    itf, orc = force_tracking_setup if name == "force_tracking" else (interface, oracle)
    sc = KS.build(KS.gpu_scenarios(), name, itf, orc)
    plain_sol = G.make_solver(itf, sc.B, sc.N)
    _, plain = _solve(G, plain_sol, sc)                                  # a handle that never makes the call
    plain_sol.close()
    sol = G.make_solver(itf, sc.B, sc.N)
    sol.enable_debug(True)
    mb, out = _solve(G, sol, sc)
    *dev, st = _value(sol, sc.B, sc.N)
    Sm, Sv, sl, xl = _host(*dev)
    assert not st.any() and (out["stats"][:, 7] == 0).all(), (name, st)
    instances, nodes = REDUCED.get(name, (None, lambda N: None))
    VR.check_value(sc, Sm, Sv, sl, xl, sol.debug_lq, instances=instances, nodes=nodes(sc.N), record_path=RECORD)
    _, again = _solve(G, sol, sc)                                        # the next solve on the handle that made the call
    for key in ("T", "X", "U", "mode", "stats"):
        assert np.array_equal(out[key], plain[key]), (name, key)
        assert np.array_equal(again[key], plain[key]), (name, key)
    sol.close()


@pytest.mark.parametrize("name", ["mixed_gaits", "horizon_N1"])
def test_value_function_evaluation(interface, oracle, name):
    import torch
    import gpu_harness as G
    sc = KS.build(KS.gpu_scenarios(), name, interface, oracle)
    sol = G.make_solver(interface, sc.B, sc.N)
    mb, out = _solve(G, sol, sc)
    Sm, Sv, _, _, _ = _value(sol, sc.B, sc.N)
    Sm, Sv = _host(Sm, Sv)
    check_evaluation(name, sol, sc, out["T"], Sm, Sv, to_dev=lambda a: G.dev(a, torch.float64), to_host=lambda t: (torch.cuda.synchronize(), t.cpu().numpy())[1],
                     new=lambda shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda"))
    sol.close()


def test_a_flagged_instance_gets_a_zero_value_function(interface, oracle):
    """The construction of test_gpu_feedback.py::test_a_flagged_instance_gets_the_feed_forward_policy (the input weights negated through qmgpu_update_settings: the
    backward sweep's Cholesky fails, the instance is flagged): Sm = Sv = sv_lin = 0, x_lin still the iterate, status non-zero, everything finite; the handle
    recovers once the settings are restored."""
    import gpu_harness as G
    from qm_door_amd import abi
    from test_gpu_edges import _batch
    B, N = 3, 8
    sol = G.make_solver(interface, B, N)
    mb, (x0, *_rest) = _batch(G, interface, oracle, B, N, seed=23)
    P2 = type(interface.problem).from_buffer_copy(interface.problem)
    for k in range(900):
        P2.settings.R_task[k] = -P2.settings.R_task[k]
    abi.check(interface.lib, interface.lib.qmgpu_update_settings(sol.handle, C.byref(P2.settings)))
    sol.mpc(mb.args)
    bad = mb.results()
    assert (bad["stats"][:, 7] != 0).all()
    *dev, st = _value(sol, B, N)
    Sm, Sv, sl, xl = _host(*dev)
    assert (st != 0).all(), st
    for arr in (Sm, Sv, sl, xl):
        assert np.isfinite(arr).all()
    assert not Sm.any() and not Sv.any() and not sl.any()
    assert np.array_equal(xl, bad["X"])                                  # a flagged instance takes no step: its output IS the iterate it was linearised at
    abi.check(interface.lib, interface.lib.qmgpu_update_settings(sol.handle, C.byref(interface.problem.settings)))
    sol.mpc(mb.args)
    assert (mb.results()["stats"][:, 7] == 0).all()
    *dev, st = _value(sol, B, N)
    Sm, Sv, sl, xl = _host(*dev)
    assert not st.any() and Sm.any() and np.isfinite(Sm).all() and np.isfinite(Sv).all()
    sol.close()


def test_value_function_of_several_sqp_iterations_belongs_to_the_last_one_performed(oracle):
    """sqp.sqpIteration = 3 in one call against three chained calls with sqp.sqpIteration = 1, each warm-started from the previous outputs (the batch of
    test_gpu_feedback.py::test_gains_of_several_sqp_iterations_belong_to_the_last_one_performed): an instance that performed i iterations (out_stats[8]) has Sm,
    Sv, x_lin bit-identical to those taken after the i-th chained call."""
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
    *dev, st3 = _value(sol3, B, N)
    Sm3, Sv3, _, xl3 = _host(*dev)
    its = r3["stats"][:, 8].astype(int)
    print("iterations performed", its.tolist())
    assert not st3.any() and its.max() == 3 and its.min() < 3, its
    sol1 = G.make_solver(one, B, N)
    warm = None
    for call in (1, 2, 3):
        mb = G.MpcBatch(x0, tt, ts, sn, se, sm, N, warm=warm)
        sol1.mpc(mb.args)
        r = mb.results()
        *dev, _ = _value(sol1, B, N)
        Sm, Sv, _, xl = _host(*dev)
        for i in np.nonzero(its == call)[0]:
            assert np.array_equal(r["X"][i], r3["X"][i]), (call, i)
            assert np.array_equal(Sm[i], Sm3[i]) and np.array_equal(Sv[i], Sv3[i]) and np.array_equal(xl[i], xl3[i]), (call, i)
        warm = (r["X"], r["U"])
    sol3.close(); sol1.close()


def test_value_function_needs_a_matching_sqp_solve(interface, oracle):
    import torch
    import gpu_harness as G
    from qm_door_amd import abi
    sc = KS.build(KS.gpu_scenarios(), "horizon_N2", interface, oracle)
    B, N = sc.B, sc.N
    sol = G.make_solver(interface, B, N)
    Sm = torch.zeros((B, N + 1, 30, 30), dtype=torch.float64, device="cuda"); Sv = torch.zeros((B, N + 1, 30), dtype=torch.float64, device="cuda")

    def refused(s, b, n):
        with pytest.raises(abi.QmGpuError) as e:
            s.mpc_value_function(b, n, Sm, Sv)
        assert e.value.status == abi.ERR_INVALID_ARGUMENT and str(e.value)
    refused(sol, B, N)                                                   # before any solve
    mb, _ = _solve(G, sol, sc)
    refused(sol, B - 1, N); refused(sol, B, N - 1); refused(sol, B, N + 1)
    sol.mpc_value_function(B, N, Sm, Sv)
    mb.args.algorithm = 1                                                # QMGPU_ALG_DDP: the value function is the SQP solver's
    sol.mpc(mb.args)
    refused(sol, B, N)
    f32 = G.make_solver(interface, B, N, dtype="f32")
    mb.args.algorithm = 0
    f32.mpc(mb.args)
    refused(f32, B, N)
    torch.cuda.synchronize()
    sol.close(); f32.close()


def test_value_function_runs_next_to_a_pending_overlap_wbc(interface, oracle):
    """With qmgpu_set_overlap on, a value-function call behind qmgpu_cycle_batch does not join the WBC pending on the overlap stream and disturbs nothing: its
    outputs and the WBC outputs are bit-identical to the serial order (overlap off)."""
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
        *dev, st = _value(sol, B, N)
        sol.synchronize()
        res.append((_host(*dev), st, wb.results(), mb.results()))
        sol.close()
    (va, sa, wa, ma), (vb, sb, wbr, mbr) = res
    for x, y in zip(va, vb):
        assert np.array_equal(x, y)
    assert np.array_equal(sa, sb) and va[0].any()
    assert np.array_equal(wa["out"], wbr["out"]) and np.array_equal(wa["status"], wbr["status"]) and np.array_equal(wa["input_last"], wbr["input_last"])
    assert np.array_equal(ma["X"], mbr["X"]) and np.array_equal(ma["U"], mbr["U"])
