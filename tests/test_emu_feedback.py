"""CPU tier: the feedback-policy kernels (kernels/feedback_kernel.h) on host threads (tests/emu), on every scenario of kkt_scenarios.emu_scenarios(): the gains of
every node of every instance against the reference from the emulated library's OWN LQ blocks, the structural properties, the policy evaluation against the plain
statement of its formula, and the solve untouched by the feedback call."""
import numpy as np
import pytest

import feedback_reference as FR
import kkt_scenarios as KS
import support as S
from qm_door_amd import abi, api
from test_kkt_reference import emu_solve


@pytest.fixture(scope="module")
def emu():
    lib = abi.load_library(S.build_emu())
    itf = api.QMInterface(lib=lib)
    return itf, S.Oracle(itf.problem)


def _feedback(sol, sc, out):
    B, N = sc.B, sc.N
    K, uff, st = np.full((B, N + 1, 30, 30), np.nan), np.full((B, N + 1, 30), np.nan), np.full(B, -1, dtype=np.int32)
    sol.mpc_feedback(B, N, out["X"], out["U"], K, uff, st)
    return K, uff, st


@pytest.mark.parametrize("name", list(KS.emu_scenarios()))
def test_emu_gains_equal_kkt_sensitivities(emu, name):
    itf, orc = emu
    sc = KS.build(KS.emu_scenarios(), name, itf, orc)
    _, plain = emu_solve(itf, sc, True)
    sol, out = emu_solve(itf, sc, True)
    K, uff, st = _feedback(sol, sc, out)
    assert not st.any()
    FR.check_structure(name, out, K, uff)
    FR.check_gains(sc, out, K, sol.debug_lq)
    for key in ("T", "X", "U", "mode", "stats"):
        assert np.array_equal(out[key], plain[key]), (name, key)
    # a second solve on the handle that made the feedback call: bit-identical to one that never did
    B, N = sc.B, sc.N
    oT, oX, oU, oM, oS = np.zeros((B, N + 1)), np.zeros((B, N + 1, 30)), np.zeros((B, N, 30)), np.zeros((B, N + 1), dtype=np.int32), np.zeros((B, abi.NSTATS))
    a = sol.mpc_args(B, N, sc.x0, sc.tt, sc.ts, sc.nev, sc.ev, sc.md, oT, oX, oU, oM, oS, t0=np.zeros(B) if sc.uniform else None,
                     time_grid=None if sc.uniform else sc.grid, warm_x=sc.X if sc.warm else None, warm_u=sc.U if sc.warm else None, line_search=sc.line_search,
                     ee_contact_ref=sc.contact)
    sol.mpc(a)
    for key, got in (("T", oT), ("X", oX), ("U", oU), ("mode", oM), ("stats", oS)):
        assert np.array_equal(got, plain[key]), (name, key)


@pytest.mark.parametrize("name", ["static_walk", "event_grid"])
def test_emu_policy_evaluation_with_feedback(emu, name):
    """u = uff(t) + K(t) x_measured on a node, inside an interval, before t_0 and beyond t_N against the numpy statement (64 eps (|uff(t)| + |K(t)||x|) row by
    row: two 31-term accumulations); x_out / mode_out bit-identical to qmgpu_policy_eval_batch; x_measured = X_k at T_k returns U_k to the fixed-point bound."""
    itf, orc = emu
    sc = KS.build(KS.emu_scenarios(), name, itf, orc)
    sol, out = emu_solve(itf, sc, False)
    K, uff, _ = _feedback(sol, sc, out)
    B, N = sc.B, sc.N
    rng = np.random.default_rng(3)
    x_ff, u_ff, m_ff, x_fb, u_fb, m_fb = np.zeros((B, 30)), np.zeros((B, 30)), np.zeros(B, dtype=np.int32), np.zeros((B, 30)), np.zeros((B, 30)), np.zeros(B, dtype=np.int32)
    for t in FR.policy_cases(out["T"], rng):
        xm = out["X"][:, 0] + 0.05 * rng.standard_normal((B, 30))
        sol.policy_eval(B, N, out["T"], out["X"], out["U"], out["mode"], t, x_ff, u_ff, m_ff)
        sol.policy_eval_feedback(B, N, out["T"], out["X"], uff, K, out["mode"], t, xm, x_fb, u_fb, m_fb)
        u, bound = FR.policy_reference(out["T"], out["X"], uff, K, t, xm)
        print(name, "policy: worst error / bound", float((np.abs(u_fb - u) / np.where(bound > 0, bound, 1.0)).max()))
        assert (np.abs(u_fb - u) <= bound).all(), name
        assert np.array_equal(x_fb, x_ff) and np.array_equal(m_fb, m_ff), name
    for k in (0, N // 2, N - 1):
        xm = np.ascontiguousarray(out["X"][:, k])
        sol.policy_eval_feedback(B, N, out["T"], out["X"], uff, K, out["mode"], np.ascontiguousarray(out["T"][:, k]), xm, x_fb, u_fb, m_fb)
        for i in range(B):
            assert (np.abs(u_fb[i] - out["U"][i, k]) <= FR.fixed_point_bound(K[i, k], xm[i], out["U"][i, k])).all(), (name, i, k)


def test_emu_feedback_needs_a_matching_solve(emu):
    itf, orc = emu
    sc = KS.build(KS.emu_scenarios(), "stance", itf, orc)
    B, N = sc.B, sc.N
    fresh = api.GpuSolver(itf, max_batch=B, max_nodes=N)
    K, uff = np.zeros((B, N + 1, 30, 30)), np.zeros((B, N + 1, 30))
    with pytest.raises(abi.QmGpuError) as e:
        fresh.mpc_feedback(B, N, sc.X, sc.U, K, uff)
    assert e.value.status == abi.ERR_INVALID_ARGUMENT
    sol, out = emu_solve(itf, sc, False)
    for b, n in ((B - 1, N), (B, N - 1)):
        with pytest.raises(abi.QmGpuError) as e:
            sol.mpc_feedback(b, n, out["X"], out["U"], K, uff)
        assert e.value.status == abi.ERR_INVALID_ARGUMENT
    sol.mpc_feedback(B, N, out["X"], out["U"], K, uff)
