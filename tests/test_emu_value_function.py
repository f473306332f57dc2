"""CPU tier: the value-function kernels (kernels/value_kernel.h) on host threads (tests/emu), on every scenario of kkt_scenarios.emu_scenarios(): Sm and sv_lin of
every node of every instance against the reference from the emulated library's OWN LQ blocks (value_reference.py), the structural properties, the evaluation
against the plain statement of its formula, and the solve untouched by the call."""
import numpy as np
import pytest

import feedback_reference as FR
import kkt_scenarios as KS
import support as S
import value_reference as VR
from qm_door_amd import abi, api
from test_kkt_reference import emu_solve


@pytest.fixture(scope="module")
def emu():
    lib = abi.load_library(S.build_emu())
    itf = api.QMInterface(lib=lib)
    return itf, S.Oracle(itf.problem)


def _value(sol, sc):
    """Sm, Sv, sv_lin, x_lin, status of the last solve (the outputs start as NaN / -1: every entry must be written)"""
    B, N = sc.B, sc.N
    Sm, Sv, sl, xl = np.full((B, N + 1, 30, 30), np.nan), np.full((B, N + 1, 30), np.nan), np.full((B, N + 1, 30), np.nan), np.full((B, N + 1, 30), np.nan)
    st = np.full(B, -1, dtype=np.int32)
    sol.mpc_value_function(B, N, Sm, Sv, sl, xl, st)
    return Sm, Sv, sl, xl, st


@pytest.mark.parametrize("name", list(KS.emu_scenarios()))
def test_emu_value_function_equals_kkt_cost_to_go(emu, name):
    itf, orc = emu
    sc = KS.build(KS.emu_scenarios(), name, itf, orc)
    _, plain = emu_solve(itf, sc, True)                                  # a handle that never makes the call
    sol, out = emu_solve(itf, sc, True)
    Sm, Sv, sl, xl, st = _value(sol, sc)
    assert not st.any() and (out["stats"][:, 7] == 0).all()
    VR.check_value(sc, Sm, Sv, sl, xl, sol.debug_lq)
    Sm2, Sv2 = np.full_like(Sm, np.nan), np.full_like(Sv, np.nan)       # the optional outputs left out: the same Sm, Sv
    sol.mpc_value_function(sc.B, sc.N, Sm2, Sv2)
    assert np.array_equal(Sm2, Sm) and np.array_equal(Sv2, Sv)
    for key in ("T", "X", "U", "mode", "stats"):
        assert np.array_equal(out[key], plain[key]), (name, key)
    # a second solve on the handle that made the call: bit-identical to one that never did
    B, N = sc.B, sc.N
    oT, oX, oU, oM, oS = np.zeros((B, N + 1)), np.zeros((B, N + 1, 30)), np.zeros((B, N, 30)), np.zeros((B, N + 1), dtype=np.int32), np.zeros((B, abi.NSTATS))
    a = sol.mpc_args(B, N, sc.x0, sc.tt, sc.ts, sc.nev, sc.ev, sc.md, oT, oX, oU, oM, oS, t0=np.zeros(B) if sc.uniform else None,
                     time_grid=None if sc.uniform else sc.grid, warm_x=sc.X if sc.warm else None, warm_u=sc.U if sc.warm else None, line_search=sc.line_search,
                     ee_contact_ref=sc.contact)
    sol.mpc(a)
    for key, got in (("T", oT), ("X", oX), ("U", oU), ("mode", oM), ("stats", oS)):
        assert np.array_equal(got, plain[key]), (name, key)


def check_evaluation(name, sol, sc, T, Sm, Sv, to_dev=lambda a: a, to_host=lambda a: a, new=np.zeros):
    """dfdx = Sv(t) + Sm(t) x, dfdxx = Sm(t) on a node, inside an interval, before t_0 and beyond t_N for a random x against the numpy statement: dfdx row by row
    within 64 eps (|Sv(t)| + |Sm(t)||x|) (two 31-term accumulations, the kernel's and numpy's, each below 31 eps times that sum), dfdxx symmetric bit for bit and
    within 4 eps of the entry's largest magnitude over the nodes of the numpy statement (two products and a sum, one rounding each, on either side).  Shared with the GPU tier (to_dev / to_host / new: torch there)."""
    B, N = sc.B, sc.N
    rng = np.random.default_rng(3)
    Sd, vd, Td = to_dev(Sm), to_dev(Sv), to_dev(T)
    for t in FR.policy_cases(T, rng):
        x = sc.x0 + 0.05 * rng.standard_normal((B, 30))
        g, H = new((B, 30)), new((B, 30, 30))
        sol.value_function_eval(B, N, Td, Sd, vd, to_dev(t), to_dev(x), g, H)
        g, H = to_host(g), to_host(H)
        ref_g, ref_H, bound = VR.eval_reference(T, Sm, Sv, t, x)
        print(name, "evaluation: worst error / bound", float((np.abs(g - ref_g) / np.where(bound > 0, bound, 1.0)).max()))
        assert np.array_equal(H, np.swapaxes(H, 1, 2)), name
        assert (np.abs(H - ref_H) <= 4 * VR.EPS * np.abs(Sm).max(axis=1)).all(), name
        assert (np.abs(g - ref_g) <= bound).all(), name


@pytest.mark.parametrize("name", ["static_walk", "event_grid"])
def test_emu_value_function_evaluation(emu, name):
    itf, orc = emu
    sc = KS.build(KS.emu_scenarios(), name, itf, orc)
    sol, out = emu_solve(itf, sc, False)
    Sm, Sv, _, _, _ = _value(sol, sc)
    check_evaluation(name, sol, sc, out["T"], Sm, Sv)


def test_emu_value_function_needs_a_matching_solve(emu):
    itf, orc = emu
    sc = KS.build(KS.emu_scenarios(), "stance", itf, orc)
    B, N = sc.B, sc.N
    fresh = api.GpuSolver(itf, max_batch=B, max_nodes=N)
    Sm, Sv = np.zeros((B, N + 1, 30, 30)), np.zeros((B, N + 1, 30))
    with pytest.raises(abi.QmGpuError) as e:
        fresh.mpc_value_function(B, N, Sm, Sv)
    assert e.value.status == abi.ERR_INVALID_ARGUMENT
    sol, _ = emu_solve(itf, sc, False)
    for b, n in ((B - 1, N), (B, N - 1)):
        with pytest.raises(abi.QmGpuError) as e:
            sol.mpc_value_function(b, n, Sm, Sv)
        assert e.value.status == abi.ERR_INVALID_ARGUMENT
    sol.mpc_value_function(B, N, Sm, Sv)
    assert Sm.any()
