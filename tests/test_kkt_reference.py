"""CPU tier: the high-precision one-step reference (kkt_reference.py) checked against a 50-digit solve, the oracle's projected-Riccati step checked against the
reference on every scenario of the GPU tier (kkt_scenarios.py), and the host-emulated kernels (tests/emu) checked against the reference on a reduced set."""
import mpmath as mp
import numpy as np
import pytest

import kkt_reference as KR
import kkt_scenarios as KS
import support as S
from qm_door_amd import abi, api


# ------------------------------------------------------------------------------------------------ (a) the reference against mpmath
def _random_lq(rng, N=3, nx=4, nu=3, nc=2):
    """a small well-conditioned LQ: stable dynamics, SPD costs, two constraint rows per node with D of full row rank"""
    blocks = []
    for k in range(N + 1):
        M = rng.standard_normal((nx, nx))
        o = dict(Q=M @ M.T / nx + np.eye(nx), q=rng.standard_normal(nx))
        if k < N:
            Mr = rng.standard_normal((nu, nu))
            o.update(A=np.eye(nx) + 0.2 * rng.standard_normal((nx, nx)), B=rng.standard_normal((nx, nu)), b=rng.standard_normal(nx), R=Mr @ Mr.T / nu + np.eye(nu),
                     r=rng.standard_normal(nu), C=rng.standard_normal((nc, nx)), D=rng.standard_normal((nc, nu)), e=rng.standard_normal(nc), nc=nc)
        blocks.append(o)
    return blocks


def _mp_kkt(blocks, dx0):
    """the same QP as a dense mpmath system, assembled independently of kkt_reference: variables interleaved per stage [dx_0, du_0, dx_1, ..., dx_N]"""
    N = len(blocks) - 1
    nx, nu = blocks[0]["A"].shape[0], blocks[0]["B"].shape[1]
    ofs_x = [k * (nx + nu) for k in range(N + 1)]
    ofs_u = [k * (nx + nu) + nx for k in range(N)]
    nz = N * (nx + nu) + nx
    rows, rhs = [], []                                                   # equality rows over the nz primal unknowns
    for i in range(nx):
        r = [0.0] * nz; r[ofs_x[0] + i] = 1.0; rows.append(r); rhs.append(dx0[i])
    for k in range(N):
        o = blocks[k]
        for i in range(nx):
            r = [0.0] * nz
            for j in range(nx):
                r[ofs_x[k] + j] = o["A"][i, j]
            for j in range(nu):
                r[ofs_u[k] + j] = o["B"][i, j]
            r[ofs_x[k + 1] + i] = -1.0
            rows.append(r); rhs.append(-o["b"][i])
        for i in range(o["nc"]):
            r = [0.0] * nz
            for j in range(nx):
                r[ofs_x[k] + j] = o["C"][i, j]
            for j in range(nu):
                r[ofs_u[k] + j] = o["D"][i, j]
            rows.append(r); rhs.append(-o["e"][i])
    m = len(rows)
    K = mp.zeros(nz + m, nz + m)
    f = mp.zeros(nz + m, 1)
    for k, o in enumerate(blocks):
        for i in range(nx):
            f[ofs_x[k] + i] = -mp.mpf(o["q"][i])
            for j in range(nx):
                K[ofs_x[k] + i, ofs_x[k] + j] = mp.mpf(o["Q"][i, j])
        if k < N:
            for i in range(nu):
                f[ofs_u[k] + i] = -mp.mpf(o["r"][i])
                for j in range(nu):
                    K[ofs_u[k] + i, ofs_u[k] + j] = mp.mpf(o["R"][i, j])
    for i, r in enumerate(rows):
        f[nz + i] = mp.mpf(rhs[i])
        for j, v in enumerate(r):
            if v != 0.0:
                K[nz + i, j] = K[j, nz + i] = mp.mpf(v)
    return K, f, ofs_x, ofs_u


def test_reference_agrees_with_a_50_digit_solve():
    """(a) On a small random well-conditioned LQ (N = 3, two constraint rows per node, dx0 != 0) the refined step, and the plain fp64 LU step, are within
    10 eps kappa(K) of the 50-digit solution (kappa: the infinity-norm condition number of the KKT matrix, also in 50 digits) -- the first-order error bound
    of a backward-stable fp64 solve, with a factor 10 for the dimension-dependent constant."""
    mp.mp.dps = 50
    rng = np.random.default_rng(5)
    blocks = _random_lq(rng)
    dx0 = rng.standard_normal(4)
    K, f, ofs_x, ofs_u = _mp_kkt(blocks, dx0)
    z = mp.lu_solve(K, f)
    norm = lambda M: max(sum(abs(M[i, j]) for j in range(M.cols)) for i in range(M.rows))   # noqa: E731
    kappa = float(norm(K) * norm(mp.inverse(K)))
    N = len(blocks) - 1
    dX = np.array([[float(z[ofs_x[k] + i]) for i in range(4)] for k in range(N + 1)])
    dU = np.array([[float(z[ofs_u[k] + i]) for i in range(3)] for k in range(N)])
    r = KR.solve(blocks, dx0)
    bound = 10 * KR.EPS * kappa
    errs = dict(dX=KR.rel_err(r["dX"], dX), dU=KR.rel_err(r["dU"], dU), dX_lu=KR.rel_err(r["dX_lu"], dX), dU_lu=KR.rel_err(r["dU_lu"], dU))
    print("kappa", kappa, "bound", bound, errs, "correction", r["correction"], "refinements", r["refinements"])
    assert 1.0 < kappa < 1e6                                             # well-conditioned, as intended
    assert all(e <= bound for e in errs.values()), (errs, bound)
    assert max(r["correction"]) <= bound


# ------------------------------------------------------------------------------------------------ (b) the oracle's step against the reference
@pytest.fixture(scope="module")
def host():
    itf = api.QMInterface()
    ft = KS.force_tracking_interface()
    return itf, S.Oracle(itf.problem), ft, S.Oracle(ft.problem)


@pytest.mark.parametrize("name", list(KS.gpu_scenarios()))
def test_oracle_step_equals_kkt_reference(host, name):
    """(b) The oracle's step (mpc_solve warm = the iterate, no line search) from its own blocks against the reference, on every scenario of the GPU tier (all four
    factorisation unrolls, mixed gaits, defect-laden and cold iterates, the event grid, the barriers' quadratic branches, force tracking, N = 1, 2, 200, 300 and
    the 300-instance batch): the tolerance rule of kkt_scenarios.py with the reference's correction below 1e-2 of it, and the bar of the N = 5 dense check
    (test_oracle_invariants.py::test_riccati_step_equals_dense_kkt_solve: 1e-9 on X, 1e-8 on U relative to max(1, |step|)) on every instance."""
    itf, orc, ft, orc_ft = host
    i_, o_ = (ft, orc_ft) if name == "force_tracking" else (itf, orc)
    sc = KS.build(KS.gpu_scenarios(), name, i_, o_)
    rows = [KS.oracle_errors(sc, o_, i) for i in range(sc.B)]
    tol = KS.tolerance(rows)
    ncs = sorted(set().union(*[{int(b["nc"]) for b in r["blocks"][:-1]} for r in rows]))
    print(name, "nc", ncs, "e_orc", [max(r["e_orc"][j] for r in rows) for j in (0, 1)], "e_lu", [max(r["e_lu"][j] for r in rows) for j in (0, 1)], "tol", tol)
    if sc.nc is not None:
        assert set(ncs) == set(sc.nc), (name, ncs)
    for i, r in enumerate(rows):
        dX, dU = r["step"]["X"] - sc.X[i], r["step"]["U"] - sc.U[i]
        for j, (got, ref) in enumerate(((dX, r["ref"]["dX"]), (dU, r["ref"]["dU"]))):
            assert r["ref"]["correction"][j] <= 1e-2 * tol[j], (name, i, j, r["ref"]["correction"], tol)
            assert KR.rel_err(got, ref) <= tol[j], (name, i, j)
        assert np.abs(dX - r["ref"]["dX"]).max() <= 1e-9 * max(1.0, np.abs(r["ref"]["dX"]).max()), (name, i)
        assert np.abs(dU - r["ref"]["dU"]).max() <= 1e-8 * max(1.0, np.abs(r["ref"]["dU"]).max()), (name, i)


# ------------------------------------------------------------------------------------------------ (c) the host-emulated kernels against the reference
@pytest.fixture(scope="module")
def emu():
    lib = abi.load_library(S.build_emu())
    itf = api.QMInterface(lib=lib)
    return itf, S.Oracle(itf.problem)


def emu_solve(itf, sc, debug):
    """one solve of scenario sc through the host-emulated library (numpy arrays as device memory); returns the solver (for its dump) and the outputs"""
    B, N = sc.B, sc.N
    sol = api.GpuSolver(itf, max_batch=B, max_nodes=N)
    sol.enable_debug(debug)
    oT, oX, oU, oM, oS = np.zeros((B, N + 1)), np.zeros((B, N + 1, 30)), np.zeros((B, N, 30)), np.zeros((B, N + 1), dtype=np.int32), np.zeros((B, abi.NSTATS))
    a = sol.mpc_args(B, N, sc.x0, sc.tt, sc.ts, sc.nev, sc.ev, sc.md, oT, oX, oU, oM, oS, t0=np.zeros(B) if sc.uniform else None,
                     time_grid=None if sc.uniform else sc.grid, warm_x=sc.X if sc.warm else None, warm_u=sc.U if sc.warm else None, line_search=sc.line_search,
                     ee_contact_ref=sc.contact)
    sol.mpc(a)
    return sol, dict(T=oT, X=oX, U=oU, mode=oM, stats=oS)


@pytest.mark.parametrize("name", list(KS.emu_scenarios()))
def test_emu_step_equals_kkt_reference(emu, name):
    """(c) The kernel sources on host threads: the LQ blocks of every node against the oracle, the step against the reference from the kernels' own blocks under
    the tolerance rule, and the same solve with the dump off bit-identical (the checked path is the product path)."""
    itf, orc = emu
    sc = KS.build(KS.emu_scenarios(), name, itf, orc)
    _, off = emu_solve(itf, sc, False)
    sol, on = emu_solve(itf, sc, True)
    for key in ("T", "X", "U", "mode", "stats"):
        assert np.array_equal(on[key], off[key]), (name, key)
    KS.check_product(sc, orc, on, sol.debug_lq)
