"""CPU tier: the yardstick of the value-function checks (value_reference.py) before any kernel is involved: on the oracle's LQ blocks of
kkt_scenarios.emu_scenarios() the two routes of the reference agree and numpy_value is within the tolerance rule; a hand case with a closed form."""
import numpy as np
import pytest

import kkt_reference as KR
import kkt_scenarios as KS
import support as S
import value_reference as VR
from qm_door_amd import api


@pytest.fixture(scope="module")
def host():
    itf = api.QMInterface()
    return itf, S.Oracle(itf.problem)


@pytest.mark.parametrize("name", list(KS.emu_scenarios()))
def test_reference_routes_agree_and_numpy_value_is_within_the_rule(host, name):
    """Z' H Z and Z' (H z0 + g) against the multipliers of the dx_0 rows (asserted inside reference_value, printed here), on three nodes and the terminal one; the
    plain fp64 projected recursion against them within FACTOR * max(e_lu, e_np) -- which it satisfies by construction unless FACTOR < 1 -- and, the real content,
    both errors far below the size at which a wrong term shows (1e-6: a missing affine term or projection is O(1))."""
    itf, orc = host
    sc = KS.build(KS.emu_scenarios(), name, itf, orc)
    grid, nev, ev, md, tt, ts = sc.instance(0)
    blocks = KR.oracle_blocks(orc, grid, sc.X[0], sc.U[0], nev, ev, md, tt, ts)
    Snp, snp = VR.numpy_value(blocks)
    nodes = sorted({0, sc.N // 2, sc.N - 1, sc.N})
    refs = {k: VR.reference_value(blocks[k:]) for k in nodes}
    e_lu = [max(r["e_lu"][j] for r in refs.values()) for j in (0, 1)]
    e_np = [max(KR.rel_err((Snp, snp)[j][k], (r["Sm"], r["sv"])[j]) for k, r in refs.items()) for j in (0, 1)]
    tol = [KS.FACTOR * max(e_lu[j], e_np[j]) for j in (0, 1)]
    print(name, "e_lu", e_lu, "e_np", e_np, "tol", tol, "route gap", [r["route_gap"] for r in refs.values()], "correction", [r["correction"] for r in refs.values()])
    for k, r in refs.items():
        for j in (0, 1):
            assert r["correction"][j] <= 1e-2 * tol[j], (name, k, j)
            assert KR.rel_err((Snp, snp)[j][k], (r["Sm"], r["sv"])[j]) <= tol[j] <= 1e-6, (name, k, j, tol)
        assert np.array_equal(r["Sm"], r["Sm"].T) and np.linalg.eigvalsh(r["Sm"])[0] >= -tol[0] * np.abs(r["Sm"]).sum(axis=1).max(), (name, k)
    term = refs[sc.N]
    assert np.abs(term["Sm"] - 0.5 * (blocks[sc.N]["Q"] + blocks[sc.N]["Q"].T)).max() <= 4 * VR.EPS * np.abs(blocks[sc.N]["Q"]).max()
    assert np.abs(term["sv"] - blocks[sc.N]["q"]).max() <= 4 * VR.EPS * np.abs(blocks[sc.N]["q"]).max()


def test_one_stage_without_constraints_has_a_closed_form():
    """N = 1, no equality rows: S_0 = Q + A' S1 A - G' H^-1 G and s_0 = q + A' y - G' H^-1 g with H = R + B' S1 B, G = B' S1 A, y = S1 b + q1, g = r + B' y, stated
    here on a 3-state, 2-input problem in np.longdouble.  Bound: 1e-12 relative -- the condition numbers of this H and of the KKT matrix are below 1e3, so fp64
    solves carry about 1e3 eps = 2e-13."""
    rng = np.random.default_rng(5)
    nx, nu = 3, 2
    A, B, b = rng.standard_normal((nx, nx)), rng.standard_normal((nx, nu)), rng.standard_normal(nx)
    L, M, T = rng.standard_normal((nx, nx)), rng.standard_normal((nu, nu)), rng.standard_normal((nx, nx))
    Q, R, Q1 = L @ L.T + np.eye(nx), M @ M.T + np.eye(nu), T @ T.T + np.eye(nx)
    q, r, q1 = rng.standard_normal(nx), rng.standard_normal(nu), rng.standard_normal(nx)
    blocks = [dict(A=A, B=B, b=b, Q=Q, R=R, q=q, r=r, C=np.zeros((0, nx)), D=np.zeros((0, nu)), e=np.zeros(0), nc=0), dict(Q=Q1, q=q1)]
    ld = lambda a: np.asarray(a, dtype=np.longdouble)  # noqa: E731
    Al, Bl, S1 = ld(A), ld(B), ld(0.5 * (Q1 + Q1.T))
    H, G = ld(0.5 * (R + R.T)) + Bl.T @ S1 @ Bl, Bl.T @ S1 @ Al
    y = S1 @ ld(b) + ld(q1)
    g = ld(r) + Bl.T @ y
    Hi = np.linalg.inv(H.astype(np.float64)).astype(np.longdouble)
    Hi = Hi @ (2 * np.eye(nu) - H @ Hi)                                   # one Newton step in extended precision
    S0 = ld(0.5 * (Q + Q.T)) + Al.T @ S1 @ Al - G.T @ Hi @ G
    s0 = ld(q) + Al.T @ y - G.T @ Hi @ g
    ref = VR.reference_value(blocks)
    Snp, snp = VR.numpy_value(blocks)
    for got_S, got_s in ((ref["Sm"], ref["sv"]), (ref["Sm_mult"], ref["sv_mult"]), (Snp[0], snp[0])):
        assert KR.rel_err(got_S, S0.astype(np.float64)) <= 1e-12 and KR.rel_err(got_s, s0.astype(np.float64)) <= 1e-12
    assert np.array_equal(Snp[1], 0.5 * (Q1 + Q1.T)) and np.array_equal(snp[1], q1)
