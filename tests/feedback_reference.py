"""Reference for the SQP feedback policy (qmgpu_mpc_feedback_batch / qmgpu_policy_eval_feedback_batch), independent of the projected Riccati recursion.

The gain K_k of node k is the sensitivity of the first input of the QP over nodes k .. N (kkt_reference.py) to its initial state.  With every affine term zero the
KKT system is linear in dx0, so the solution for the right-hand side that is zero except for a unit entry in row j of the `dx_0 = dx0` equalities (rows nz + j)
has column j of K_k as its du_0.  Per tail the matrix is assembled once (kkt_reference.assemble), factorised once by SuperLU and all 30 right-hand sides are refined
with the residual in np.longdouble, as kkt_reference.solve refines its one.

Tolerance rule, the shape of kkt_scenarios.py (measured against the reference, never against the code under test).  Per scenario
    e_lu = error of the plain LU gains against the refined ones,
    e_np = error of numpy_gains (a plain fp64 restatement of the projected recursion, used ONLY here) against them,
both max over the checked nodes of |dK_k|_inf / |K_ref,k|_inf (entrywise maxima, kkt_reference.rel_err);  tol = kkt_scenarios.FACTOR * max(e_lu, e_np);  the
refinement's last correction must stay below 1e-2 tol.  Test helper, no GPU.
"""
import json
import os

import numpy as np
import scipy.sparse.linalg as spla

import kkt_reference as KR
import kkt_scenarios as KS
from support import contact_flags

EPS = np.finfo(np.float64).eps


def reference_gain(tail):
    """K of the first node of `tail` (blocks k .. N, at least one stage).  dict(K: refined, K_lu: plain LU, correction: the last refinement correction in the
    measure of rel_err, refinements)."""
    Nt = len(tail) - 1
    nx = tail[Nt]["Q"].shape[0]
    Kmat, _, (_, _, nu) = KR.assemble(tail, np.zeros(nx))
    nz = nx * (Nt + 1) + nu * Nt
    n = Kmat.shape[0]
    rhs = np.zeros((n, nx))
    rhs[nz + np.arange(nx), np.arange(nx)] = 1.0
    lu = spla.splu(Kmat, permc_spec="COLAMD", diag_pivot_thresh=1.0)
    z = lu.solve(rhs)
    z_lu = z.copy()
    Kr = Kmat.tocsr()
    assert (np.diff(Kr.indptr) > 0).all()
    data, starts = Kr.data.astype(np.longdouble)[:, None], Kr.indptr[:-1]
    rhs_l, zl = rhs.astype(np.longdouble), z.astype(np.longdouble)
    prev, last, count = np.inf, np.zeros_like(z), 0
    for _ in range(KR.MAX_REFINEMENTS):
        res = rhs_l.copy()
        for c in range(0, nx, 5):                                          # five columns at a time: the products of a long horizon are large in extended precision
            res[:, c:c + 5] -= np.add.reduceat(data * zl[Kr.indices, c:c + 5], starts, axis=0)
        d = lu.solve(res.astype(np.float64))
        size = float(np.abs(d).max())
        zl += d
        count, last = count + 1, d
        if size == 0.0 or size >= prev:
            break
        prev = size
    u0 = slice(nx * (Nt + 1), nx * (Nt + 1) + nu)
    K = zl.astype(np.float64)[u0]
    return dict(K=K, K_lu=z_lu[u0], correction=KR.rel_err(K + last[u0], K), refinements=count)


def numpy_gains(blocks):
    """[K_0 .. K_{N-1}] by the projected recursion in plain numpy fp64: QR projection of D, backward Riccati on the projected stages, K = Px + Pu K~.
    Used only to size the tolerance (a second backward-stable fp64 route to the same gains)."""
    N = len(blocks) - 1
    S = 0.5 * (blocks[N]["Q"] + blocks[N]["Q"].T)
    out = [None] * N
    for k in range(N - 1, -1, -1):
        o = blocks[k]
        nc = int(o["nc"])
        A, B, Q, R = o["A"], o["B"], 0.5 * (o["Q"] + o["Q"].T), 0.5 * (o["R"] + o["R"].T)
        nu = B.shape[1]
        if nc:
            Qf, Rf = np.linalg.qr(o["D"][:nc].T, mode="complete")          # D' = Q1 R1:  D du = -C dx  <=>  du = -Q1 R1^-T C dx + Q2 du~
            Q1, Pu, R1 = Qf[:, :nc], Qf[:, nc:], Rf[:nc]
            Px = -Q1 @ np.linalg.solve(R1.T, o["C"][:nc])
        else:
            Pu, Px = np.eye(nu), np.zeros((nu, A.shape[1]))
        At, Bt = A + B @ Px, B @ Pu
        Qt, Pt, Rt = Q + Px.T @ R @ Px, Pu.T @ R @ Px, Pu.T @ R @ Pu
        H, G = Rt + Bt.T @ S @ Bt, Pt + Bt.T @ S @ At
        Kt = -np.linalg.solve(H, G)
        S = Qt + At.T @ S @ At + G.T @ Kt
        S = 0.5 * (S + S.T)
        out[k] = Px + Pu @ Kt
    return out


def checked_nodes(N, modes):
    """The nodes of an instance whose gains are compared with the reference: all of them, except on the long horizons (N >= 200, where a tail's KKT system has
    tens of thousands of unknowns): there the first and the last three, every node whose contact mode differs from a neighbour's together with that neighbour,
    and every 25th node."""
    if N < 200:
        return list(range(N))
    keep = {0, 1, 2, N - 3, N - 2, N - 1} | set(range(0, N, 25))
    for k in range(N - 1):
        if modes[k] != modes[k + 1]:
            keep |= {k, k + 1}
    return sorted(k for k in keep if 0 <= k < N)


def fixed_point_bound(K, x, u):
    """64 eps (|u| + |K||x|) row by row: two 31-term accumulations (the kernel's and numpy's), each below 31 eps times that sum"""
    return 64 * EPS * (np.abs(u) + np.abs(K) @ np.abs(x))


def check_structure(name, out, K, uff):
    """The checks that need no reference, on EVERY node of every instance: uff_k + K_k X_k = U_k, the last entry a copy, zero force rows of a swing foot."""
    B, N = out["U"].shape[0], out["U"].shape[1]
    assert np.isfinite(K).all() and np.isfinite(uff).all(), name
    worst = 0.0
    for i in range(B):
        assert np.array_equal(K[i, N], K[i, N - 1]) and np.array_equal(uff[i, N], uff[i, N - 1]), (name, i)
        for k in range(N):
            X, U = out["X"][i, k], out["U"][i, k]
            gap, bound = np.abs(uff[i, k] + K[i, k] @ X - U), fixed_point_bound(K[i, k], X, U)
            worst = max(worst, float((gap / np.where(bound > 0, bound, 1.0)).max()))
            assert (gap <= bound).all(), (name, i, k, gap.max())
            mode = int(out["mode"][i, k])
            for leg in range(4):
                if not contact_flags(mode)[leg]:
                    assert not K[i, k, 3 * leg:3 * leg + 3].any(), (name, i, k, leg)
    print(name, "fixed point: worst |uff + K X - U| / bound", worst)


def check_gains(sc, out, K, product_lq, record_path=None):
    """K [B][N+1][30][30] of scenario sc against the reference built from the product's OWN LQ blocks (product_lq(i, k)) on checked_nodes, under the tolerance rule
    of this module.  Every figure is printed (and recorded under record_path) before anything is asserted."""
    B, N = sc.B, sc.N
    rows = []
    for i in range(B):
        blocks = [product_lq(i, k) for k in range(N + 1)]
        Knp = numpy_gains(blocks)
        for k in checked_nodes(N, out["mode"][i]):
            r = reference_gain(blocks[k:])
            rows.append(dict(i=i, k=k, e_lu=KR.rel_err(r["K_lu"], r["K"]), e_np=KR.rel_err(Knp[k], r["K"]), err=KR.rel_err(K[i, k], r["K"]), correction=r["correction"],
                             scale=float(np.abs(r["K"]).max())))
    e_lu, e_np = max(r["e_lu"] for r in rows), max(r["e_np"] for r in rows)
    tol = KS.FACTOR * max(e_lu, e_np)
    worst = max(rows, key=lambda r: r["err"])
    rec = dict(instances=B, N=N, nodes_checked=len(rows), e_lu=e_lu, e_np=e_np, product=worst["err"], product_at=[worst["i"], worst["k"]], tolerance=tol,
               correction=max(r["correction"] for r in rows), gain_scale=[min(r["scale"] for r in rows), max(r["scale"] for r in rows)])
    print(sc.name, json.dumps(rec))
    if record_path:
        os.makedirs(os.path.dirname(os.path.abspath(record_path)), exist_ok=True)
        try:
            allrec = json.load(open(record_path))
        except (OSError, ValueError):
            allrec = {}
        allrec[sc.name] = rec
        json.dump(allrec, open(record_path, "w"), indent=1)
    assert (out["stats"][:, 7] == 0).all(), sc.name
    for r in rows:
        assert r["correction"] <= 1e-2 * tol, (sc.name, r, tol)
        assert r["err"] <= tol, (sc.name, r, tol)
    return rec


def policy_reference(T, X, uff, K, t, xm):
    """Plain numpy statement of qmgpu_policy_eval_feedback_batch: (u [B][30], bound [B][30]) at the times t [B] for the measured states xm [B][30];
    interval and weight as harness.interp_plan (LinearInterpolation, end values held), bound = 64 eps (|uff(t)| + |K(t)||xm|) row by row."""
    B, N = X.shape[0], X.shape[1] - 1
    rows = np.arange(B)
    interval = (T < t[:, None]).sum(axis=1) - 1
    idx = np.clip(interval, 0, N - 1)
    t0, t1 = T[rows, idx], T[rows, idx + 1]
    length = t1 - t0
    alpha = np.where(length > 2 * EPS, (t1 - t) / np.where(length == 0, 1.0, length), 1.0)
    alpha = np.where(interval < 0, 1.0, np.where(interval >= N, 0.0, alpha))
    a1, a2 = alpha[:, None], alpha[:, None, None]
    ft = a1 * uff[rows, idx] + (1 - a1) * uff[rows, idx + 1]
    Kt = a2 * K[rows, idx] + (1 - a2) * K[rows, idx + 1]
    u = ft + np.einsum("bij,bj->bi", Kt, xm)
    return u, 64 * EPS * (np.abs(ft) + np.einsum("bij,bj->bi", np.abs(Kt), np.abs(xm)))


def policy_cases(T, rng):
    """evaluation times [4][B]: on a node, inside an interval, before t_0 and beyond t_N"""
    B, N = T.shape[0], T.shape[1] - 1
    rows = np.arange(B)
    k = rng.integers(1, N + 1, B) if N > 1 else np.ones(B, dtype=int)
    j = rng.integers(0, N, B)
    return [T[rows, k].copy(), T[rows, j] + rng.uniform(0.1, 0.9, B) * (T[rows, j + 1] - T[rows, j]), T[:, 0] - 0.01, T[:, N] + 0.02]
