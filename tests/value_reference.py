"""Reference for the SQP value function (qmgpu_mpc_value_function_batch / qmgpu_value_function_eval_batch), independent of the projected Riccati recursion.

V_k(dx) is the optimal cost of the QP over nodes k .. N (kkt_reference.py) as a function of its initial state dx_k = dx.  The KKT system of that tail is assembled
once (kkt_reference.assemble), factorised once by SuperLU and solved for 31 right-hand sides, each refined with the residual in np.longdouble as
feedback_reference.reference_gain refines its thirty:
    z0   the system's own right-hand side with dx0 = 0 and every affine term,
    Z    the 30 unit columns of the `dx_0 = dx0` rows with every affine term zero,
so the primal solution is z(dx) = z0 + Z dx and, with H the Hessian block and g the gradient of the objective,
    Sm_ref = sym(Z' H Z),      sv_ref = Z' (H z0 + g)          (products block by block in np.longdouble).
Second route from the same solves: with the system [[H, E'], [E, 0]] [z; lam] = [-g; f] the sensitivity of the optimal cost to the right-hand side f is -lam, so the
multipliers of the dx_0 rows give sv = -lam(z0) and Sm = -lam(Z).  reference_value asserts that the two routes agree within the LU error of the same solves.

Tolerance rule, the shape of kkt_scenarios.py (measured against the reference, never against the code under test), separately for Sm and sv_lin.  Per scenario
    e_lu = error of the plain LU values against the refined ones,
    e_np = error of numpy_value (a plain fp64 restatement of the projected recursion, used ONLY here) against them,
both maxima over the checked nodes in kkt_reference.rel_err;  tol = kkt_scenarios.FACTOR * max(e_lu, e_np);  the refinement's last correction must stay below
1e-2 tol.  Test helper, no GPU.
"""
import json
import os

import numpy as np
import scipy.sparse.linalg as spla

import kkt_reference as KR
import kkt_scenarios as KS

EPS = np.finfo(np.float64).eps
LD = np.longdouble


def _sym(M):
    return 0.5 * (M + M.T)


def _quadratic_terms(tail, z, layout):
    """(Z' H Z, Z' (H z0 + g)) for z = [z0 | Z] (longdouble, primal rows only), block by block: H = blockdiag(sym Q_k, sym R_k), g = [q_k; r_k]"""
    Nt, nx, nu = layout
    Sm, sv = np.zeros((nx, nx), dtype=LD), np.zeros(nx, dtype=LD)
    for k, o in enumerate(tail):
        parts = [(slice(nx * k, nx * (k + 1)), o["Q"], o["q"])]
        if k < Nt:
            u0 = nx * (Nt + 1) + nu * k
            parts.append((slice(u0, u0 + nu), o["R"], o["r"]))
        for rows, W, w in parts:
            Wl, z0, Z = _sym(np.asarray(W, dtype=np.float64)).astype(LD), z[rows, 0], z[rows, 1:]
            Sm += Z.T @ (Wl @ Z)
            sv += Z.T @ (Wl @ z0 + np.asarray(w, dtype=np.float64).astype(LD))
    return Sm, sv


def reference_value(tail):
    """Sm, sv of the first node of `tail` (blocks k .. N; the terminal node alone is a tail).  dict(Sm, sv: refined; Sm_lu, sv_lu: from the plain LU solution;
    Sm_mult, sv_mult: the multiplier route; route_gap: (Sm, sv) difference of the two routes in rel_err; correction: (Sm, sv) change the last refinement correction
    makes, in rel_err; refinements)."""
    Nt = len(tail) - 1
    nx = tail[Nt]["Q"].shape[0]
    Kmat, rhs0, layout = KR.assemble(tail, np.zeros(nx))
    nu = layout[2]
    nz = nx * (Nt + 1) + nu * Nt
    n = Kmat.shape[0]
    rhs = np.zeros((n, nx + 1))
    rhs[:, 0] = rhs0
    rhs[nz + np.arange(nx), 1 + np.arange(nx)] = 1.0
    lu = spla.splu(Kmat, permc_spec="COLAMD", diag_pivot_thresh=1.0)
    z = lu.solve(rhs)
    z_lu = z.copy()
    Kr = Kmat.tocsr()
    assert (np.diff(Kr.indptr) > 0).all()
    data, starts = Kr.data.astype(LD)[:, None], Kr.indptr[:-1]
    rhs_l, zl = rhs.astype(LD), z.astype(LD)
    prev, last, count = np.inf, np.zeros_like(z), 0
    for _ in range(KR.MAX_REFINEMENTS):
        res = rhs_l.copy()
        for c in range(0, nx + 1, 5):                                      # five columns at a time, as feedback_reference.reference_gain
            res[:, c:c + 5] -= np.add.reduceat(data * zl[Kr.indices, c:c + 5], starts, axis=0)
        d = lu.solve(res.astype(np.float64))
        size = float(np.abs(d).max())
        zl += d
        count, last = count + 1, d
        if size == 0.0 or size >= prev:
            break
        prev = size
    f64 = lambda pair: (_sym(pair[0].astype(np.float64)), pair[1].astype(np.float64))  # noqa: E731
    Sm, sv = f64(_quadratic_terms(tail, zl[:nz], layout))
    Sm_lu, sv_lu = f64(_quadratic_terms(tail, z_lu[:nz].astype(LD), layout))
    Sm_c, sv_c = f64(_quadratic_terms(tail, zl[:nz] + last[:nz].astype(LD), layout))
    lam = zl[nz:nz + nx].astype(np.float64)                                # multipliers of the dx_0 rows (the first equality rows)
    Sm_mult, sv_mult = _sym(-lam[:, 1:]), -lam[:, 0]
    e_lu = (KR.rel_err(Sm_lu, Sm), KR.rel_err(sv_lu, sv))
    gap = (KR.rel_err(Sm_mult, Sm), KR.rel_err(sv_mult, sv))
    # both routes come from the same refined solves; what separates them is bounded by the error the plain LU solution of those solves shows (floor: the 64 eps of
    # the products' own rounding where the LU error happens to vanish)
    for j in (0, 1):
        assert gap[j] <= KS.FACTOR * max(e_lu[j], 64 * EPS), ("value-function routes disagree", Nt, gap, e_lu)
    return dict(Sm=Sm, sv=sv, Sm_lu=Sm_lu, sv_lu=sv_lu, Sm_mult=Sm_mult, sv_mult=sv_mult, route_gap=gap, e_lu=e_lu,
                correction=(KR.rel_err(Sm_c, Sm), KR.rel_err(sv_c, sv)), refinements=count)


def numpy_value(blocks):
    """([Sm_0 .. Sm_N], [sv_0 .. sv_N]) by the projected recursion in plain numpy fp64: QR projection of D (du = Pe + Px dx + Pu du~), backward Riccati on the
    projected stages with the affine terms.  Used only to size the tolerance (a second backward-stable fp64 route to the same values)."""
    N = len(blocks) - 1
    S, s = _sym(blocks[N]["Q"]), np.array(blocks[N]["q"], dtype=np.float64)
    Sm, sv = [None] * (N + 1), [None] * (N + 1)
    Sm[N], sv[N] = S, s
    for k in range(N - 1, -1, -1):
        o = blocks[k]
        nc = int(o["nc"])
        A, B, b, Q, R, q, r = o["A"], o["B"], o["b"], _sym(o["Q"]), _sym(o["R"]), o["q"], o["r"]
        nu = B.shape[1]
        if nc:
            Qf, Rf = np.linalg.qr(o["D"][:nc].T, mode="complete")          # D' = Q1 R1:  D du = -C dx - e  <=>  du = -Q1 R1^-T (C dx + e) + Q2 du~
            Q1, Pu, R1 = Qf[:, :nc], Qf[:, nc:], Rf[:nc]
            Px = -Q1 @ np.linalg.solve(R1.T, o["C"][:nc])
            Pe = -Q1 @ np.linalg.solve(R1.T, o["e"][:nc])
        else:
            Pu, Px, Pe = np.eye(nu), np.zeros((nu, A.shape[1])), np.zeros(nu)
        At, Bt, bt = A + B @ Px, B @ Pu, b + B @ Pe
        rr = r + R @ Pe
        Qt, Pt, Rt, qt, rt = Q + Px.T @ R @ Px, Pu.T @ R @ Px, Pu.T @ R @ Pu, q + Px.T @ rr, Pu.T @ rr
        y = S @ bt + s
        H, G, g = Rt + Bt.T @ S @ Bt, Pt + Bt.T @ S @ At, rt + Bt.T @ y
        Kt, kt = -np.linalg.solve(H, G), -np.linalg.solve(H, g)
        s = qt + At.T @ y + G.T @ kt
        S = _sym(Qt + At.T @ S @ At + G.T @ Kt)
        Sm[k], sv[k] = S, s
    return Sm, sv


def fixed_point_bound(Sm, x, sl):
    """64 eps (|sv_lin| + |Sm||x|) row by row: two 31-term accumulations (the kernel's and numpy's), each below 31 eps times that sum"""
    return 64 * EPS * (np.abs(sl) + np.abs(Sm) @ np.abs(x))


def check_structure(name, sc, Sm, Sv, sv_lin, x_lin, product_lq, tol_Sm):
    """The checks that need no reference, on EVERY node of every instance (Sm, Sv, sv_lin, x_lin [B][N+1][..] started as NaN: every entry must have been written)."""
    B, N = sc.B, sc.N
    for arr in (Sm, Sv, sv_lin, x_lin):
        assert np.isfinite(arr).all(), name
    assert np.array_equal(Sm, np.swapaxes(Sm, 2, 3)), name
    assert np.array_equal(x_lin, sc.X), name
    worst_fp, worst_eig = 0.0, 0.0
    for i in range(B):
        term = product_lq(i, N)
        assert np.abs(Sm[i, N] - _sym(term["Q"])).max() <= 2 * EPS * np.abs(term["Q"]).max(), (name, i)
        assert np.abs(sv_lin[i, N] - term["q"]).max() <= 2 * EPS * max(np.abs(term["q"]).max(), np.finfo(np.float64).tiny), (name, i)
        for k in range(N + 1):
            gap, bound = np.abs(Sv[i, k] + Sm[i, k] @ x_lin[i, k] - sv_lin[i, k]), fixed_point_bound(Sm[i, k], x_lin[i, k], sv_lin[i, k])
            worst_fp = max(worst_fp, float((gap / np.where(bound > 0, bound, 1.0)).max()))
            assert (gap <= bound).all(), (name, i, k, gap.max())
            low, norm = float(np.linalg.eigvalsh(Sm[i, k])[0]), float(np.abs(Sm[i, k]).sum(axis=1).max())
            worst_eig = min(worst_eig, low / norm if norm > 0 else 0.0)
            assert low >= -tol_Sm * norm, (name, i, k, low, norm, tol_Sm)
    print(name, "structure: worst |Sv + Sm x - sv_lin| / bound", worst_fp, " smallest eigenvalue / |Sm|_inf", worst_eig, " allowed", -tol_Sm)


def check_value(sc, Sm, Sv, sv_lin, x_lin, product_lq, instances=None, nodes=None, record_path=None):
    """Sm, sv_lin of scenario sc against the reference built from the product's OWN LQ blocks (product_lq(i, k)) on `nodes` (default: all N + 1) of `instances`
    (default: all), under the tolerance rule of this module, then the structural checks on everything.  Every figure is printed (and recorded under record_path)
    before anything is asserted."""
    B, N = sc.B, sc.N
    instances = list(range(B)) if instances is None else list(instances)
    nodes = list(range(N + 1)) if nodes is None else list(nodes)
    rows = []
    for i in instances:
        blocks = [product_lq(i, k) for k in range(N + 1)]
        Snp, snp = numpy_value(blocks)
        for k in nodes:
            r = reference_value(blocks[k:])
            rows.append(dict(i=i, k=k, e_lu=r["e_lu"], e_np=(KR.rel_err(Snp[k], r["Sm"]), KR.rel_err(snp[k], r["sv"])),
                             err=(KR.rel_err(Sm[i, k], r["Sm"]), KR.rel_err(sv_lin[i, k], r["sv"])), correction=r["correction"], route_gap=r["route_gap"],
                             scale=(float(np.abs(r["Sm"]).max()), float(np.abs(r["sv"]).max()))))
    mx = lambda key: [max(r[key][j] for r in rows) for j in (0, 1)]  # noqa: E731
    e_lu, e_np = mx("e_lu"), mx("e_np")
    tol = [KS.FACTOR * max(e_lu[j], e_np[j]) for j in (0, 1)]
    worst = [max(rows, key=lambda r: r["err"][j]) for j in (0, 1)]
    rec = dict(instances=len(instances), N=N, nodes_checked=len(rows), e_lu=e_lu, e_np=e_np, product=[worst[j]["err"][j] for j in (0, 1)],
               product_at=[[worst[j]["i"], worst[j]["k"]] for j in (0, 1)], tolerance=tol, correction=mx("correction"), route_gap=mx("route_gap"),
               scale_Sm=[min(r["scale"][0] for r in rows), max(r["scale"][0] for r in rows)], scale_sv=[min(r["scale"][1] for r in rows), max(r["scale"][1] for r in rows)])
    print(sc.name, json.dumps(rec))
    if record_path:
        os.makedirs(os.path.dirname(os.path.abspath(record_path)), exist_ok=True)
        try:
            allrec = json.load(open(record_path))
        except (OSError, ValueError):
            allrec = {}
        allrec[sc.name] = rec
        json.dump(allrec, open(record_path, "w"), indent=1)
    for r in rows:
        for j, part in enumerate(("Sm", "sv_lin")):
            assert r["correction"][j] <= 1e-2 * tol[j], (sc.name, part, r, tol)
            assert r["err"][j] <= tol[j], (sc.name, part, r, tol)
    check_structure(sc.name, sc, Sm, Sv, sv_lin, x_lin, product_lq, tol[0])
    return rec


def eval_reference(T, Sm, Sv, t, x):
    """Plain numpy statement of qmgpu_value_function_eval_batch: (dfdx [B][30], dfdxx [B][30][30], bound [B][30]) at the times t [B] for the states x [B][30];
    interval and weight as feedback_reference.policy_reference (LinearInterpolation, end values held), bound = 64 eps (|Sv(t)| + |Sm(t)||x|) row by row."""
    B, N = T.shape[0], T.shape[1] - 1
    rows = np.arange(B)
    interval = (T < t[:, None]).sum(axis=1) - 1
    idx = np.clip(interval, 0, N - 1)
    t0, t1 = T[rows, idx], T[rows, idx + 1]
    length = t1 - t0
    alpha = np.where(length > 2 * EPS, (t1 - t) / np.where(length == 0, 1.0, length), 1.0)
    alpha = np.where(interval < 0, 1.0, np.where(interval >= N, 0.0, alpha))
    a1, a2 = alpha[:, None], alpha[:, None, None]
    vt = a1 * Sv[rows, idx] + (1 - a1) * Sv[rows, idx + 1]
    St = a2 * Sm[rows, idx] + (1 - a2) * Sm[rows, idx + 1]
    return vt + np.einsum("bij,bj->bi", St, x), St, 64 * EPS * (np.abs(vt) + np.einsum("bij,bj->bi", np.abs(St), np.abs(x)))
