"""Reference for the SQP dual solution (qmgpu_mpc_dual_batch), independent of the Riccati recursion, the oracle and the kernels.

The KKT system of the QP stated in kkt_reference.py, [[H, E'], [E, 0]] [z; mu] = [-g; f], carries the multipliers mu of the equality rows in the order assemble()
appends them: the dx_0 row, then per node k < N the dynamics row A_k dx_k + B_k du_k - dx_{k+1} = -b_k and the nc_k constraint rows.  Stationarity, H z + g + E' mu = 0,
read block by block is
    lambda_N = Q_N dx_N + q_N,     lambda_k = Q_k dx_k + q_k + A_k' lambda_{k+1} + C_k' nu_k,     0 = R_k du_k + r_k + B_k' lambda_{k+1} + D_k' nu_k
with lambda_{k+1} = mu(dynamics row k), nu_k = mu(constraint rows k) and lambda_0 = -mu(dx_0 row).  The system is factorised once by SuperLU and refined with the
residual in np.longdouble exactly as kkt_reference.solve refines the step.

Tolerance rule (measured against the reference, never against the code under test), separately for the costates and for nu, per scenario:
    e_lu  = max over the checked instances of the plain fp64 LU multipliers' error against the refined ones (kkt_reference.rel_err over the instance),
    floor = rounding_floor() below: what ONE fp64 evaluation of the defining identity costs, in the same measure,
    tol   = max(kkt_scenarios.FACTOR * e_lu, floor);
the refinement's last correction must stay below 1e-2 tol.  Test helper, no GPU.
"""
import json
import os

import numpy as np
import scipy.sparse.linalg as spla

import kkt_reference as KR
import kkt_scenarios as KS

EPS = np.finfo(np.float64).eps
LD = np.longdouble
NCMAX = 16


def _sym(M):
    return 0.5 * (np.asarray(M, dtype=np.float64) + np.asarray(M, dtype=np.float64).T)


def _split_dual(mu, blocks, layout):
    """(lambda [N+1][nx], [nu_k for k < N]) from the multiplier part of a KKT solution"""
    N, nx, _ = layout
    lam = np.zeros((N + 1, nx))
    lam[0] = -mu[:nx]
    nu, at = [], nx
    for k in range(N):
        lam[k + 1] = mu[at:at + nx]
        at += nx
        nc = int(blocks[k]["nc"])
        nu.append(np.array(mu[at:at + nc]))
        at += nc
    assert at == len(mu)
    return lam, nu


def _flat(nu):
    return np.concatenate(nu) if len(nu) and sum(len(v) for v in nu) else np.zeros(0)


def solve(blocks, dx0=None):
    """The primal and dual solution of the QP of `blocks`.  dict(dX, dU, lam [N+1][nx], nu [N] arrays of nc_k: refined; lam_lu, nu_lu: the plain fp64 LU values;
    e_lu = (lam, nu): their error against the refined ones; correction = (lam, nu): the last refinement correction, both in kkt_reference.rel_err; refinements)."""
    N = len(blocks) - 1
    nx = blocks[N]["Q"].shape[0]
    K, rhs, layout = KR.assemble(blocks, np.zeros(nx) if dx0 is None else dx0)
    nz = nx * (N + 1) + layout[2] * N
    lu = spla.splu(K, permc_spec="COLAMD", diag_pivot_thresh=1.0)
    z = lu.solve(rhs)
    z_lu = z.copy()
    Kr = K.tocsr()
    assert (np.diff(Kr.indptr) > 0).all()
    data, starts = Kr.data.astype(LD), Kr.indptr[:-1]
    rhs_l, zl = rhs.astype(LD), z.astype(LD)
    prev, last, count = np.inf, np.zeros_like(z), 0
    for _ in range(KR.MAX_REFINEMENTS):
        res = rhs_l - np.add.reduceat(data * zl[Kr.indices], starts)
        d = lu.solve(res.astype(np.float64))
        size = float(np.abs(d).max())
        zl += d
        count, last = count + 1, d
        if size == 0.0 or size >= prev:
            break
        prev = size
    zf = zl.astype(np.float64)
    dX, dU = KR._split(zf, layout)
    lam, nu = _split_dual(zf[nz:], blocks, layout)
    lam_lu, nu_lu = _split_dual(z_lu[nz:], blocks, layout)
    lam_c, nu_c = _split_dual(zf[nz:] + last[nz:], blocks, layout)
    return dict(dX=dX, dU=dU, lam=lam, nu=nu, lam_lu=lam_lu, nu_lu=nu_lu, e_lu=(KR.rel_err(lam_lu, lam), KR.rel_err(_flat(nu_lu), _flat(nu))),
                correction=(KR.rel_err(lam_c, lam), KR.rel_err(_flat(nu_c), _flat(nu))), refinements=count)


def identity_terms(blocks, dX, dU, lam, nu):
    """The three KKT identities node by node.  Returns (residuals, sizes): per identity a list of arrays -- the residual and the sum of the magnitudes of its terms
        terminal   Q_N dx_N + q_N - lambda_N
        state      Q_k dx_k + q_k + A_k' lambda_{k+1} + C_k' nu_k - lambda_k
        input      R_k du_k + r_k + B_k' lambda_{k+1} + D_k' nu_k"""
    N = len(blocks) - 1
    res, size = dict(terminal=[], state=[], input=[]), dict(terminal=[], state=[], input=[])
    o = blocks[N]
    Q = _sym(o["Q"])
    res["terminal"].append(Q @ dX[N] + o["q"] - lam[N])
    size["terminal"].append(np.abs(Q) @ np.abs(dX[N]) + np.abs(o["q"]) + np.abs(lam[N]))
    for k in range(N):
        o = blocks[k]
        nc = int(o["nc"])
        Q, R, C, D, v = _sym(o["Q"]), _sym(o["R"]), o["C"][:nc], o["D"][:nc], np.asarray(nu[k])[:nc]
        res["state"].append(Q @ dX[k] + o["q"] + o["A"].T @ lam[k + 1] + C.T @ v - lam[k])
        size["state"].append(np.abs(Q) @ np.abs(dX[k]) + np.abs(o["q"]) + np.abs(o["A"]).T @ np.abs(lam[k + 1]) + np.abs(C).T @ np.abs(v) + np.abs(lam[k]))
        res["input"].append(R @ dU[k] + o["r"] + o["B"].T @ lam[k + 1] + D.T @ v)
        size["input"].append(np.abs(R) @ np.abs(dU[k]) + np.abs(o["r"]) + np.abs(o["B"]).T @ np.abs(lam[k + 1]) + np.abs(D).T @ np.abs(v))
    return res, size


def worst_identity(blocks, dX, dU, lam, nu):
    """max over nodes and rows of |residual| / (sum of the magnitudes of the identity's terms), per identity: 1 means a term is missing, eps-size means it holds"""
    res, size = identity_terms(blocks, dX, dU, lam, nu)
    out = {}
    for key in res:
        r, s = (np.concatenate(res[key]), np.concatenate(size[key])) if res[key] else (np.zeros(0), np.zeros(0))
        out[key] = float((np.abs(r) / np.where(s > 0, s, 1.0)).max()) if r.size else 0.0
    return out


# an identity is a sum of at most 30 + 1 + 30 + 16 + 1 products: each side of a comparison evaluates it with a relative rounding error below TERMS eps of the sum of
# the magnitudes of its terms (the standard bound n eps sum|terms| of an n-term fp64 sum)
TERMS = 78


def rounding_floor(blocks, ref):
    """(floor_lam, floor_nu) in kkt_reference.rel_err over the instance: the error ONE fp64 evaluation of the defining identities makes at the exact solution --
    the least any fp64 route to these numbers can promise, whatever its order of operations.
        lambda_k is a 77-term sum: |d lambda_k| <= TERMS eps (|Q||dx| + |q| + |A'||lambda_{k+1}| + |C'||nu|);
        nu_k solves D' nu = -g with g a 61-term sum, and the solve (30 x nc) adds as many again:  |d nu_k| <= 2 TERMS eps |D'^+| (|R||du| + |r| + |B'||lambda_{k+1}|).
    Taken as the largest entry over the nodes, relative to |lambda|_inf and |nu|_inf of the instance.  No accumulation over the horizon is granted."""
    N = len(blocks) - 1
    lam, nu, dX, dU = ref["lam"], ref["nu"], ref["dX"], ref["dU"]
    worst_l, worst_n = 0.0, 0.0
    for k in range(N):
        o = blocks[k]
        nc = int(o["nc"])
        Q, R, C, D = _sym(o["Q"]), _sym(o["R"]), o["C"][:nc], o["D"][:nc]
        worst_l = max(worst_l, float((np.abs(Q) @ np.abs(dX[k]) + np.abs(o["q"]) + np.abs(o["A"]).T @ np.abs(lam[k + 1]) + np.abs(C).T @ np.abs(nu[k])).max()))
        if nc:
            g_abs = np.abs(R) @ np.abs(dU[k]) + np.abs(o["r"]) + np.abs(o["B"]).T @ np.abs(lam[k + 1])
            worst_n = max(worst_n, float((np.abs(np.linalg.pinv(D.T)) @ g_abs).max()))
    sl, sn = float(np.abs(lam).max()), float(np.abs(_flat(nu)).max()) if _flat(nu).size else 0.0
    return TERMS * EPS * worst_l / (sl if sl > 0 else 1.0), 2 * TERMS * EPS * worst_n / (sn if sn > 0 else 1.0)


def pad_nu(nu):
    """[N][NCMAX] with rows >= nc_k zero: the layout of qmgpu_mpc_dual_batch"""
    out = np.zeros((len(nu), NCMAX))
    for k, v in enumerate(nu):
        out[k, :len(v)] = v
    return out


def check_dual(sc, costate, nu, nc, product_lq, instances=None, record_path=None):
    """costate [B][N+1][30], nu [B][N][16], nc [B][N] of scenario sc against the reference built from the product's OWN LQ blocks (product_lq(i, k)) on `instances`
    (default: all), under the tolerance rule of this module; nc and the zero padding exact on every instance.  Every figure is printed (and recorded under
    record_path) before anything is asserted.  Returns (record, {i: (blocks, reference, tol)})."""
    B, N = sc.B, sc.N
    instances = list(range(B)) if instances is None else list(instances)
    rows, kept = [], {}
    for i in instances:
        blocks = [product_lq(i, k) for k in range(N + 1)]
        ref = solve(blocks)
        fl = rounding_floor(blocks, ref)
        rows.append(dict(i=i, e_lu=ref["e_lu"], floor=fl, correction=ref["correction"], err=(KR.rel_err(costate[i], ref["lam"]), KR.rel_err(nu[i], pad_nu(ref["nu"]))),
                         scale=(float(np.abs(ref["lam"]).max()), float(np.abs(pad_nu(ref["nu"])).max())), nc=sorted({int(b["nc"]) for b in blocks[:N]})))
        kept[i] = (blocks, ref)
    mx = lambda key: [max(r[key][j] for r in rows) for j in (0, 1)]  # noqa: E731
    e_lu, floor = mx("e_lu"), mx("floor")
    tol = [max(KS.FACTOR * e_lu[j], floor[j]) for j in (0, 1)]
    rec = dict(instances=len(instances), N=N, nc=sorted(set().union(*[r["nc"] for r in rows])), e_lu=e_lu, floor=floor, tolerance=tol, product=mx("err"),
               product_at=[max(rows, key=lambda r: r["err"][j])["i"] for j in (0, 1)], correction=mx("correction"),
               scale_costate=[min(r["scale"][0] for r in rows), max(r["scale"][0] for r in rows)], scale_nu=[min(r["scale"][1] for r in rows), max(r["scale"][1] for r in rows)])
    print(sc.name, json.dumps(rec))
    if record_path:
        os.makedirs(os.path.dirname(os.path.abspath(record_path)), exist_ok=True)
        try:
            allrec = json.load(open(record_path))
        except (OSError, ValueError):
            allrec = {}
        allrec[sc.name] = rec
        json.dump(allrec, open(record_path, "w"), indent=1)
    assert np.isfinite(costate).all() and np.isfinite(nu).all(), sc.name
    for i in range(B):
        for k in range(N):
            n = int(product_lq(i, k)["nc"]) if i in kept else int(nc[i, k])
            assert nc[i, k] == n and 0 <= n <= NCMAX and not nu[i, k, n:].any(), (sc.name, i, k, nc[i, k], n)
    for r in rows:
        for j, part in enumerate(("costate", "nu")):
            assert r["correction"][j] <= 1e-2 * tol[j], (sc.name, part, r, tol)
            assert r["err"][j] <= tol[j], (sc.name, part, r, tol)
    return rec, {i: kept[i] + (tol,) for i in kept}
