"""High-precision reference for ONE SQP step, independent of the projected Riccati recursion that the kernels and the oracle both implement.

The per-node LQ blocks of one instance (as qmgpu_debug_get_lq or oracle.lq_node return them) define the equality-constrained QP

    min  sum_k 1/2 dx_k' Q_k dx_k + q_k' dx_k + 1/2 du_k' R_k du_k + r_k' du_k   (+ 1/2 dx_N' Q_N dx_N + q_N' dx_N)
    s.t. dx_0 = dx0,   dx_{k+1} = A_k dx_k + B_k du_k + b_k,   C_k dx_k + D_k du_k + e_k = 0

(the formulation of test_oracle_invariants.py::test_riccati_step_equals_dense_kkt_solve).  Its KKT system is assembled sparse, factorised once by
SuperLU in fp64 and refined iteratively with the residual b - K z formed in np.longdouble until the correction stops shrinking.  Test helper, no GPU.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

EPS = np.finfo(np.float64).eps
MAX_REFINEMENTS = 30


def assemble(blocks, dx0):
    """KKT matrix (csc, fp64) and right-hand side of the QP above.  blocks: N + 1 dicts, A B b Q R q r C D e nc for k < N, Q q for k = N.
    Unknowns: [dx_0 .. dx_N, du_0 .. du_{N-1}, multipliers]; Q and R enter through their symmetric parts (the Hessian of the quadratic form)."""
    N = len(blocks) - 1
    nx = blocks[N]["Q"].shape[0]
    nu = blocks[0]["R"].shape[0] if N > 0 else 0
    nz = nx * (N + 1) + nu * N
    ix = lambda k: nx * k                      # noqa: E731
    iu = lambda k: nx * (N + 1) + nu * k       # noqa: E731
    rows, cols, vals = [], [], []
    g = np.zeros(nz)

    def put(r0, c0, M):
        M = np.asarray(M, dtype=np.float64)
        i, j = np.nonzero(M)
        rows.append(r0 + i); cols.append(c0 + j); vals.append(M[i, j])

    for k, o in enumerate(blocks):
        put(ix(k), ix(k), 0.5 * (o["Q"] + o["Q"].T)); g[ix(k):ix(k) + nx] += o["q"]
        if k < N:
            put(iu(k), iu(k), 0.5 * (o["R"] + o["R"].T)); g[iu(k):iu(k) + nu] += o["r"]
    # equality rows E z = f: below the Hessian, and E' to its right
    eqs, f, m = [], [], 0

    def eq(c0, M):
        M = np.asarray(M, dtype=np.float64)
        i, j = np.nonzero(M)
        eqs.append((m + i, c0 + j, M[i, j]))

    eq(ix(0), np.eye(nx)); f.append(np.asarray(dx0, dtype=np.float64)); m += nx
    for k in range(N):
        o = blocks[k]
        eq(ix(k), o["A"]); eq(iu(k), o["B"]); eq(ix(k + 1), -np.eye(nx)); f.append(-np.asarray(o["b"], dtype=np.float64)); m += nx
        nc = int(o["nc"])
        if nc:
            eq(ix(k), o["C"][:nc]); eq(iu(k), o["D"][:nc]); f.append(-np.asarray(o["e"][:nc], dtype=np.float64)); m += nc
    er, ec, ev = (np.concatenate([t[i] for t in eqs]) for i in range(3))
    rows += [nz + er, ec]; cols += [ec, nz + er]; vals += [ev, ev]
    n = nz + m
    K = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    K.sum_duplicates()
    return K, np.r_[-g, np.concatenate(f)], (N, nx, nu)


def _split(z, layout):
    N, nx, nu = layout
    return z[:nx * (N + 1)].reshape(N + 1, nx), z[nx * (N + 1):nx * (N + 1) + nu * N].reshape(N, nu)


def rel_err(got, ref):
    """||got - ref||_inf / ||ref||_inf: the measure of every step error of the KKT checks"""
    if np.size(ref) == 0:
        return 0.0
    scale = float(np.abs(ref).max())
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)).max() / (scale if scale > 0 else 1.0))


def solve(blocks, dx0=None):
    """The step of the QP of `blocks`.  dict(dX [N+1][nx], dU [N][nu]: the refined solution; dX_lu, dU_lu: the plain fp64 LU solution; correction =
    (dX part, dU part) of the last refinement correction in the measure of rel_err -- a bound on the refined solution's own error; refinements: the
    number of corrections computed)."""
    N = len(blocks) - 1
    nx = blocks[N]["Q"].shape[0]
    K, rhs, layout = assemble(blocks, np.zeros(nx) if dx0 is None else dx0)
    lu = spla.splu(K, permc_spec="COLAMD", diag_pivot_thresh=1.0)       # partial pivoting: the KKT matrix is symmetric indefinite
    z = lu.solve(rhs)
    z_lu = z.copy()
    # residual in extended precision: products of the row-sorted entries, summed per row
    Kr = K.tocsr()
    assert (np.diff(Kr.indptr) > 0).all()                                # no empty row (reduceat would not give 0 for one)
    data, starts = Kr.data.astype(np.longdouble), Kr.indptr[:-1]
    rhs_l, zl = rhs.astype(np.longdouble), z.astype(np.longdouble)
    prev, last, count = np.inf, np.zeros_like(z), 0
    for _ in range(MAX_REFINEMENTS):
        res = rhs_l - np.add.reduceat(data * zl[Kr.indices], starts)
        d = lu.solve(res.astype(np.float64))
        size = float(np.abs(d).max())
        zl += d
        count, last = count + 1, d
        if size == 0.0 or size >= prev:
            break
        prev = size
    dX, dU = _split(zl.astype(np.float64), layout)
    cX, cU = _split(last, layout)
    dX_lu, dU_lu = _split(z_lu, layout)
    return dict(dX=dX, dU=dU, dX_lu=dX_lu, dU_lu=dU_lu, correction=(rel_err(dX + cX, dX), rel_err(dU + cU, dU)), refinements=count)


def oracle_blocks(oracle, grid, X, U, nev, ev, md, tt, ts):
    """LQ blocks of one instance at the iterate (X, U) on the shooting grid, from the oracle.  X[0] must be x0 already: both solvers overwrite it
    before they linearise, so dx_0 = 0."""
    N = len(grid) - 1
    out = [oracle.lq_node(grid[k], grid[k + 1] - grid[k], X[k], U[k], X[k + 1], False, nev, ev, md, tt, ts) for k in range(N)]
    out.append(oracle.lq_node(grid[N], 0.0, X[N], None, X[N], True, nev, ev, md, tt, ts))
    return out
