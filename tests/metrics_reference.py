"""A numpy-only reference for the SQP solution metrics (qmgpu_mpc_metrics_batch): per node the seven cost terms and their sum, the RK2 defect, the values of the
state-input equalities with nc; per trajectory the eight numbers of upstream's PerformanceIndex, summed with math.fsum.

Rule of lq_reference.py: nothing of support.Oracle, nothing under oracle/, no kernel-derived helper; of the product only the VALUES of interface.problem.settings.
Built from lq_reference's value functions (rk2 / flow, kinematics, references, ee_error, swing_reference, barrier, cone, nominal_input, the input weight, node_mode,
contact_flags), one real pass per node.  Force tracking is left out (ee_contact_ref = NULL), as in ls_reference.py.

Sign convention: lq_reference's.  defect = rk2(x, u, dt) - x_next is lq_node's b; eq is lq_node's e, the VALUE of the row, in lq_node's row order (foot by foot:
a swing foot's three zero-force rows then its normal-velocity row; a stance foot's three zero-velocity rows).

Magnitudes.  Next to every value the reference returns the sum of the magnitudes of the terms the value was formed from, one level down: a value y = sum_i t_i whose
terms carry their own rounding (t_i = g(z), z itself a sum) is given  sum_i |t_i| + |dg/dz| * (magnitude of z).  They are the scale of the tolerance rule
    |kernel - reference| <= C * eps * magnitude                                 (per node outputs)
    ... + (N + 2) * eps * sum |summand|                                          (the sums of performance)
with one C per output class, set in test_emu_metrics.py from ratios measured on the host build (profiles/metrics_parity.json)."""
import math

import numpy as np

import lq_reference as LR

EPS = np.finfo(np.float64).eps
NCMAX, NTERMS, NPERF = 16, 8, 8
CLASSES = ("defect", "eq", "cost_terms", "performance")


def _flow_mag(P, x, u):
    """flow map f(x, u) of lq_reference with the magnitude of every entry: sum |f_c| / m + g; sum |(p_c - com) x f_c| / m termwise; |A_b^-1| (m |h| + |A_j| |v_j|); |v_j|.
    Also the kinematics and the magnitude of the generalised velocity [v_b; v_j] the foot velocities are formed from."""
    f, kin = LR.flow(x[None, :].astype(complex), u[None, :].astype(complex), P.gravity)
    f = f[0].real
    A = kin["A"][0].real
    F = np.abs(u[:12].reshape(4, 3))
    r = np.abs((kin["feet"][0] - kin["com"][0]).real)
    lin = F.sum(axis=0) / LR.MASS + np.array([0.0, 0.0, P.gravity])
    ang = np.stack([r[:, 1] * F[:, 2] + r[:, 2] * F[:, 1], r[:, 2] * F[:, 0] + r[:, 0] * F[:, 2], r[:, 0] * F[:, 1] + r[:, 1] * F[:, 0]], axis=1).sum(axis=0) / LR.MASS
    vj = np.abs(u[12:30])
    vb = np.abs(np.linalg.inv(A[:, :6])) @ (LR.MASS * np.abs(x[:6]) + np.abs(A[:, 6:]) @ vj)
    return f, np.concatenate([lin, ang, vb, vj]), kin, np.concatenate([vb, vj])


def node_metrics(P, t, dt, x, u, xnext, terminal, events, modes, ttimes, tstates):
    """dict(terms [8], cost, defect [30], eq [16] zero padded, nc) and under "mag" the magnitudes of terms, cost, defect, eq.  Terminal node: terms[2] only, nc = 0."""
    x = np.asarray(x, float)
    xref, ee_pos, ee_quat = LR.references(ttimes, tstates, t)
    terms, tmag = np.zeros(NTERMS), np.zeros(NTERMS)
    out = dict(defect=np.zeros(30), eq=np.zeros(NCMAX), nc=0)
    mag = dict(defect=np.zeros(30), eq=np.zeros(NCMAX))

    def ee_term(kin, mu_p, mu_o):
        h = LR.ee_error(kin, ee_pos, ee_quat)[0].real
        mu = np.r_[np.full(3, mu_p), np.full(3, mu_o)]
        # h_pos = p_ee - p_ref; h_ori = quaternionDistance: three products of unit-quaternion entries per component, each at most 1
        hm = np.r_[np.abs(kin["ee"][0].real) + np.abs(ee_pos), np.full(3, 3.0)]
        return 0.5 * float(mu @ h**2), 0.5 * float(mu @ h**2) + float(mu @ (np.abs(h) * hm))

    if terminal:
        kin = LR.kinematics(x[None, 6:30])
        terms[2], tmag[2] = ee_term(kin, P.ee_final_mu_position, P.ee_final_mu_orientation)
        return dict(out, terms=terms, cost=float(terms[2]), mag=dict(mag, terms=tmag, cost=float(tmag[2])))
    u = np.asarray(u, float)
    xnext = np.asarray(xnext, float)
    mode = LR.node_mode(events, modes, t)
    fl = LR.contact_flags(mode)
    # ---- RK2 defect
    k1, k1m, kin, vmag = _flow_mag(P, x, u)
    k2, k2m, _, _ = _flow_mag(P, x + dt * k1, u)
    out["defect"] = x + 0.5 * dt * (k1 + k2) - xnext
    mag["defect"] = np.abs(x) + 0.5 * dt * (k1m + k2m) + np.abs(xnext)
    # ---- equality rows
    feet, J = kin["feet"][0].real, kin["Jfeet"][0].real               # J [4][24][3]
    fv = kin["footvel"][0].real
    fvm = np.einsum("d,cdk->ck", vmag, np.abs(J))
    rows, rmag = [], []
    for c in range(4):
        if fl[c]:
            rows += [fv[c, 0], fv[c, 1], fv[c, 2] + P.position_error_gain * feet[c, 2]]
            rmag += [fvm[c, 0], fvm[c, 1], fvm[c, 2] + P.position_error_gain * abs(feet[c, 2])]
        else:
            zp, zv = LR.swing_reference(P, events, modes, c, t)
            rows += [u[3 * c], u[3 * c + 1], u[3 * c + 2], fv[c, 2] - zv + P.position_error_gain * (feet[c, 2] - zp)]
            rmag += [abs(u[3 * c]), abs(u[3 * c + 1]), abs(u[3 * c + 2]), fvm[c, 2] + abs(zv) + P.position_error_gain * (abs(feet[c, 2]) + abs(zp))]
    out["nc"] = len(rows)
    out["eq"][:len(rows)] = rows
    mag["eq"][:len(rows)] = rmag
    # ---- cost terms
    unom = LR.nominal_input(P, mode)
    dx, du = x - xref, u - unom
    terms[0], terms[1] = 0.5 * dx @ P.Q @ dx, 0.5 * du @ P.R @ du
    tmag[0] = 0.5 * np.abs(dx) @ np.abs(P.Q) @ np.abs(dx) + np.abs(P.Q @ dx) @ (np.abs(x) + np.abs(xref))
    tmag[1] = 0.5 * np.abs(du) @ np.abs(P.R) @ np.abs(du) + np.abs(P.R @ du) @ (np.abs(u) + np.abs(unom))
    terms[2], tmag[2] = ee_term(kin, P.ee_mu_position, P.ee_mu_orientation)
    for slot, m_, d_, vals, los, ups in ((3, P.joint_pos_barrier_mu, P.joint_pos_barrier_delta, x[24:30], LR.ARM_LOWER, LR.ARM_UPPER),
                                         (4, P.joint_vel_barrier_mu, P.joint_vel_barrier_delta, u[24:30], P.arm_vel_lower, P.arm_vel_upper)):
        for val, lo, up in zip(vals, los, ups):
            parts = [LR.barrier(m_, d_, val - lo), LR.barrier(m_, d_, up - val), LR.barrier(m_, d_, 0.0 - lo), LR.barrier(m_, d_, up - 0.0)]
            terms[slot] += parts[0] + parts[1] - parts[2] - parts[3]
            tmag[slot] += sum(abs(p_) for p_ in parts) + abs(LR.barrier_slope(m_, d_, val - lo)) * (abs(val) + abs(lo)) + abs(LR.barrier_slope(m_, d_, up - val)) * (abs(val) + abs(up))
    for c in range(4):
        if fl[c]:
            f = u[3 * c:3 * c + 3]
            h = LR.cone(P, f)
            terms[5] += LR.barrier(P.friction_barrier_mu, P.friction_barrier_delta, h)
            hm = P.friction_coefficient * abs(f[2]) + np.sqrt(f[0] ** 2 + f[1] ** 2 + P.friction_regularization)
            tmag[5] += abs(LR.barrier(P.friction_barrier_mu, P.friction_barrier_delta, h)) + abs(LR.barrier_slope(P.friction_barrier_mu, P.friction_barrier_delta, h)) * hm
    cost = ((((((terms[0] + terms[1]) + terms[2]) + terms[3]) + terms[4]) + terms[5]) + terms[6])
    return dict(out, terms=terms, cost=float(cost), mag=dict(mag, terms=tmag, cost=float(tmag.sum())))


def trajectory_metrics(P, grid, X, U, events, modes, ttimes, tstates, x0=None):
    """Every output of the call for one instance: node_cost [N+1], cost_terms [N+1][8], defect [N][30], eq [N][16], nc [N], performance [8]; under "mag" the
    magnitudes of cost_terms, node_cost, defect, eq and of performance (the sum rule's (N + 2) eps sum |summand| already divided by eps and added in)."""
    grid = np.asarray(grid, float)
    N = len(grid) - 1
    nodes = [node_metrics(P, grid[k], 0.0 if k == N else grid[k + 1] - grid[k], X[k], None if k == N else U[k], None if k == N else X[k + 1], k == N,
                          events, modes, ttimes, tstates) for k in range(N + 1)]
    dts = np.r_[np.diff(grid), 1.0]
    o = dict(node_cost=np.array([n["cost"] for n in nodes]), cost_terms=np.array([n["terms"] for n in nodes]), defect=np.array([n["defect"] for n in nodes[:N]]),
             eq=np.array([n["eq"] for n in nodes[:N]]), nc=np.array([n["nc"] for n in nodes[:N]], dtype=np.int32))
    m = dict(node_cost=np.array([n["mag"]["cost"] for n in nodes]), cost_terms=np.array([n["mag"]["terms"] for n in nodes]),
             defect=np.array([n["mag"]["defect"] for n in nodes[:N]]), eq=np.array([n["mag"]["eq"] for n in nodes[:N]]))
    cost_s = [dts[k] * o["node_cost"][k] for k in range(N + 1)]
    dyn_s = [dts[k] * float(o["defect"][k] @ o["defect"][k]) for k in range(N)]
    eq_s = [dts[k] * float(o["eq"][k] @ o["eq"][k]) for k in range(N)]
    # |d|^2 from entries d_i of magnitude m_i: sum d_i^2 + 2 |d_i| m_i
    dyn_m = [dts[k] * float(o["defect"][k] @ o["defect"][k] + 2 * np.abs(o["defect"][k]) @ m["defect"][k]) for k in range(N)]
    eq_m = [dts[k] * float(o["eq"][k] @ o["eq"][k] + 2 * np.abs(o["eq"][k]) @ m["eq"][k]) for k in range(N)]
    cost_m = [dts[k] * m["node_cost"][k] for k in range(N + 1)]
    if x0 is not None:
        d = np.asarray(x0, float) - X[0]
        dyn_s.append(float(d @ d))
        dyn_m.append(float(d @ d + 2 * np.abs(d) @ (np.abs(x0) + np.abs(X[0]))))
    perf, pm = np.zeros(NPERF), np.zeros(NPERF)
    perf[0] = perf[1] = math.fsum(cost_s)
    perf[3], perf[4] = math.fsum(dyn_s), math.fsum(eq_s)
    for slot, mags, summands in ((0, cost_m, cost_s), (1, cost_m, cost_s), (3, dyn_m, dyn_s), (4, eq_m, eq_s)):
        pm[slot] = math.fsum(mags)
    o["performance"] = perf
    m["performance"] = pm
    m["performance_sum"] = np.array([(N + 2) * math.fsum(abs(v) for v in s) for s in (cost_s, cost_s, [], dyn_s, eq_s, [], [], [])])
    o["mag"] = m
    return o


def ratios(got, ref):
    """worst |got - ref| / (eps * magnitude) per output class of one instance (got: the call's arrays of that instance; ref: trajectory_metrics).  The performance
    class is measured against the magnitude alone: the sum rule's own allowance is subtracted from the difference first."""
    m = ref["mag"]
    out = {}
    for cls, key in (("defect", "defect"), ("eq", "eq"), ("cost_terms", "cost_terms")):
        d, s = np.abs(got[key] - ref[key]), m[key]
        assert (d[s == 0] == 0).all(), (cls, "a value without terms must be exact")
        out[cls] = float((d[s > 0] / (EPS * s[s > 0])).max()) if (s > 0).any() else 0.0
    d = np.maximum(np.abs(got["performance"] - ref["performance"]) - EPS * m["performance_sum"], 0.0)
    s = m["performance"]
    assert (d[s == 0] == 0).all()
    out["performance"] = float((d[s > 0] / (EPS * s[s > 0])).max())
    return out


def within(got, ref, C):
    """the tolerance rule, every entry: returns the list of (class, worst excess ratio) that break it (empty: all within)"""
    r = ratios(got, ref)
    return [(cls, r[cls], C[cls]) for cls in CLASSES if r[cls] > C[cls]]
