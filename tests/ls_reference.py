"""A numpy-only reference for the filter line search and the convergence test of one SQP iteration: the value-only node evaluation, the performance sums,
FilterLinesearch::acceptStep, the sequential trial loop and SqpSolver::checkConvergence, written from the upstream rules.

Rule of lq_reference.py: nothing of support.Oracle, nothing under oracle/, no kernel-derived helper; of the product only the VALUES of interface.problem.settings.
The node evaluation is built from lq_reference's value functions (rk2, kinematics, swing_reference, references, ee_error, barrier, cone, nominal_input, the input
weight), one real pass per node.  Force tracking is left out (ee_contact_ref = NULL).

Every comparison the filter, the trial loop and the convergence test evaluate is reported as an (lhs, rhs) pair (the test is always lhs < rhs or lhs > rhs), so that a
scenario can assert its decision margin: a correct implementation in another order of summation can then never flip a decision by rounding.  Comparisons of integers
(the iteration limit) are exact and not reported."""
import numpy as np

import lq_reference as LR

LS_SETTINGS = ("g_max", "g_min", "alpha_min", "alpha_decay", "gamma_c", "armijo_factor", "cost_tol", "delta_tol")


class Params(LR.Params):
    """lq_reference.Params and the line-search / convergence settings"""
    def __init__(self, settings):
        super().__init__(settings)
        for name in LS_SETTINGS:
            setattr(self, name, float(getattr(settings, name)))
        self.sqp_iterations = int(settings.sqp_iterations)


# ------------------------------------------------------------------------------------------------ one node, values only
def node_performance(P, t, dt, x, u, xnext, terminal, events, modes, ttimes, tstates):
    """(cost, dyn_sse, eq_sse) of the node at (x, u, xnext): the dt-scaled cost of lq_reference.lq_node, dt |rk2(x, u) - xnext|^2 and dt |e|^2 with lq_node's rows.
    Terminal node: the cost only (the other two are 0)."""
    x = np.asarray(x, float)
    xref, ee_pos, ee_quat = LR.references(ttimes, tstates, t)
    if terminal:
        kin = LR.kinematics(x[None, 6:30])
        h = LR.ee_error(kin, ee_pos, ee_quat)[0].real
        mu = np.r_[np.full(3, P.ee_final_mu_position), np.full(3, P.ee_final_mu_orientation)]
        return 0.5 * float(mu @ h**2), 0.0, 0.0
    u = np.asarray(u, float)
    mode = LR.node_mode(events, modes, t)
    fl = LR.contact_flags(mode)
    xp, kin = LR.rk2(x[None, :].astype(complex), u[None, :].astype(complex), dt, P.gravity)
    defect = xp[0].real - np.asarray(xnext, float)
    rows = []
    for c in range(4):
        fv, fz = kin["footvel"][0, c].real, kin["feet"][0, c, 2].real
        if fl[c]:
            rows += [fv[0], fv[1], fv[2] + P.position_error_gain * fz]
        else:
            zp, zv = LR.swing_reference(P, events, modes, c, t)
            rows += [u[3 * c], u[3 * c + 1], u[3 * c + 2], fv[2] - zv + P.position_error_gain * (fz - zp)]
    e = np.array(rows)
    dx, du = x - xref, u - LR.nominal_input(P, mode)
    cost = 0.5 * dx @ P.Q @ dx + 0.5 * du @ P.R @ du
    h = LR.ee_error(kin, ee_pos, ee_quat)[0].real
    cost += 0.5 * float(np.r_[np.full(3, P.ee_mu_position), np.full(3, P.ee_mu_orientation)] @ h**2)
    for i in range(6):
        for m_, d_, val, lo, up in ((P.joint_pos_barrier_mu, P.joint_pos_barrier_delta, x[24 + i], LR.ARM_LOWER[i], LR.ARM_UPPER[i]),
                                    (P.joint_vel_barrier_mu, P.joint_vel_barrier_delta, u[24 + i], P.arm_vel_lower[i], P.arm_vel_upper[i])):
            cost += LR.barrier(m_, d_, val - lo) + LR.barrier(m_, d_, up - val) - LR.barrier(m_, d_, 0.0 - lo) - LR.barrier(m_, d_, up - 0.0)
    for c in range(4):
        if fl[c]:
            cost += LR.barrier(P.friction_barrier_mu, P.friction_barrier_delta, LR.cone(P, u[3 * c:3 * c + 3]))
    return dt * float(cost), dt * float(defect @ defect), dt * float(e @ e)


def node_args(grid, X, U, events, modes, ttimes, tstates, k):
    """the arguments of node_performance / lq_reference.lq_node for node k of a trajectory on `grid`"""
    N = len(grid) - 1
    term = k == N
    return dict(t=grid[k], dt=0.0 if term else grid[k + 1] - grid[k], x=X[k], u=None if term else U[k], xnext=None if term else X[k + 1], terminal=term,
                events=events, modes=modes, ttimes=ttimes, tstates=tstates)


def performance(P, grid, X, U, events, modes, ttimes, tstates):
    """(merit, violation) of a trajectory: the sum of the node costs, sqrt(sum dyn_sse + sum eq_sse)"""
    per = np.array([node_performance(P, **node_args(grid, X, U, events, modes, ttimes, tstates, k)) for k in range(len(grid))])
    return float(per[:, 0].sum()), float(np.sqrt(per[:, 1].sum() + per[:, 2].sum()))


# ------------------------------------------------------------------------------------------------ the filter
def _lt(log, lhs, rhs):
    log.append((float(lhs), float(rhs)))
    return lhs < rhs


def accept_step(P, base, trial, alpha_armijo, line_search=True, log=None):
    """upstream FilterLinesearch::acceptStep: (accepted, step type) of the trial (merit, violation) against the baseline's, alpha_armijo = alpha * Armijo metric.
    Type 1: the constraint violation decides; 3: the Armijo condition on the cost; 2: cost or violation; 0: line search off."""
    log = [] if log is None else log
    (m0, v0), (m1, v1) = base, trial
    if not line_search:
        return True, 0
    if _lt(log, P.g_max, v1):                                                          # v1 > g_max
        return _lt(log, v1, (1.0 - P.gamma_c) * v0), 1
    if _lt(log, v1, P.g_min) and _lt(log, v0, P.g_min) and _lt(log, alpha_armijo, 0.0):
        return _lt(log, m1, m0 + P.armijo_factor * alpha_armijo), 3
    by_merit, by_violation = _lt(log, m1, m0 - P.gamma_c * v0), _lt(log, v1, (1.0 - P.gamma_c) * v0)    # both reported: either may be the one that decides
    return by_merit or by_violation, 2


def line_search(P, perf, base, armijo, on=True):
    """The sequential loop of SqpSolver::takeStep: trial steps alpha = 1, alpha_decay, alpha_decay^2, ... one at a time until one is accepted or alpha < alpha_min.
    perf(alpha) -> (merit, violation) of the trial iterate; base: the baseline's.  Nothing accepted: alpha 0, type 4, the outcome is the baseline.
    Returns dict(alpha, type, merit, violation, trail = [(alpha, type, accepted, merit, violation, by_merit, by_violation)], comparisons)."""
    log, trail = [], []
    alpha = 1.0
    while True:
        m1, v1 = perf(alpha)
        n = len(log)
        ok, kind = accept_step(P, base, (m1, v1), alpha * armijo, on, log)
        clauses = (log[-2][0] < log[-2][1], log[-1][0] < log[-1][1]) if kind == 2 else (None, None)
        trail.append((alpha, kind, ok, m1, v1) + clauses)
        assert len(log) > n or not on
        if ok:
            return dict(alpha=alpha, type=kind, merit=m1, violation=v1, trail=trail, comparisons=log)
        alpha *= P.alpha_decay
        if _lt(log, alpha, P.alpha_min):
            return dict(alpha=0.0, type=4, merit=base[0], violation=base[1], trail=trail, comparisons=log)


def convergence_conditions(P, iteration, alpha, m0, m1, v1, dx_norm, du_norm, log=None):
    """the four conditions of SqpSolver::checkConvergence, each on its own: {1: iteration limit, 2: step size, 3: metrics, 4: primal step}"""
    log = [] if log is None else log
    return {1: iteration + 1 >= P.sqp_iterations,
            2: _lt(log, alpha, P.alpha_min),
            3: _lt(log, abs(m1 - m0), P.cost_tol) & _lt(log, v1, P.g_min),
            4: _lt(log, alpha * dx_norm, P.delta_tol) & _lt(log, alpha * du_norm, P.delta_tol)}


def check_convergence(P, iteration, alpha, m0, m1, v1, dx_norm, du_norm):
    """(reason, comparisons): 1 iteration limit, 2 alpha < alpha_min, 3 |m1 - m0| < cost_tol and v1 < g_min, 4 alpha |dX| < delta_tol and alpha |dU| < delta_tol, 0 none;
    the first that holds, in this order.  Only the comparisons in front of the deciding one (and that one) are evaluated, as upstream's if-chain does."""
    log = []
    if iteration + 1 >= P.sqp_iterations:
        return 1, log
    if _lt(log, alpha, P.alpha_min):
        return 2, log
    if _lt(log, abs(m1 - m0), P.cost_tol) and _lt(log, v1, P.g_min):
        return 3, log
    if _lt(log, alpha * dx_norm, P.delta_tol) and _lt(log, alpha * du_norm, P.delta_tol):
        return 4, log
    return 0, log


def margin(comparisons):
    """the smallest |lhs - rhs| / max(|lhs|, |rhs|, 1e-12) of a list of comparisons (inf for none)"""
    return min([abs(a - b) / max(abs(a), abs(b), 1e-12) for a, b in comparisons], default=np.inf)


# ------------------------------------------------------------------------------------------------ Armijo metric, one iteration
def armijo_metric(blocks, dX, dU, projected=True):
    """The Armijo descent metric of the step.  projected = False: sum_k q_k . dx_k + r_k . du_k (terminal node: q_N . dx_N), the directional derivative of the cost
    model along the step.  projected = True: what upstream's SqpSolver::getOCPSolution evaluates -- armijoDescentMetric of the PROJECTED cost and the projected
    input step, before the input is mapped back: sum_k q~_k . dx_k + r~_k . du~_k with du = Pe + Px dx + Pu du~, q~ = q + Px'(r + R Pe), r~ = Pu'(r + R Pe), that is
    sum_k q_k . dx_k + (r_k + R_k Pe_k) . (du_k - Pe_k), Pe_k = -D_k^+ e_k the least-norm input that meets the node's equality rows.  The two agree where e = 0
    (a feasible iterate: the only place the filter reads the metric, type 3 needs viol0 < g_min)."""
    N = len(blocks) - 1
    total = float(blocks[N]["q"] @ dX[N])
    for k in range(N):
        o = blocks[k]
        nc = int(o["nc"])
        Pe = -np.linalg.pinv(o["D"][:nc]) @ o["e"][:nc] if projected and nc else np.zeros(len(dU[k]))
        total += float(o["q"] @ dX[k] + (o["r"] + 0.5 * (o["R"] + o["R"].T) @ Pe) @ (dU[k] - Pe))
    return total


def iteration(P, grid, X, U, events, modes, ttimes, tstates, dX, dU, armijo, line_search_on=True, iteration_index=0):
    """One SQP iteration behind the direction: baseline performance, line search, new iterate, convergence test.  dict(base, ls, reason, comparisons, X, U)."""
    perf = lambda a: performance(P, grid, X + a * dX, U + a * dU, events, modes, ttimes, tstates)  # noqa: E731
    base = performance(P, grid, X, U, events, modes, ttimes, tstates)
    ls = line_search(P, perf, base, armijo, line_search_on)
    a = ls["alpha"]
    norms = float(np.sqrt((dX**2).sum())), float(np.sqrt((dU**2).sum()))
    reason, clog = check_convergence(P, iteration_index, a, base[0], ls["merit"], ls["violation"], *norms)
    conds = convergence_conditions(P, iteration_index, a, base[0], ls["merit"], ls["violation"], *norms)
    return dict(base=base, ls=ls, reason=reason, conditions=conds, comparisons=ls["comparisons"] + clog, norms=norms,
                X=X.copy() if a == 0.0 else X + a * dX, U=U.copy() if a == 0.0 else U + a * dU)
