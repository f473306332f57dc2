"""numpy statement of the WBC solution report (include/qmgpu.h: qmgpu_wbc_report_batch), the reference of test_emu_wbc_report.py /
test_gpu_wbc_report.py.

Task data: the oracle's stacked tasks support.Oracle.wbc_task(level, ...) = (A, b, D, f) per level, and M, nle, the feet Jacobian of support.Oracle.wbc_model for the
torque.  The products A x - b, f - D x and M_j a - J_j' F + nle_j are accumulated in numpy.longdouble.

Tolerance rule, from the reference alone, per row i:   tol_i = 10 max(e_np_i, e_in_i, floor_i)
    e_np   (n_terms + 1) eps (|A_i| |x| + |b_i|): the rounding of a sum of n_terms products formed in any order (n_terms = 36 for a task row, 37 for a torque row:
           its three-term sum M_j a - J_j' F + nle_j has 24 + 12 + 1 summands); D, f for the margins;
    e_in   the spread of the row over five seeded draws in which rbd_measured, state_desired, input_desired and input_last are perturbed by 4 eps relative and the
           oracle's task data rebuilt: the conditioning of the inputs (it covers (v_des - input_last) / period).  Any implementation that forms these terms in
           another order is entitled to it;
    floor  eps times the row's scale |A_i| |x| + |b_i|;
    10     the factor the value-function, dual and plant tests grant.
summary: a 2-norm moves by at most the 2-norm of its rows' errors, and its own sum of r squares and root round by (r + 2) eps of it; an inf-norm and a minimum move
by at most the largest error of their rows; counts are exact where every margin lies farther than 2 tol_i from both thresholds +-active_tol (1 + |f_i|) (`separated`;
2: the threshold itself is formed from an f that carries the row's error); the row of minimum margin is any row within the two rows' tolerances of the minimum.
"""
import numpy as np

import support as S

EPS = np.finfo(np.float64).eps
LD = np.longdouble
FACTOR = 10.0
LEVELS, EQ_ROWS, INEQ_ROWS, NSUM = 3, 22, 56, 12
ROW_TERMS, TAU_TERMS = 36, 37
DRAWS = 5


def effort_limits(problem):
    lim = np.array(problem.model.effort_limit[:])
    return np.r_[np.tile(lim[:3], 4), lim[12:18]]


def task_data(orc, inp, i, variant, ee_force=None):
    """the oracle's stacked tasks of instance i of the inputs `inp` (dict xd u rbd mode t il period, arrays over instances), and the model terms of the torque"""
    args = (inp["xd"][i], inp["u"][i], np.ascontiguousarray(inp["rbd"][i]), int(inp["mode"][i]), float(inp["period"][i]), float(inp["t"][i]), inp["il"][i])
    levels = [orc.wbc_task(level, *args, variant=variant) for level in range(LEVELS)]
    o = orc.wbc_model(args[0], args[1], args[2], args[4], args[6])
    nle = o["nle"].copy()
    if ee_force is not None:
        nle = nle - o["armJ"][:3].T @ np.asarray(ee_force, float)
    return dict(levels=levels, M=o["M"].copy(), nle=nle, J=o["J"].copy())


def perturbed(inp, i, rng):
    """instance i alone with rbd, xd, u, il perturbed by 4 eps relative"""
    pert = lambda a: a * (1.0 + 4 * EPS * rng.uniform(-1, 1, np.shape(a)))  # noqa: E731
    one = {k: np.asarray(v)[i:i + 1].copy() for k, v in inp.items()}
    for k in ("rbd", "xd", "u", "il"):
        one[k] = pert(one[k])
    return one


def tick_data(orc, inp, i, variant, seed=0):
    """everything of the reference that does not depend on x: the task data of instance i and of its DRAWS perturbed copies.  Computed once per instance, shared by every
    comparison of that instance."""
    rng = np.random.default_rng(1000 + seed)
    return dict(base=task_data(orc, inp, i, variant), draws=[task_data(orc, perturbed(inp, i, rng), 0, variant) for _ in range(DRAWS)], mode=int(inp["mode"][i]))


def evaluate(td, x):
    """(values, scales) of one set of task data at x: eq [3][22], ineq [56], tau [18], rows zero-filled; scale = sum |terms| per row; rows = r_0 r_1 r_2 m_0"""
    xl, xa = np.asarray(x, dtype=LD), np.abs(np.asarray(x, float))
    eq, eqs = np.zeros((LEVELS, EQ_ROWS)), np.zeros((LEVELS, EQ_ROWS))
    rows = []
    for level, T in enumerate(td["levels"]):
        r = T["A"].shape[0]
        rows.append(r)
        eq[level, :r] = (T["A"].astype(LD) @ xl - T["b"].astype(LD)).astype(np.float64)
        eqs[level, :r] = np.abs(T["A"]) @ xa + np.abs(T["b"])
    D, f = td["levels"][0]["D"], td["levels"][0]["f"]
    m0 = D.shape[0]
    rows.append(m0)
    ineq, ineqs = np.zeros(INEQ_ROWS), np.zeros(INEQ_ROWS)
    ineq[:m0] = (f.astype(LD) - D.astype(LD) @ xl).astype(np.float64)
    ineqs[:m0] = np.abs(D) @ xa + np.abs(f)
    Mj, Jj, nlej = td["M"][6:], td["J"][:, 6:].T, td["nle"][6:]
    tau = (Mj.astype(LD) @ xl[:24] - Jj.astype(LD) @ xl[24:] + nlej.astype(LD)).astype(np.float64)
    taus = np.abs(Mj) @ xa[:24] + np.abs(Jj) @ xa[24:] + np.abs(nlej)
    return dict(eq=eq, ineq=ineq, tau=tau, rows=np.array(rows, dtype=np.int32)), dict(eq=eqs, ineq=ineqs, tau=taus)


def report(tick, x, active_tol):
    """the report of one instance at x: dict(eq_residual, ineq_margin, tau, rows, summary), tol (the same keys; rows and the counts exact), separated, f (the f0 of the rows)"""
    val, scale = evaluate(tick["base"], x)
    spread = {k: np.zeros_like(val[k]) for k in ("eq", "ineq", "tau")}
    for d in tick["draws"]:
        v, _ = evaluate(d, x)
        assert np.array_equal(v["rows"], val["rows"])
        for k in spread:
            spread[k] = np.maximum(spread[k], np.abs(v[k] - val[k]))
    terms = dict(eq=ROW_TERMS, ineq=ROW_TERMS, tau=TAU_TERMS)
    tol = {k: FACTOR * np.maximum(np.maximum((terms[k] + 1) * EPS * scale[k], spread[k]), EPS * scale[k]) for k in spread}
    r0, r1, r2, m0 = (int(v) for v in val["rows"])
    nst = sum(S.contact_flags(tick["mode"]))
    assert r0 == 18 and m0 == 36 + 5 * nst + 3 * (4 - nst)
    f = np.zeros(INEQ_ROWS); f[:m0] = tick["base"]["levels"][0]["f"]
    thr = active_tol * (1.0 + np.abs(f))
    mg, mt = val["ineq"], tol["ineq"]
    summary, stol = np.zeros(NSUM), np.zeros(NSUM)
    for level, r in enumerate((r0, r1, r2)):
        e = val["eq"][level, :r]
        summary[level] = float(np.sqrt(np.sum(e.astype(LD) ** 2)))
        summary[3 + level] = np.abs(e).max() if r else 0.0
        stol[level] = float(np.sqrt(np.sum(tol["eq"][level, :r] ** 2))) + (r + 2) * EPS * summary[level]
        stol[3 + level] = tol["eq"][level, :r].max() if r else 0.0
    summary[6], stol[6] = mg[:36].min(), mt[:36].max()
    fr = slice(36, 36 + 5 * nst)
    summary[7], stol[7] = (mg[fr].min(), mt[fr].max()) if nst else (np.inf, 0.0)
    summary[8] = float((mg[:m0] <= thr[:m0]).sum())
    summary[9] = float((mg[:m0] < -thr[:m0]).sum())
    summary[10] = float(np.argmin(mg[:m0]))
    separated = bool((np.abs(mg[:m0] - thr[:m0]) > 2 * mt[:m0]).all() and (np.abs(mg[:m0] + thr[:m0]) > 2 * mt[:m0]).all())
    return dict(eq_residual=val["eq"], ineq_margin=mg, tau=val["tau"], rows=val["rows"], summary=summary, separated=separated, f=f,
                tol=dict(eq_residual=tol["eq"], ineq_margin=mt, tau=tol["tau"], summary=stol))


def fractions(got, ref):
    """worst |got - ref| / tol per output (the largest fraction of its bound an output uses), inf where an exact entry differs; got: dict of one instance's outputs"""
    out = {}
    for k in ("eq_residual", "ineq_margin", "tau"):
        err, tol = np.abs(np.asarray(got[k], float) - ref[k]), ref["tol"][k]
        with np.errstate(divide="ignore", invalid="ignore"):
            fr = np.where(err == 0.0, 0.0, err / tol)      # (a zero-filled row has tol 0: any difference there is inf)
        out[k] = float(np.nan_to_num(fr, nan=np.inf).max())
    s, rs, st = np.asarray(got["summary"], float), ref["summary"], ref["tol"]["summary"]
    worst = 0.0
    for j in range(8):
        if np.isinf(rs[j]):
            worst = max(worst, 0.0 if s[j] == rs[j] else np.inf)
        else:
            e = abs(s[j] - rs[j])
            worst = max(worst, 0.0 if e == 0.0 else (e / st[j] if st[j] > 0 else np.inf))
    m0 = int(ref["rows"][3])
    k = int(s[10])
    if not (0 <= k < m0 and s[10] == k):
        worst = np.inf
    else:   # the row the kernel names is, for the reference, within the two rows' tolerances of the minimum
        kmin = int(rs[10])
        gap, room = ref["ineq_margin"][k] - ref["ineq_margin"][kmin], ref["tol"]["ineq_margin"][k] + ref["tol"]["ineq_margin"][kmin]
        worst = max(worst, 0.0 if gap == 0.0 else (gap / room if room > 0 else np.inf))
    if s[11] != 0.0:
        worst = np.inf
    out["summary"] = float(worst)
    out["rows"] = 0.0 if np.array_equal(np.asarray(got["rows"]), ref["rows"]) else np.inf
    out["counts"] = 0.0 if (not ref["separated"] or (s[8] == rs[8] and s[9] == rs[9])) else np.inf
    return out
