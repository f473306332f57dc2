"""numpy statement of the plant step (include/qmgpu.h: qmgpu_plant_step_batch), the reference of test_emu_plant.py / test_gpu_plant.py.

Model terms: M, nle, the feet Jacobian and the arm Jacobian of support.Oracle.wbc_model at the same rbd (the terms every WBC test rests on); -J_ee' f_e is folded into
nle here.  Solve: the dense saddle system [[M/h, -Jc'], [Jc, 0]] [v+; F] = [M v / h + S' tau - nle; 0] by numpy.linalg.solve, refined in numpy.longdouble until the
correction is below 1e-18 relative.  Integration and the output record are written here on their own; the end-effector slots come from tests/urdf_model.fk.

Tolerance rule (accuracy of v+, q+, F, tau_applied: relative inf-norm per instance against the refined solution): 10 max(e_np, e_in, floor), from the reference alone --
    e_np   the plain fp64 numpy solve against its refinement;
    e_in   the spread of the refined solution when M, nle, Jc are perturbed by 4 eps relative (seeded, five draws): a kernel that forms these terms in its own
           summation order is such a perturbation;
    floor  the rounding of ONE fp64 evaluation of the defining identities at the solution (as dual_reference.rounding_floor): the momentum row is a TERMS-term sum,
           |d v+| <= TERMS eps h |M^-1| sum|terms|, |d F| <= 2 TERMS eps |Jc'^+| sum|terms|; q+ = q + h v+ and the joint law are three-term sums;
    10     the factor the value-function and dual tests grant a solve.
"""
import numpy as np

import lq_reference as LR
import support as S
import urdf_model as UM

EPS = np.finfo(np.float64).eps
LD = np.longdouble
FACTOR = 10.0
TERMS = 24 + 24 + 1 + 1 + 12     # M v+ / h, M v / h, nle, tau, Jc' F
FAILED, PULL, FRICTION = 1, 2, 4
KEYS = ("v", "q", "F", "tau")
FOOT_LINKS = [f"{leg}_FOOT" for leg in UM.FEET]


def coordinates(rbd):
    """(q, v) = ([p, zyx, q_j], d/dt of it) of an rbd state: the map WbcBase::updateMeasured applies (WbcBase.cpp:150-156)"""
    q = np.r_[rbd[3:6], rbd[0:3], rbd[6:24]]
    sz, cz, sy, cy = np.sin(q[3]), np.cos(q[3]), np.sin(q[4]), np.cos(q[4])
    wx, wy, wz = rbd[24:27]
    tmp = cz * wx / cy + sz * wy / cy
    v = np.r_[rbd[27:30], sy * tmp + wz, -sz * wx + cz * wy, tmp, rbd[30:48]]
    return q, v


def euler_rates_to_omega(zyx, de):
    sz, cz, sy, cy = np.sin(zyx[0]), np.cos(zyx[0]), np.sin(zyx[1]), np.cos(zyx[1])
    T = np.array([[0.0, -sz, cy * cz], [0.0, cz, cy * sz], [1.0, 0.0, -sy]])
    return T @ de


def state_record(q, v):
    """rbd[55] of (q, v): the inverse of coordinates(), the end-effector slots from the URDF's own forward kinematics at q"""
    r = np.zeros(55)
    r[0:3] = q[3:6]; r[3:6] = q[0:3]; r[6:24] = q[6:24]
    r[24:27] = euler_rates_to_omega(q[3:6], v[3:6]); r[27:30] = v[0:3]; r[30:48] = v[6:24]
    pose = UM.fk(q)
    r[48:51] = pose[UM.EE_LINK][1].real
    r[51:55] = np.real(LR.quaternion_of(pose[UM.EE_LINK][0].real[None])).reshape(4)
    return r


def contact_rows(mode):
    """rows of the feet Jacobian [12][24] of the feet in contact by `mode`, in foot order"""
    return [3 * c + a for c in range(4) if S.contact_flags(mode)[c] for a in range(3)]


def effort_limits(problem):
    lim = np.array(problem.model.effort_limit[:])
    return np.r_[np.tile(lim[:3], 4), lim[12:18]]


def joint_law(q, v, tau_ff, pos_des=None, vel_des=None, kp=None, kd=None, limits=None):
    """tau_j = kp_j (pos_des_j - q_j) + kd_j (vel_des_j - v_j) + tau_ff_j (the hybrid joint command law), clamped to +-limits if given; and sum|terms|"""
    z = np.zeros(18)
    pos_des, vel_des, kp, kd = (z if a is None else np.asarray(a, float) for a in (pos_des, vel_des, kp, kd))
    a, b = kp * (pos_des - q[6:]), kd * (vel_des - v[6:])
    tau = a + b + tau_ff
    mag = np.abs(kp) * (np.abs(pos_des) + np.abs(q[6:])) + np.abs(kd) * (np.abs(vel_des) + np.abs(v[6:])) + np.abs(tau_ff)
    if limits is not None:
        tau = np.clip(tau, -limits, limits)
    return tau, mag


def model_terms(orc, rbd, ee_force=None):
    """(M, nle, Jf) at rbd from the oracle's WBC model update, with -J_ee' f_e folded into nle"""
    q, _ = coordinates(rbd)
    x_des = np.r_[np.zeros(6), q]
    o = orc.wbc_model(x_des, np.zeros(30), np.ascontiguousarray(rbd, dtype=np.float64), 1.0, np.zeros(30))
    nle = o["nle"].copy()
    if ee_force is not None:
        nle = nle - o["armJ"][:3].T @ np.asarray(ee_force, float)
    return o["M"].copy(), nle, o["J"].copy()


def saddle_solve(M, nle, Jc, v, tau, h):
    """v+, F of  M (v+ - v) / h + nle = S' tau + Jc' F,  Jc v+ = 0: dict(v, F) refined, plain (the fp64 solve alone), iterations, correction (the last one, relative)"""
    n, m = 24, Jc.shape[0]
    K = np.zeros((n + m, n + m)); K[:n, :n] = M / h; K[:n, n:] = -Jc.T; K[n:, :n] = Jc
    Kl = np.zeros((n + m, n + m), dtype=LD); Kl[:n, :n] = M.astype(LD) / LD(h); Kl[:n, n:] = -Jc.T.astype(LD); Kl[n:, :n] = Jc.astype(LD)
    bl = np.zeros(n + m, dtype=LD)
    bl[:n] = (M.astype(LD) @ v.astype(LD)) / LD(h) - nle.astype(LD); bl[6:n] += tau.astype(LD)
    b = bl.astype(np.float64)
    x0 = np.linalg.solve(K, b)
    x = x0.astype(LD)
    corr, it = np.inf, 0
    while corr > 1e-18 and it < 40:
        dx = np.linalg.solve(K, (bl - Kl @ x).astype(np.float64))
        x = x + dx.astype(LD)
        corr = float(np.abs(dx).max() / max(float(np.abs(x).max()), 1e-300))
        it += 1
    return dict(v=x[:n].astype(np.float64), F=x[n:].astype(np.float64), plain=dict(v=x0[:n], F=x0[n:]), iterations=it, correction=corr, residual=(Kl, bl, x))


def pivots_fail(M, Jc):
    """the reference's own verdict on the two factorisations: M = L L' and G = Jc M^-1 Jc' = L L'"""
    try:
        L = np.linalg.cholesky(M)
        if Jc.shape[0]:
            Y = np.linalg.solve(L, Jc.T)
            np.linalg.cholesky(Y.T @ Y)
    except np.linalg.LinAlgError:
        return True
    return False


def substep(M, nle, Jf, q, v, tau, mode, h, mu):
    rows = contact_rows(mode)
    Jc = Jf[rows]
    if pivots_fail(M, Jc):
        return None
    sol = saddle_solve(M, nle, Jc, v, tau, h)
    if not (np.isfinite(sol["v"]).all() and np.isfinite(sol["F"]).all()):
        return None
    out = dict(v=sol["v"], q=q + h * sol["v"], F=sol["F"], tau=tau, Jc=Jc, sol=sol)
    out["plain"] = dict(v=sol["plain"]["v"], q=q + h * sol["plain"]["v"], F=sol["plain"]["F"], tau=tau)
    bits = 0
    for k in range(len(rows) // 3):
        fx, fy, fz = sol["F"][3 * k: 3 * k + 3]
        bits |= PULL if fz < 0 else 0
        bits |= FRICTION if (abs(fx) > mu * fz or abs(fy) > mu * fz) else 0
    out["bits"] = bits
    return out


def floors(M, nle, Jc, q, v, st, tau_mag, h):
    """the rounding floor of each of KEYS, relative to the inf-norm of the quantity (module docstring)"""
    terms = (np.abs(M) @ (np.abs(st["v"]) + np.abs(v))) / h + np.abs(nle) + np.r_[np.zeros(6), np.abs(st["tau"])] + np.abs(Jc).T @ np.abs(st["F"])
    rel = lambda err, x: float(np.max(err) / max(float(np.abs(x).max()), 1e-300)) if np.size(x) else 0.0  # noqa: E731
    dv = TERMS * EPS * h * (np.abs(np.linalg.inv(M)) @ terms)
    dF = 2 * TERMS * EPS * (np.abs(np.linalg.pinv(Jc.T)) @ terms) if Jc.shape[0] else np.zeros(0)
    dq = 3 * EPS * (np.abs(q) + h * np.abs(st["v"])) + h * dv
    return dict(v=rel(dv, st["v"]), F=rel(dF, st["F"]), q=rel(dq, st["q"]), tau=rel(4 * EPS * tau_mag, st["tau"]))


def rel_err(got, ref):
    ref = np.asarray(ref, float)
    if ref.size == 0:
        return 0.0
    return float(np.abs(np.asarray(got, float) - ref).max() / max(float(np.abs(ref).max()), 1e-300))


def step(orc, problem, rbd, tau_ff, mode, dt, substeps=1, clamp_effort=False, pos_des=None, vel_des=None, kp=None, kd=None, ee_force=None, bounds=True, draws=5, seed=0):
    """One call of the plant step for one instance.  Returns dict(rbd_next, contact_force [12], tau_applied, status, q, v, F, tau) and, with bounds, `bound`: per key of
    KEYS 10 max(e_np, e_in, floor) accumulated (summed) over the substeps, with its parts in `parts`."""
    rbd = np.asarray(rbd, float)
    mu = problem.settings.wbc_friction_coefficient
    limits = effort_limits(problem) if clamp_effort else None
    h = dt / substeps
    q, v = coordinates(rbd)
    status = 0
    parts = {k: dict(e_np=0.0, e_in=0.0, floor=0.0) for k in KEYS}
    rng = np.random.default_rng(seed)
    st = None
    for _ in range(substeps):
        tau, tau_mag = joint_law(q, v, tau_ff, pos_des, vel_des, kp, kd, limits)
        M, nle, Jf = model_terms(orc, state_record_light(q, v), ee_force)
        st = substep(M, nle, Jf, q, v, tau, mode, h, mu) if np.isfinite(tau).all() else None
        if st is None:
            return dict(rbd_next=rbd.copy(), contact_force=np.zeros(12), tau_applied=np.zeros(18), status=status | FAILED, bound=None)
        status |= st["bits"]
        if bounds:
            fl = floors(M, nle, st["Jc"], q, v, st, tau_mag, h)
            spread = {k: 0.0 for k in KEYS}
            for _d in range(draws):
                pert = lambda a: a * (1.0 + 4 * EPS * rng.uniform(-1, 1, a.shape))  # noqa: E731
                p = substep(pert(M), pert(nle), pert(Jf), q, v, tau, mode, h, mu)
                for k in KEYS:
                    spread[k] = max(spread[k], rel_err(p[k], st[k]))
            for k in KEYS:
                parts[k]["e_np"] += rel_err(st["plain"][k], st[k]); parts[k]["e_in"] += spread[k]; parts[k]["floor"] += fl[k]
        q, v = coordinates(state_record_light(st["q"], st["v"]))      # through the rbd form, as between calls
    force = np.zeros(12)
    force[contact_rows(mode)] = st["F"]
    out = dict(rbd_next=state_record(st["q"], st["v"]), contact_force=force, tau_applied=st["tau"], status=status, q=q, v=v, F=st["F"], tau=st["tau"], last=st)
    out["parts"] = parts
    out["bound"] = {k: FACTOR * max(parts[k].values()) for k in KEYS} if bounds else None
    return out


def state_record_light(q, v):
    """rbd[55] of (q, v) without the end-effector slots (the model update does not read them)"""
    r = np.zeros(55)
    r[0:3] = q[3:6]; r[3:6] = q[0:3]; r[6:24] = q[6:24]
    r[24:27] = euler_rates_to_omega(q[3:6], v[3:6]); r[27:30] = v[0:3]; r[30:48] = v[6:24]; r[54] = 1.0
    return r


def errors(got_rbd, got_force, got_tau, mode, ref):
    """relative inf-norm errors per key of KEYS of a kernel's outputs against step()'s"""
    q, v = coordinates(got_rbd)
    return dict(v=rel_err(v, ref["v"]), q=rel_err(q, ref["q"]), F=rel_err(np.asarray(got_force)[contact_rows(mode)], ref["F"]), tau=rel_err(got_tau, ref["tau"]))


def foot_velocities(q, v, step_size=1e-30):
    """[4][3] world velocities of the feet at (q, v): the complex-step directional derivative of the URDF's own forward kinematics along v"""
    pose = UM.fk(np.asarray(q, dtype=complex) + 1j * step_size * np.asarray(v, float))
    return np.stack([pose[f][1].imag / step_size for f in FOOT_LINKS])


def foot_velocity_magnitude(q, v, step_size=1e-30):
    """sum over the coordinates of |d p_foot / d q_k| |v_k| per foot and axis: the magnitude of the terms of foot_velocities (for C eps sum|terms| bounds)"""
    mag = np.zeros((4, 3))
    for k in range(24):
        e = np.zeros(24, dtype=complex); e[k] = 1j * step_size
        pose = UM.fk(np.asarray(q, dtype=complex) + e)
        mag += np.abs(np.stack([pose[f][1].imag / step_size for f in FOOT_LINKS])) * abs(v[k])
    return mag
