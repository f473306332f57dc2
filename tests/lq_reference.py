"""A live, numpy-only reference for the LQ blocks of ONE shooting node: A, B, b, C, D, e, Q, R, q, r and nc, derived a third time.

The kernels (ad_node_kernel + lq_node_kernel) and the oracle (oracle/qmo_mpc.h::nodeLQ) were written by the same hands; this module shares no code with either.
It imports neither support.Oracle nor anything under oracle/ nor a kernel-derived helper, and it never reads problem.model: the robot comes from its own URDF
parse (tests/urdf_model.py, the geometry model_independent.npz is built on).  From the product it takes only the VALUES of interface.problem.settings (weights,
barrier constants, gains, swing parameters, dt, bounds; the loader is pinned by test_host_config.py).

Rule of construction: VALUES are written from the formulation, DERIVATIVES are never written by hand.  Every Jacobian is the complex step (h = 1e-30) of a
holomorphic numpy value function, all 60 directions of a node in one vectorised pass (a (61, 60) complex batch of [x; u]).  Complex steps cannot be nested, so
the momentum map A_G(q), the foot velocities and the EE pose come from twists propagated along the kinematic tree: a value computation, holomorphic in q.
The three second-order scalars the formulation needs (p'' of the relaxed barrier, the Hessian of the friction cone) are complex steps of the first-order
formulas, and those first-order formulas are themselves checked against the complex step of the values (test_lq_reference.py).

What each piece restates (the reference tree's files):
  flow map      f = [sum f_c / m + g ; sum (p_c - com) x f_c / m ; A_b^-1 (m h - A_j v_j) ; v_j]      qm_interface/src/dynamics/QMDynamicsAD.cpp:22-33
                Euler ZYX, state and input layout of SURVEY.md Appendix A
  RK2 map       x+ = x + dt/2 (k1 + f(x + dt k1, u)); A, B = its complex-step Jacobian (= upstream's rk2SensitivityDiscretization); b = x+ - x_next
  equality rows insertion order of QMInterface.cpp:116-131: zero force on swing feet, zero velocity on stance feet with positionErrorGain on z
                (QMInterface.cpp:324-339), the normal-velocity row on swing feet (constraint/NormalVelocityConstraintCppAd.cpp:37-66, QMPreComputation.cpp:50-89)
  swing z       lift-off / touch-down from the mode schedule, cubic Hermite through the mid height (task.info swing block)
  node mode     a node ON an event time takes the mode that starts there
  cost          tracking 1/2 dx'Q dx + 1/2 du'R'du, R' with the J^T R_task J leg block (QMInterface.cpp:274-299), u_nom = weight compensation
  EE pose       soft constraint, Gauss-Newton; position error and quaternionDistance; reference by lerp and Eigen's slerp from the left knot
                (constraint/EndEffectorConstraint.cpp:36-113); rotation -> quaternion with Eigen's branches (trace <= 0 included)
  barriers      relaxed log barriers on arm joint position and velocity with the constant offset (QMInterface.cpp:177-259)
  friction cone R += p''(h) g g' + p'(h) (hess h - shift I) (QMInterface.cpp:327-358)
  everything scaled by dt; terminal node: EE term with the final weights only, nc = 0.
Left out on purpose: force tracking (ee_contact_ref = NULL), the project's own formulation."""
import numpy as np

import urdf_model as UM

H = 1e-30
MASSIVE = [(name, L) for name, L in UM.LINKS.items() if L["m"] != 0.0]
MASS = sum(L["m"] for _, L in MASSIVE)
FOOT_LINKS = [f"{leg}_FOOT" for leg in UM.FEET]
_LIMITS = {jt["name"]: (jt["lower"], jt["upper"]) for jt in UM.JOINTS}
ARM_LOWER = np.array([_LIMITS[f"z1_joint_{i}"][0] for i in range(1, 7)])
ARM_UPPER = np.array([_LIMITS[f"z1_joint_{i}"][1] for i in range(1, 7)])
BLOCKS = ("A", "B", "b", "Q", "R", "q", "r", "C", "D", "e")
TERMINAL_BLOCKS = ("Q", "q")


def cross(a, b):
    """a x b on the last axis, without conjugation (complex step)"""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


# ------------------------------------------------------------------------------------------------ kinematics: poses and propagated twists
def twists(pose, q, V):
    """(angular velocity, velocity of the link origin) of every link, world axes, for the generalised velocities V [..., D, 24] at q [..., 24]:
    v = [dp_base, Euler ZYX rates (yaw, pitch, roll), joint rates].  Propagated from the base outwards: a child turns with its parent plus its own joint
    rate about the joint axis, and its origin rides on the parent."""
    Rz, Ry = UM.rot((0, 0, 1), q[..., 3]), UM.rot((0, 1, 0), q[..., 4])
    ez, ey, ex = np.array([0, 0, 1.0]), Rz @ np.array([0, 1.0, 0]), (Rz @ Ry) @ np.array([1.0, 0, 0])
    w0 = V[..., 3:4] * ez + V[..., 4:5] * ey[..., None, :] + V[..., 5:6] * ex[..., None, :]
    tw = {"base": (w0, V[..., 0:3])}
    stack = ["base"]
    while stack:
        parent = stack.pop()
        Rp, pp = pose[parent]
        wp, vp = tw[parent]
        for jt in UM.CHILDREN.get(parent, []):
            pc = pose[jt["child"]][1]
            vc = vp + cross(wp, (pc - pp)[..., None, :])
            wc = wp
            if jt["type"] == "revolute" and jt["name"] in UM.JOINT_ORDER:
                k = 6 + UM.JOINT_ORDER.index(jt["name"])
                wc = wp + V[..., k:k + 1] * (Rp @ jt["axis"])[..., None, :]
            tw[jt["child"]] = (wc, vc)
            stack.append(jt["child"])
    return tw


def centroidal(pose, tw):
    """(A_G [..., 6, D], com [..., 3]): the momentum about the total com, world axes, of each of the D velocity fields of tw"""
    com = sum(L["m"] * (pose[n][1] + pose[n][0] @ L["c"]) for n, L in MASSIVE) / MASS
    lin, ang = 0.0, 0.0
    for n, L in MASSIVE:
        R, p = pose[n]
        r = R @ L["c"]
        w, v = tw[n]
        vc = v + cross(w, r[..., None, :])
        Iw = R @ L["I"] @ np.swapaxes(R, -1, -2)
        lin = lin + L["m"] * vc
        ang = ang + cross((p + r - com)[..., None, :], L["m"] * vc) + np.einsum("...ij,...dj->...di", Iw, w)
    return np.swapaxes(np.concatenate([lin, ang], axis=-1), -1, -2), com


def kinematics(q):
    """everything the node needs of a configuration batch q [..., 24]: A_G, com, feet [..., 4, 3], foot Jacobians [..., 4, 24, 3], EE position and rotation"""
    q = np.asarray(q, dtype=complex)
    pose = UM.fk(q)
    tw = twists(pose, q, np.broadcast_to(np.eye(24, dtype=complex), q.shape[:-1] + (24, 24)))
    A, com = centroidal(pose, tw)
    feet = np.stack([pose[f][1] for f in FOOT_LINKS], axis=-2)
    Jfeet = np.stack([tw[f][1] for f in FOOT_LINKS], axis=-3)
    return dict(A=A, com=com, feet=feet, Jfeet=Jfeet, ee=pose[UM.EE_LINK][1], Ree=pose[UM.EE_LINK][0])


def flow(x, u, gravity):
    """centroidal flow map f(x, u) [..., 30] and the kinematic quantities of the evaluation (foot velocities included)"""
    k = kinematics(x[..., 6:30])
    vj = u[..., 12:30]
    rhs = MASS * x[..., 0:6] - np.einsum("...ij,...j->...i", k["A"][..., :, 6:], vj)
    vb = np.linalg.solve(k["A"][..., :, :6], rhs[..., None])[..., 0]
    F = u[..., :12].reshape(u.shape[:-1] + (4, 3))
    lin = F.sum(axis=-2) / MASS + np.array([0.0, 0.0, -gravity])
    ang = cross(k["feet"] - k["com"][..., None, :], F).sum(axis=-2) / MASS
    v = np.concatenate([vb, vj], axis=-1)
    k["footvel"] = np.einsum("...d,...cdk->...ck", v, k["Jfeet"])
    return np.concatenate([lin, ang, vb, vj], axis=-1), k


def rk2(x, u, dt, gravity):
    k1, kin = flow(x, u, gravity)
    k2, _ = flow(x + dt * k1, u, gravity)
    return x + 0.5 * dt * (k1 + k2), kin


# ------------------------------------------------------------------------------------------------ schedule, swing reference, targets
def contact_flags(mode):
    """stance flag of (LF, RF, LH, RH): mode = 8 LF + 4 RF + 2 LH + RH"""
    return [bool((int(mode) >> (3 - c)) & 1) for c in range(4)]


def node_phase(events, t):
    """index of the schedule phase of a shooting node at t: a node ON an event time belongs to the phase that starts there"""
    return int(np.sum(np.asarray(events) <= t))


def node_mode(events, modes, t):
    return int(modes[node_phase(events, t)])


def hermite(t0, p0, v0, t1, p1, v1, t):
    T = t1 - t0
    s = (t - t0) / T
    return (2 * s**3 - 3 * s**2 + 1) * p0 + (s**3 - 2 * s**2 + s) * T * v0 + (-2 * s**3 + 3 * s**2) * p1 + (s**3 - s**2) * T * v1


def swing_z(P, events, modes, leg, t):
    """height reference of swing foot `leg` at t (t may carry a complex step: the velocity reference is its derivative).  Flat terrain at height 0.
    Where the schedule does not hold the lift-off or the touch-down (upstream throws), the swing is extended by touchdownAfterHorizon beyond the first /
    last event: the project's stated choice (oracle/qmo_mpc.h swingReference), followed here so that all sixteen modes can be held over a horizon."""
    events = np.asarray(events, float)
    ph = node_phase(events, np.real(t))
    stance = [contact_flags(m)[leg] for m in modes]
    assert not stance[ph]
    before = [i for i in range(ph) if stance[i]]
    after = [i for i in range(ph + 1, len(modes)) if stance[i]]
    lift = events[before[-1]] if before else (events[0] if len(events) else np.real(t)) - P.touchdown_after_horizon
    touch = events[after[0] - 1] if after else (events[-1] if len(events) else np.real(t)) + P.touchdown_after_horizon
    scale = min(1.0, (touch - lift) / P.swing_time_scale)
    mid, top = 0.5 * (lift + touch), scale * P.swing_height
    if np.real(t) < mid:
        return hermite(lift, 0.0, scale * P.liftoff_velocity, mid, top, 0.0, t)
    return hermite(mid, top, 0.0, touch, 0.0, scale * P.touchdown_velocity, t)


def swing_reference(P, events, modes, leg, t):
    """(z, dz/dt) of the swing reference"""
    z = swing_z(P, events, modes, leg, t + 1j * H)
    return z.real, z.imag / H


def time_segment(times, t):
    """(index of the left knot, weight of the LEFT knot) of linear interpolation; clamped outside the knots"""
    K = len(times)
    if K == 1 or t <= times[0]:
        return 0, 1.0
    if t > times[-1]:
        return K - 2, 0.0
    i = int(np.searchsorted(times, t, side="left")) - 1
    return i, (times[i + 1] - t) / (times[i + 1] - times[i])


def slerp(a, b, s):
    """Eigen's QuaternionBase::slerp(s, b) from a; (x, y, z, w)"""
    d = float(a @ b)
    if abs(d) >= 1.0 - np.finfo(float).eps:
        s0, s1 = 1.0 - s, s
    else:
        th = np.arccos(abs(d))
        s0, s1 = np.sin((1.0 - s) * th) / np.sin(th), np.sin(s * th) / np.sin(th)
    return s0 * a + (-s1 if d < 0 else s1) * b


def references(ttimes, tstates, t):
    """(x_ref [30], EE position [3], EE quaternion [4]) at t"""
    ttimes, tstates = np.asarray(ttimes, float), np.asarray(tstates, float)
    if len(ttimes) == 1:
        return tstates[0, :30], tstates[0, 30:33], tstates[0, 33:37]
    i, al = time_segment(ttimes, t)
    lhs, rhs = tstates[i], tstates[i + 1]
    return al * lhs[:30] + (1 - al) * rhs[:30], al * lhs[30:33] + (1 - al) * rhs[30:33], slerp(lhs[33:37], rhs[33:37], 1 - al)


# ------------------------------------------------------------------------------------------------ end-effector error
def quaternion_of(R):
    """Eigen's Quaternion(Matrix3) for a batch R [..., 3, 3] of rotations a complex step apart (the branch is that of the unperturbed one); (x, y, z, w)"""
    R0 = R.reshape(-1, 3, 3)[0].real
    qt = [None] * 4
    if R0[0, 0] + R0[1, 1] + R0[2, 2] > 0:
        s = np.sqrt(R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] + 1.0)
        qt[3] = 0.5 * s
        s = 0.5 / s
        qt[0], qt[1], qt[2] = (R[..., 2, 1] - R[..., 1, 2]) * s, (R[..., 0, 2] - R[..., 2, 0]) * s, (R[..., 1, 0] - R[..., 0, 1]) * s
    else:
        i = 1 if R0[1, 1] > R0[0, 0] else 0
        i = 2 if R0[2, 2] > R0[i, i] else i
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[..., i, i] - R[..., j, j] - R[..., k, k] + 1.0)
        qt[i] = 0.5 * s
        s = 0.5 / s
        qt[3], qt[j], qt[k] = (R[..., k, j] - R[..., j, k]) * s, (R[..., j, i] + R[..., i, j]) * s, (R[..., k, i] + R[..., i, k]) * s
    return np.stack(qt, axis=-1)


def quaternion_distance(qm, qr):
    """upstream's quaternionDistance(q, q_ref) = w q_ref.v - w_ref q.v + q.v x q_ref.v"""
    return qm[..., 3:4] * qr[:3] - qr[3] * qm[..., :3] + cross(qm[..., :3], np.broadcast_to(qr[:3].astype(complex), qm[..., :3].shape))


def ee_error(kin, pos_ref, quat_ref):
    return np.concatenate([kin["ee"] - pos_ref, quaternion_distance(quaternion_of(kin["Ree"]), quat_ref)], axis=-1)


# ------------------------------------------------------------------------------------------------ penalties
def barrier(mu, delta, h):
    """RelaxedBarrierPenalty: -mu ln h above delta, the quadratic extension below (value and slope continuous at delta)"""
    return -mu * np.log(h) if np.real(h) > delta else mu * (-np.log(delta) + 0.5 * ((h - 2 * delta) / delta) ** 2 - 0.5)


def barrier_slope(mu, delta, h):
    return -mu / h if np.real(h) > delta else mu * (h - 2 * delta) / delta**2


def barrier_curvature(mu, delta, h):
    return np.imag(barrier_slope(mu, delta, h + 1j * H)) / H


def cone(P, f):
    """friction cone h(f) = mu f_z - sqrt(f_x^2 + f_y^2 + regularisation)"""
    return P.friction_coefficient * f[2] - np.sqrt(f[0] ** 2 + f[1] ** 2 + P.friction_regularization)


def cone_gradient(P, f):
    F = np.sqrt(f[0] ** 2 + f[1] ** 2 + P.friction_regularization)
    return np.array([-f[0] / F, -f[1] / F, P.friction_coefficient + 0 * F])


def cone_hessian(P, f):
    f = np.asarray(f, dtype=complex)
    return np.stack([np.imag(cone_gradient(P, f + 1j * H * np.eye(3)[a])) / H for a in range(3)], axis=1)


# ------------------------------------------------------------------------------------------------ settings
class Params:
    """the values of interface.problem.settings this reference uses, and what is derived once from them (the input weight R')"""
    SCALARS = ("dt", "gravity", "position_error_gain", "liftoff_velocity", "touchdown_velocity", "swing_height", "touchdown_after_horizon", "swing_time_scale",
               "ee_mu_position", "ee_mu_orientation", "ee_final_mu_position", "ee_final_mu_orientation", "friction_coefficient", "friction_barrier_mu",
               "friction_barrier_delta", "friction_regularization", "friction_hessian_shift", "joint_pos_barrier_mu", "joint_pos_barrier_delta", "joint_vel_barrier_mu",
               "joint_vel_barrier_delta")

    def __init__(self, settings):
        for name in self.SCALARS:
            setattr(self, name, float(getattr(settings, name)))
        self.Q = np.array(settings.Q[:]).reshape(30, 30)
        self.R_task = np.array(settings.R_task[:]).reshape(30, 30)
        self.initial_state = np.array(settings.initial_state[:])
        self.arm_vel_lower, self.arm_vel_upper = np.array(settings.arm_vel_lower[:]), np.array(settings.arm_vel_upper[:])
        self.R = input_weight(self)


def input_weight(P):
    """R' (QMInterface.cpp:274-299): the leg joint-rate block of R_task seen through the feet Jacobian (contact order) w.r.t. the 12 leg joints at the initial state"""
    q = P.initial_state[6:30] + 1j * H * np.eye(24)[6:18]
    pose = UM.fk(q)
    J = np.concatenate([pose[f][1].imag.T / H for f in FOOT_LINKS], axis=0)
    R = P.R_task.copy()
    R[12:24, 12:24] = J.T @ P.R_task[12:24, 12:24] @ J
    return R


def nominal_input(P, mode):
    fl = contact_flags(mode)
    u = np.zeros(30)
    for c in range(4):
        if fl[c]:
            u[3 * c + 2] = MASS * P.gravity / sum(fl)
    return u


# ------------------------------------------------------------------------------------------------ one node
def _jac(values):
    """values [61, m] of a pass over [z0; z0 + i h e_k]: (value [m], Jacobian [m, 60])"""
    return values[0].real, values[1:].imag.T / H


def lq_node(P, t, dt, x, u, xnext, terminal, events, modes, ttimes, tstates):
    """The LQ blocks of the node at time t, step dt, iterate (x, u), next state xnext; events / modes: the mode schedule (modes has one entry more);
    ttimes [K], tstates [K][37]: the target knots.  Returns A B b Q R q r C D e nc and the node's cost as the oracle's and the kernels' dumps name them."""
    x = np.asarray(x, float)
    u = np.zeros(30) if terminal else np.asarray(u, float)
    xref, ee_pos, ee_quat = references(ttimes, tstates, t)
    Z = np.concatenate([x, u])[None, :] + 1j * H * np.vstack([np.zeros(60), np.eye(60)])
    X, U = Z[:, :30], Z[:, 30:]
    o = {}
    if terminal:
        kin = kinematics(X[:, 6:30])
        hv, hJ = _jac(ee_error(kin, ee_pos, ee_quat))
        mu = np.r_[np.full(3, P.ee_final_mu_position), np.full(3, P.ee_final_mu_orientation)]
        Jx = hJ[:, :30]
        return dict(Q=Jx.T @ (mu[:, None] * Jx), q=Jx.T @ (mu * hv), nc=0, cost=0.5 * float(mu @ hv**2))
    mode = node_mode(events, modes, t)
    fl = contact_flags(mode)
    xp, kin = rk2(X, U, dt, P.gravity)
    # ---- dynamics
    xv, xJ = _jac(xp)
    o["A"], o["B"], o["b"] = xJ[:, :30], xJ[:, 30:], xv - np.asarray(xnext, float)
    # ---- equality rows
    rows = []
    for c in range(4):
        if not fl[c]:
            rows += [U[:, 3 * c + a] for a in range(3)]
        else:
            rows += [kin["footvel"][:, c, 0], kin["footvel"][:, c, 1], kin["footvel"][:, c, 2] + P.position_error_gain * kin["feet"][:, c, 2]]
        if not fl[c]:
            zp, zv = swing_reference(P, events, modes, c, t)
            rows.append(kin["footvel"][:, c, 2] - zv + P.position_error_gain * (kin["feet"][:, c, 2] - zp))
    ev_, eJ = _jac(np.stack(rows, axis=1))
    o["C"], o["D"], o["e"], o["nc"] = eJ[:, :30], eJ[:, 30:], ev_, len(rows)
    # ---- cost: tracking
    dx, du = x - xref, u - nominal_input(P, mode)
    Q, R = P.Q.copy(), P.R.copy()
    q, r = P.Q @ dx, P.R @ du
    cost = 0.5 * dx @ P.Q @ dx + 0.5 * du @ P.R @ du
    # ---- EE pose, Gauss-Newton
    hv, hJ = _jac(ee_error(kin, ee_pos, ee_quat))
    mu = np.r_[np.full(3, P.ee_mu_position), np.full(3, P.ee_mu_orientation)]
    Jx = hJ[:, :30]
    assert np.abs(hJ[:, 30:]).max() == 0.0
    Q += Jx.T @ (mu[:, None] * Jx); q += Jx.T @ (mu * hv); cost += 0.5 * float(mu @ hv**2)
    # ---- arm joint position / velocity boxes: two one-sided relaxed barriers each, offset = their value at x = 0, u = 0
    for i in range(6):
        for (m_, d_, val, lo, up, grad, hess, k) in ((P.joint_pos_barrier_mu, P.joint_pos_barrier_delta, x[24 + i], ARM_LOWER[i], ARM_UPPER[i], q, Q, 24 + i),
                                                    (P.joint_vel_barrier_mu, P.joint_vel_barrier_delta, u[24 + i], P.arm_vel_lower[i], P.arm_vel_upper[i], r, R, 24 + i)):
            cost += barrier(m_, d_, val - lo) + barrier(m_, d_, up - val) - barrier(m_, d_, 0.0 - lo) - barrier(m_, d_, up - 0.0)
            grad[k] += barrier_slope(m_, d_, val - lo) - barrier_slope(m_, d_, up - val)
            hess[k, k] += barrier_curvature(m_, d_, val - lo) + barrier_curvature(m_, d_, up - val)
    # ---- friction cone on the stance feet
    for c in range(4):
        if fl[c]:
            f = u[3 * c:3 * c + 3]
            h = cone(P, f)
            g = np.array([np.imag(cone(P, f + 1j * H * np.eye(3)[a])) / H for a in range(3)])
            p1, p2 = barrier_slope(P.friction_barrier_mu, P.friction_barrier_delta, h), barrier_curvature(P.friction_barrier_mu, P.friction_barrier_delta, h)
            cost += barrier(P.friction_barrier_mu, P.friction_barrier_delta, h)
            r[3 * c:3 * c + 3] += p1 * g
            R[3 * c:3 * c + 3, 3 * c:3 * c + 3] += p2 * np.outer(g, g) + p1 * (cone_hessian(P, f) - P.friction_hessian_shift * np.eye(3))
    o.update(Q=dt * Q, R=dt * R, q=dt * q, r=dt * r, cost=dt * float(cost))
    return o


def deviations(got, ref, terminal):
    """per block |got - ref|_inf / max(1, |ref|_inf): the scale of the project's LQ-block bar"""
    return {k: float(np.abs(got[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())) for k in (TERMINAL_BLOCKS if terminal else BLOCKS)}
