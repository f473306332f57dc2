"""CPU tier of the LQ-block pin: the numpy reference of one shooting node (lq_reference.py) against the independent model fixture, against itself in 50 digits,
and then the oracle and the host-emulated kernels against it over the scenarios of lq_scenarios.py, under the project's LQ-block bar."""
import time

import mpmath as mp
import numpy as np
import pytest

import lq_reference as LR
import lq_scenarios as LS
import support as S
from qm_door_amd import abi, api

GOLDEN = S.os.path.join(S.ROOT, "tests", "golden", "model_independent.npz")


# ------------------------------------------------------------------------------------------------ 1. the propagated twists against complex-step FK
def test_propagated_twists_against_the_independent_model_fixture():
    """A_G, com, feet and EE position of the reference against model_independent.npz (made by complex-step forward kinematics) at its three configurations."""
    fx = np.load(GOLDEN)
    assert abs(LR.MASS - float(fx["total_mass"])) <= 1e-12
    for i in range(3):
        k = LR.kinematics(fx["q"][i])
        for got, ref in ((k["A"], fx["AG"][i]), (k["com"], fx["com"][i]), (k["feet"], fx["feet"][i]), (k["ee"], fx["ee"][i])):
            assert np.abs(got.imag).max() == 0.0 and np.abs(got.real - ref).max() <= 1e-12


def test_first_order_formulas_are_the_complex_step_of_their_values(interface):
    """the two first-order formulas the reference writes out (barrier slope, cone gradient) -- whose complex steps are its only second derivatives"""
    P = LS.params(interface)
    for h in (-0.3, 0.0, 4e-4, 0.999e-3, 1.001e-3, 0.02, 7.0):
        for mu, delta in ((P.joint_pos_barrier_mu, P.joint_pos_barrier_delta), (P.friction_barrier_mu, P.friction_barrier_delta)):
            cs = np.imag(LR.barrier(mu, delta, h + 1j * LR.H)) / LR.H
            assert abs(LR.barrier_slope(mu, delta, h) - cs) <= 1e-14 * abs(cs)
    for f in ([4.0, -1.0, 3.0], [0.0, 0.0, 60.0], [-12.0, 7.0, -6.0]):
        f = np.array(f)
        cs = np.array([np.imag(LR.cone(P, f + 1j * LR.H * np.eye(3)[a])) / LR.H for a in range(3)])
        assert np.abs(LR.cone_gradient(P, f) - cs).max() <= 1e-15


# ------------------------------------------------------------------------------------------------ 2. the reference against itself in 50 digits
class MpModel:
    """The value functions of lq_reference restated on mpmath numbers (object arrays), one configuration at a time: poses, propagated twists, momentum map,
    flow map, RK2 map, equality rows, EE error, stage cost pieces.  Derivatives: central differences with step 1e-20 in 50-digit arithmetic.
    NOT restated but taken from lq_reference: swing_z, references (lerp / slerp), node_mode, nominal_input, the input weight P.R."""
    STEP = mp.mpf(10) ** -20

    def __init__(self, P):
        self.P = P
        self.links = {n: dict(m=mp.mpf(L["m"]), c=self.vec(L["c"]), I=self.mat(L["I"])) for n, L in LR.UM.LINKS.items()}
        self.mass = sum(L["m"] for L in self.links.values())

    @staticmethod
    def vec(a):
        return np.array([mp.mpf(float(v)) for v in np.asarray(a).ravel()], dtype=object).reshape(np.shape(a))

    mat = vec

    @staticmethod
    def rot(axis, a):
        x, y, z = (mp.mpf(float(v)) for v in axis)
        K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]], dtype=object)
        return np.array(mp.eye(3).tolist(), dtype=object) + mp.sin(a) * K + (1 - mp.cos(a)) * K.dot(K)

    def flow(self, x, u):
        UM = LR.UM
        q = x[6:30]
        Rz, Ry = self.rot((0, 0, 1), q[3]), self.rot((0, 1, 0), q[4])
        pose = {"base": (Rz.dot(Ry).dot(self.rot((1, 0, 0), q[5])), q[0:3])}
        # velocity fields: the six base directions and the joint rates of u as the seventh
        V = np.array([[mp.mpf(int(d == k)) for k in range(24)] for d in range(6)] + [[mp.mpf(0)] * 6 + list(u[12:30])], dtype=object)
        ez, ey, ex = self.vec([0, 0, 1]), Rz.dot(self.vec([0, 1, 0])), Rz.dot(Ry).dot(self.vec([1, 0, 0]))
        tw = {"base": (np.array([V[d, 3] * ez + V[d, 4] * ey + V[d, 5] * ex for d in range(7)], dtype=object), V[:, 0:3])}
        stack = ["base"]
        while stack:
            par = stack.pop()
            Rp, pp = pose[par]
            wp, vp = tw[par]
            for jt in UM.CHILDREN.get(par, []):
                on = jt["type"] == "revolute" and jt["name"] in UM.JOINT_ORDER
                k = 6 + UM.JOINT_ORDER.index(jt["name"]) if on else None
                Rc = Rp.dot(self.rot(jt["axis"], q[k])) if on else Rp
                pc = pp + Rp.dot(self.vec(jt["xyz"]))
                vc = np.array([vp[d] + np.cross(wp[d], pc - pp) for d in range(7)], dtype=object)
                wc = np.array([wp[d] + V[d, k] * Rp.dot(self.vec(jt["axis"])) for d in range(7)], dtype=object) if on else wp
                pose[jt["child"]], tw[jt["child"]] = (Rc, pc), (wc, vc)
                stack.append(jt["child"])
        massive = [(n, L) for n, L in self.links.items() if L["m"] != 0]
        com = sum(L["m"] * (pose[n][1] + pose[n][0].dot(L["c"])) for n, L in massive) / self.mass
        Hm = np.zeros((6, 7), dtype=object)
        for n, L in massive:
            R, p = pose[n]
            r = R.dot(L["c"])
            Iw = R.dot(L["I"]).dot(R.T)
            for d in range(7):
                vc = tw[n][1][d] + np.cross(tw[n][0][d], r)
                Hm[:3, d] += L["m"] * vc
                Hm[3:, d] += np.cross(p + r - com, L["m"] * vc) + Iw.dot(tw[n][0][d])
        rhs = self.mass * x[0:6] - Hm[:, 6]
        vb = np.array(list(mp.lu_solve(mp.matrix(Hm[:, :6].tolist()), mp.matrix(list(rhs)))), dtype=object)
        feet = [pose[f][1] for f in LR.FOOT_LINKS]
        F = [u[3 * c:3 * c + 3] for c in range(4)]
        lin = sum(F) / self.mass + self.vec([0, 0, -self.P.gravity])
        ang = sum(np.cross(feet[c] - com, F[c]) for c in range(4)) / self.mass
        footvel = [sum(vb[d] * tw[f][1][d] for d in range(6)) + tw[f][1][6] for f in LR.FOOT_LINKS]
        kin = dict(feet=feet, footvel=footvel, ee=pose[UM.EE_LINK][1], Ree=pose[UM.EE_LINK][0])
        return np.concatenate([lin, ang, vb, u[12:30]]), kin

    def values(self, z, a):
        """every differentiated value of the node at z = [x; u]: x+ (30), equality rows (nc), EE error (6)"""
        x, u = z[:30], z[30:]
        k1, kin = self.flow(x, u)
        out = []
        if not a["terminal"]:
            dt = mp.mpf(float(a["dt"]))
            k2, _ = self.flow(x + dt * k1, u)
            out += list(x + dt / 2 * (k1 + k2))
            fl = LR.contact_flags(LR.node_mode(a["events"], a["modes"], a["t"]))
            g = mp.mpf(self.P.position_error_gain)
            for c in range(4):
                if not fl[c]:
                    out += list(u[3 * c:3 * c + 3])
                    zp, zv = self.swing(a, c)
                    out.append(kin["footvel"][c][2] - zv + g * (kin["feet"][c][2] - zp))
                else:
                    out += [kin["footvel"][c][0], kin["footvel"][c][1], kin["footvel"][c][2] + g * kin["feet"][c][2]]
        _, pr, qr = LR.references(a["ttimes"], a["tstates"], a["t"])
        R = kin["Ree"]
        Rf = np.array([[float(v) for v in row] for row in R])
        if np.trace(Rf) > 0:                                             # Eigen's branches, decided on the rounded rotation
            s = mp.sqrt(R[0, 0] + R[1, 1] + R[2, 2] + 1)
            qm = [(R[2, 1] - R[1, 2]) / (2 * s), (R[0, 2] - R[2, 0]) / (2 * s), (R[1, 0] - R[0, 1]) / (2 * s), s / 2]
        else:
            i = 1 if Rf[1, 1] > Rf[0, 0] else 0
            i = 2 if Rf[2, 2] > Rf[i, i] else i
            j, k = (i + 1) % 3, (i + 2) % 3
            s = mp.sqrt(R[i, i] - R[j, j] - R[k, k] + 1)
            qm = [None] * 4
            qm[i], qm[j], qm[k], qm[3] = s / 2, (R[j, i] + R[i, j]) / (2 * s), (R[k, i] + R[i, k]) / (2 * s), (R[k, j] - R[j, k]) / (2 * s)
        qv, rv = np.array(qm[:3], dtype=object), self.vec(qr[:3])
        out += list(kin["ee"] - self.vec(pr)) + list(qm[3] * rv - mp.mpf(float(qr[3])) * qv + np.cross(qv, rv))
        return np.array(out, dtype=object)

    def swing(self, a, leg):
        """swing reference in 50 digits: the Hermite cubic of lq_reference.swing_z on mpmath numbers, its time derivative by a central difference"""
        f = lambda t: LR.swing_z(_MpSettings(self.P), [mp.mpf(float(e)) for e in a["events"]], a["modes"], leg, t)  # noqa: E731
        t = mp.mpf(float(a["t"]))
        return f(t), (f(t + self.STEP) - f(t - self.STEP)) / (2 * self.STEP)

    def jacobian(self, z, a):
        v0 = self.values(z, a)
        J = np.zeros((len(v0), 60), dtype=object)
        for k in range(60):
            e = np.array([mp.mpf(0)] * 60, dtype=object); e[k] = self.STEP
            J[:, k] = (self.values(z + e, a) - self.values(z - e, a)) / (2 * self.STEP)
        return v0, J


class _MpSettings:
    """the swing parameters as mpmath numbers, for lq_reference.swing_z evaluated in 50 digits (np.real of an mpf is the mpf)"""
    def __init__(self, P):
        for n in ("touchdown_after_horizon", "swing_time_scale", "swing_height", "liftoff_velocity", "touchdown_velocity"):
            setattr(self, n, mp.mpf(getattr(P, n)))


def _mp_penalty(mu, delta, h):
    mu, delta = mp.mpf(mu), mp.mpf(delta)
    return -mu * mp.log(h) if h > delta else mu * (-mp.log(delta) + ((h - 2 * delta) / delta) ** 2 / 2 - mp.mpf(1) / 2)


def _mp_blocks(M, P, a):
    """the blocks of lq_reference.lq_node from the 50-digit values: first derivatives by central differences of the value functions, the Gauss-Newton terms from
    those, the barrier and cone terms from first and second central differences of the SCALAR stage cost pieces"""
    f = lambda v: np.array([[float(e) for e in row] for row in v]) if np.ndim(v) == 2 else np.array([float(e) for e in v])  # noqa: E731
    x = M.vec(a["x"]); u = M.vec(np.zeros(30) if a["terminal"] else a["u"])
    v0, J = M.jacobian(np.concatenate([x, u]), a)
    if a["terminal"]:
        mu = [mp.mpf(P.ee_final_mu_position)] * 3 + [mp.mpf(P.ee_final_mu_orientation)] * 3
        Jx = J[:, :30]
        return dict(Q=f(Jx.T.dot(np.diag(mu)).dot(Jx)), q=f(Jx.T.dot(np.array(mu, dtype=object) * v0)))
    dt = mp.mpf(float(a["dt"]))
    nc = len(v0) - 36
    o = dict(A=f(J[:30, :30]), B=f(J[:30, 30:]), b=f(v0[:30] - M.vec(a["xnext"])), C=f(J[30:30 + nc, :30]), D=f(J[30:30 + nc, 30:]), e=f(v0[30:30 + nc]))
    mode = LR.node_mode(a["events"], a["modes"], a["t"])
    xref = LR.references(a["ttimes"], a["tstates"], a["t"])[0]
    mu = [mp.mpf(P.ee_mu_position)] * 3 + [mp.mpf(P.ee_mu_orientation)] * 3
    Jx, h = J[30 + nc:, :30], v0[30 + nc:]

    def scalar(z):
        """the stage cost pieces that are exact in their second derivatives: tracking, barriers, friction cone (the cone WITHOUT the diagonal shift, added below)"""
        xx, uu = z[:30], z[30:]
        dx, du = xx - M.vec(xref), uu - M.vec(LR.nominal_input(P, mode))
        c = dx.dot(M.mat(P.Q)).dot(dx) / 2 + du.dot(M.mat(P.R)).dot(du) / 2
        for i in range(6):
            c += _mp_penalty(P.joint_pos_barrier_mu, P.joint_pos_barrier_delta, xx[24 + i] - mp.mpf(LR.ARM_LOWER[i])) + _mp_penalty(P.joint_pos_barrier_mu, P.joint_pos_barrier_delta, mp.mpf(LR.ARM_UPPER[i]) - xx[24 + i])
            c += _mp_penalty(P.joint_vel_barrier_mu, P.joint_vel_barrier_delta, uu[24 + i] - mp.mpf(P.arm_vel_lower[i])) + _mp_penalty(P.joint_vel_barrier_mu, P.joint_vel_barrier_delta, mp.mpf(P.arm_vel_upper[i]) - uu[24 + i])
        for cc in range(4):
            if LR.contact_flags(mode)[cc]:
                hh = mp.mpf(P.friction_coefficient) * uu[3 * cc + 2] - mp.sqrt(uu[3 * cc] ** 2 + uu[3 * cc + 1] ** 2 + mp.mpf(P.friction_regularization))
                c += _mp_penalty(P.friction_barrier_mu, P.friction_barrier_delta, hh)
        return c
    z = np.concatenate([x, u])
    st = mp.mpf(10) ** -15
    E = np.array(mp.eye(60).tolist(), dtype=object) * st
    cp, cm = [scalar(z + E[k]) for k in range(60)], [scalar(z - E[k]) for k in range(60)]
    g = np.array([(cp[k] - cm[k]) / (2 * st) for k in range(60)], dtype=object)
    Hs = np.zeros((60, 60), dtype=object)
    # the scalar pieces couple only: x with x through Q (constant), u with u inside a foot's force triple and through R' (constant): second differences in
    # the arm entries (diagonal) and in the force triples, the constant weights added exactly
    W = np.zeros((60, 60), dtype=object); W[:30, :30] = M.mat(P.Q); W[30:, 30:] = M.mat(P.R)

    def nonquadratic(zz):
        dx, du = zz[:30] - M.vec(xref), zz[30:] - M.vec(LR.nominal_input(P, mode))
        return scalar(zz) - dx.dot(M.mat(P.Q)).dot(dx) / 2 - du.dot(M.mat(P.R)).dot(du) / 2
    n0 = nonquadratic(z)
    groups = [[24 + i] for i in range(6)] + [[54 + i] for i in range(6)] + [[30 + 3 * cc + a_ for a_ in range(3)] for cc in range(4)]
    for grp in groups:
        for i_ in grp:
            for j_ in grp:
                if j_ < i_:
                    continue
                d = (nonquadratic(z + E[i_] + E[j_]) - nonquadratic(z + E[i_] - E[j_]) - nonquadratic(z - E[i_] + E[j_]) + nonquadratic(z - E[i_] - E[j_])) / (4 * st * st) if i_ != j_ \
                    else (nonquadratic(z + E[i_]) - 2 * n0 + nonquadratic(z - E[i_])) / (st * st)
                Hs[i_, j_] = Hs[j_, i_] = d
    Hs = Hs + W
    # the diagonal shift of the cone's Hessian: p'(h) (-shift I) on every stance foot
    for cc in range(4):
        if LR.contact_flags(mode)[cc]:
            uu = z[30:]
            hh = mp.mpf(P.friction_coefficient) * uu[3 * cc + 2] - mp.sqrt(uu[3 * cc] ** 2 + uu[3 * cc + 1] ** 2 + mp.mpf(P.friction_regularization))
            p1 = (_mp_penalty(P.friction_barrier_mu, P.friction_barrier_delta, hh + st) - _mp_penalty(P.friction_barrier_mu, P.friction_barrier_delta, hh - st)) / (2 * st)
            for a_ in range(3):
                Hs[30 + 3 * cc + a_, 30 + 3 * cc + a_] -= p1 * mp.mpf(P.friction_hessian_shift)
    mu_ = np.array(mu, dtype=object)
    o.update(Q=f(dt * (Hs[:30, :30] + Jx.T.dot(np.diag(mu)).dot(Jx))), R=f(dt * Hs[30:, 30:]), q=f(dt * (g[:30] + Jx.T.dot(mu_ * h))), r=f(dt * g[30:]))
    return o


def test_reference_agrees_with_itself_in_50_digits(interface):
    """Two nodes (a trot intermediate node of the event scenario in mid swing, with momentum, Euler angles, tangential forces, joint rates, defects and the
    two-knot target all non-zero; and a terminal node): the float64 complex-step blocks against central differences of the restated value functions in 50-digit
    arithmetic.  Measured on the scale of the block bar, max(1, |block|_inf); the reference may use up a tenth of that bar (1e-11) and no more.
    Measured (profiles/lq_reference.md): every block <= 3e-16.
    Shared with lq_reference, not restated: the swing spline (LR.swing_z, evaluated on mpmath numbers), the target interpolation (LR.references: lerp and slerp),
    the node mode, the nominal input and the input weight R'.  So this check covers the complex-step differentiation and the restated kinematics, flow map, RK2
    map, rows, EE error and cost pieces -- not the swing spline's or the target interpolation's formulas."""
    mp.mp.dps = 50
    P = LS.params(interface)
    sc, ref, _ = LS.scenario(interface, "events")
    mid = [k for (i, k) in sc.checks if i == 0][3]
    M = MpModel(P)
    worst = {}
    for (i, k) in ((0, mid), (0, sc.N)):
        a = sc.node(i, k)
        assert a["terminal"] or LR.node_mode(a["events"], a["modes"], a["t"]) == 9
        t0 = time.perf_counter()
        exact = _mp_blocks(M, P, a)
        for key, d in LR.deviations(ref[(i, k)], exact, a["terminal"]).items():
            worst[("terminal " if a["terminal"] else "") + key] = d
        print("50-digit node", k, f"{time.perf_counter() - t0:.1f} s")
    print("reference vs 50 digits:", {k: f"{d:.1e}" for k, d in worst.items()})
    assert max(worst.values()) <= 0.1 * LS.BAR, worst


# ------------------------------------------------------------------------------------------------ 3. the oracle against the reference
@pytest.mark.parametrize("name", list(LS.BUILDERS))
def test_oracle_blocks_equal_the_reference(interface, oracle, name):
    sc, ref, _ = LS.scenario(interface, name)
    if LS.interface_of(interface, name) is not interface:
        oracle = S.Oracle(LS.interface_of(interface, name).problem)

    def lq_of(i, k):
        a = sc.node(i, k)
        n = int(sc.nev[i])
        assert oracle.node_mode_at(sc.ev[i, :n], sc.md[i, :n + 1], a["t"]) == LR.node_mode(a["events"], a["modes"], a["t"])
        o = oracle.lq_node(a["t"], a["dt"], a["x"], a["u"], a["xnext"], a["terminal"], n, sc.ev[i], sc.md[i], sc.tt[i], sc.ts[i])
        assert abs(o["cost"] - ref[(i, k)]["cost"]) <= LS.BAR * max(1.0, abs(ref[(i, k)]["cost"])), (name, i, k, o["cost"], ref[(i, k)]["cost"])
        return o
    LS.assert_blocks(sc, ref, lq_of, "oracle")


# ------------------------------------------------------------------------------------------------ 4. the host-emulated kernels against the reference
@pytest.fixture(scope="module")
def emu():
    return api.QMInterface(lib=abi.load_library(S.build_emu()))


@pytest.mark.parametrize("name", list(LS.BUILDERS))
def test_emulated_kernel_blocks_equal_the_reference(interface, emu, name):
    """ad_node_kernel + lq_node_kernel on host threads: one SQP iteration from the warm start with the LQ dump on, every block of every checked node"""
    sc, ref, _ = LS.scenario(interface, name)
    B, N = sc.B, sc.N
    sol = api.GpuSolver(LS.interface_of(emu, name), max_batch=B, max_nodes=N)
    sol.enable_debug(True)
    oT, oX, oU, oM, oS = np.zeros((B, N + 1)), np.zeros((B, N + 1, 30)), np.zeros((B, N, 30)), np.zeros((B, N + 1), dtype=np.int32), np.zeros((B, abi.NSTATS))
    kw = LS.solve_args(sc)
    sol.mpc(sol.mpc_args(B, N, sc.x0, sc.tt, sc.ts, sc.nev, sc.ev, sc.md, oT, oX, oU, oM, oS, t0=np.zeros(B) if sc.uniform else None, time_grid=kw["time_grid"],
                         warm_x=kw["warm"][0], warm_u=kw["warm"][1], line_search=False))
    assert np.array_equal(oT, sc.grid) and (oS[:, 7] == 0).all()
    for (i, k) in sc.checks:
        if k < N:
            assert oM[i, k] == LR.node_mode(sc.ev[i, :sc.nev[i]], sc.md[i], sc.grid[i, k]), (name, i, k)
    LS.assert_blocks(sc, ref, sol.debug_lq, "emulation")
    sol.close()
