"""Scenarios of the LQ-block pin (lq_reference.py), shared by the CPU tier (test_lq_reference.py: oracle and host-emulated kernels) and the GPU tier
(test_gpu_lq.py).  Every input is built with the reference's own forward kinematics and schedule rules -- no oracle, no kernel-derived helper -- and every
iterate goes in as a warm start (X, U), so the blocks are formed exactly at the chosen points.  A scenario names the nodes (instance, node) that are checked;
the reference's blocks of those nodes are computed once per process and shared by all tests (reference_blocks)."""
import time

import numpy as np

import lq_reference as LR
from qm_door_amd import abi, api


class Scenario:
    def __init__(self, name, tt, ts, nev, ev, md, grid, X, U, checks, uniform=True):
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        self.name, self.B, self.N = name, X.shape[0], X.shape[1] - 1
        self.tt, self.ts, self.grid, self.X, self.U = f64(tt), f64(ts), f64(grid), f64(X), f64(U)
        self.x0 = f64(self.X[:, 0])                                      # the solvers put x0 into X[0] before they linearise
        self.nev, self.ev, self.md = np.ascontiguousarray(nev, dtype=np.int32), f64(ev), np.ascontiguousarray(md, dtype=np.int32)
        self.checks, self.uniform = sorted(set(checks)), uniform
        assert self.grid.shape == (self.B, self.N + 1) and self.U.shape == (self.B, self.N, 30) and len(self.checks) <= 30

    def node(self, i, k):
        """the arguments of lq_reference.lq_node (and, but for the first, of the oracle's lq_node) for node k of instance i"""
        n, N = int(self.nev[i]), self.N
        term = k == N
        return dict(t=self.grid[i, k], dt=0.0 if term else self.grid[i, k + 1] - self.grid[i, k], x=self.X[i, k], u=None if term else self.U[i, k],
                    xnext=None if term else self.X[i, k + 1], terminal=term, events=self.ev[i, :n], modes=self.md[i, :n + 1], ttimes=self.tt[i], tstates=self.ts[i])


def pad_schedule(events, modes):
    ev = np.full(abi.MAX_EVENTS, 1e300); ev[:len(events)] = events
    md = np.full(abi.MAX_EVENTS + 1, 15, dtype=np.int32); md[:len(modes)] = modes
    return len(events), ev, md


def trot_schedule(t_end, phase0, period=0.70):
    """STANCE until phase0, then LF_RH (9) / RF_LH (6) half periods past t_end, then STANCE"""
    ev, md, t = [phase0], [15], phase0
    while t < t_end:
        for mode in (9, 6):
            md.append(mode); t += period / 2; ev.append(t)
    return pad_schedule(ev, md + [15])


def ee_pose(x):
    """(position, quaternion xyzw) of the end-effector at state x, by the reference's forward kinematics"""
    k = LR.kinematics(np.asarray(x, float)[6:30])
    return k["ee"].real, LR.quaternion_of(k["Ree"]).real


def quat(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.r_[a * np.sin(angle / 2), np.cos(angle / 2)]


def quat_mul(a, b):
    return np.r_[a[3] * b[:3] + b[3] * a[:3] + np.cross(a[:3], b[:3]), a[3] * b[3] - a[:3] @ b[:3]]


def away(rng, lo, hi, shape):
    """uniform in [-hi, -lo] u [lo, hi]: never zero"""
    return rng.choice([-1.0, 1.0], shape) * rng.uniform(lo, hi, shape)


def moving_iterate(P, rng, modes_of_nodes, yaw=None):
    """(X [N+1][30], U [N][30]) with every node seeded differently: normalised momentum != 0 in all six entries, all three Euler angles != 0 (up to 0.4 rad),
    stance forces with tangential parts, joint rates != 0, and X[k+1] unrelated to rk2(X[k], U[k]) (b != 0)"""
    N = len(modes_of_nodes)
    X = P.initial_state[None, :] + np.c_[away(rng, 0.05, 0.3, (N + 1, 6)), rng.uniform(-0.1, 0.1, (N + 1, 3)), away(rng, 0.1, 0.4, (N + 1, 3)), away(rng, 0.02, 0.15, (N + 1, 18))]
    if yaw is not None:
        X[:, 9] = yaw + rng.uniform(-0.05, 0.05, N + 1)
    U = np.zeros((N, 30))
    for k, mode in enumerate(modes_of_nodes):
        fl = LR.contact_flags(mode)
        U[k] = LR.nominal_input(P, mode)
        for c in range(4):
            U[k, 3 * c:3 * c + 3] += np.r_[away(rng, 3.0, 15.0, 2), rng.uniform(-10, 10)] if fl[c] else away(rng, 0.2, 1.0, 3)
        U[k, 12:] = away(rng, 0.05, 0.5, 18)
    return X, U


def two_knots(P, rng, B, t_lo, t_hi):
    """two target knots around the horizon with different base poses, EE positions and EE orientations"""
    pos, q = ee_pose(P.initial_state)
    tt = np.tile([t_lo, t_hi], (B, 1))
    ts = np.tile(np.r_[P.initial_state, pos, q], (B, 2, 1))
    for i in range(B):
        ts[i, 0, 6:12] += rng.uniform(-0.05, 0.05, 6); ts[i, 1, 6:12] += rng.uniform(-0.1, 0.1, 6)
        ts[i, 0, 30:33] += rng.uniform(-0.05, 0.05, 3); ts[i, 1, 30:33] += rng.uniform(-0.1, 0.1, 3)
        ts[i, 0, 33:37] = quat_mul(quat(rng.standard_normal(3), 0.3), q); ts[i, 1, 33:37] = quat_mul(quat(rng.standard_normal(3), -0.7), q)
    return tt, ts


# ------------------------------------------------------------------------------------------------ the scenario groups
def all_modes(P):
    """All 16 contact modes, moving.  B = 16, N = 4: five nodes per instance, so lq_node_kernel's wavefronts of three nodes end part-filled.  Instance m holds
    mode m; its only event lies far ahead.  Checked: one intermediate node of every instance; nodes 0, N - 1 and N in four instances each."""
    B, N = 16, 4
    rng = np.random.default_rng(4101)
    grid = np.tile(np.arange(N + 1) * P.dt, (B, 1))
    nev, ev, md = zip(*[pad_schedule([20 * N * P.dt], [m, 15]) for m in range(B)])
    XU = [moving_iterate(P, rng, [m] * N) for m in range(B)]
    tt, ts = two_knots(P, rng, B, -0.05, N * P.dt + 0.05)
    checks = [(m, 1 + m % 3) for m in range(B)] + [(m, 0) for m in (0, 5, 10, 15)] + [(m, N - 1) for m in (1, 6, 11, 12)] + [(m, N) for m in (2, 7, 9, 14)]
    return Scenario("all_modes", tt, ts, nev, ev, md, grid, np.array([a for a, _ in XU]), np.array([b for _, b in XU]), checks)


HALF_TURN_W = 1e-5      # |w| of the EE quaternion of the half-turn instance: the trace > 0 formula would be off by eps / w^2 ~ 1e-6 there, four orders above the bar


def quaternion_branches(P):
    """Instance 0: base yaw 2.6 rad, the EE world rotation has a negative trace (Eigen's second branch of rotation -> quaternion).  Instance 1: the target
    quaternions lie in the opposite hemisphere from the measured one.  Instance 3: base yaw -2.6 rad, negative trace AND w < 0 in Eigen's branch (with yaw +2.6 both
    branches return the same quaternion up to its sign, which cancels in every block).  Instance 4: the EE world rotation 1e-5 short of a half turn in the quaternion's w
    (2e-5 rad), where the trace > 0 formula divides by w and loses eps / w^2 -- the region Eigen's second branch exists for, and the instance that tells the branches apart.  Instance 2: the two target knots lie in opposite hemispheres of each other (slerp's sign flip)."""
    B, N = 5, 2
    rng = np.random.default_rng(4102)
    grid = np.tile(np.arange(N + 1) * P.dt, (B, 1))
    nev, ev, md = zip(*[pad_schedule([20 * N * P.dt], [15, 15])] * B)
    XU = [moving_iterate(P, rng, [15] * N, yaw={0: 2.6, 3: -2.6}.get(i)) for i in range(B)]
    X, U = np.array([a for a, _ in XU]), np.array([b for _, b in XU])
    tt, ts = two_knots(P, rng, B, -0.05, N * P.dt + 0.05)
    # instance 4: the base yaw of every node chosen so that the EE world rotation is HALF_TURN_W short of a half turn.  R_ee = R_z(yaw) M, so
    # w(yaw) = cos(yaw / 2) w_M - sin(yaw / 2) z_M with (z_M, w_M) of the rotation at yaw = 0: zero at yaw_0 = 2 atan2(w_M, z_M)
    for k in range(N + 1):
        X[4, k, 9] = 0.0
        qM = ee_pose(X[4, k])[1]
        X[4, k, 9] = 2.0 * np.arctan2(qM[3], qM[2]) - 2.0 * HALF_TURN_W / np.hypot(qM[3], qM[2])
        R = LR.kinematics(X[4, k, 6:30])["Ree"].real
        assert np.trace(R) < 0 and 0.5 * HALF_TURN_W < 0.5 * np.sqrt(np.trace(R) + 1.0) < 2.0 * HALF_TURN_W, (k, np.trace(R))
    for j in range(2):
        ts[4, j, 33:37] = quat_mul(quat([0, 0, 1], X[4, 1, 9]), ts[4, j, 33:37])
    for k in range(N + 1):
        assert np.trace(LR.kinematics(X[0, k, 6:30])["Ree"].real) < 0 and np.trace(LR.kinematics(X[3, k, 6:30])["Ree"].real) < 0
        assert ee_pose(X[3, k])[1][3] < 0                                          # where the trace > 0 formula would return the OTHER sign of the quaternion
    q1 = ee_pose(X[1, 1])[1]
    for j in range(2):
        ts[0, j, 33:37] = quat_mul(quat([0, 0, 1], 2.6), ts[0, j, 33:37])          # the target turned with the base
        ts[3, j, 33:37] = quat_mul(quat([0, 0, 1], -2.6), ts[3, j, 33:37])
        ts[1, j, 33:37] *= -np.sign(ts[1, j, 33:37] @ q1)
    ts[2, 1, 33:37] *= -np.sign(ts[2, 1, 33:37] @ ts[2, 0, 33:37])
    assert ts[1, 0, 33:37] @ q1 < 0 and ts[1, 1, 33:37] @ q1 < 0 and ts[2, 0, 33:37] @ ts[2, 1, 33:37] < 0
    return Scenario("quaternion_branches", tt, ts, nev, ev, md, grid, X, U, [(i, k) for i in range(B) for k in range(N + 1)])


def barriers(P):
    """The relaxed barriers on both sides of delta: friction h below delta and a foot that pulls (h < 0) next to feet well inside the cone; arm joints within
    delta of a URDF limit, on it and beyond it; arm rates beyond both bounds and inside the delta band.  Stance, then trot from node 2; two distinct target knots."""
    B, N = 4, 3
    rng = np.random.default_rng(4103)
    grid = np.tile(np.arange(N + 1) * P.dt, (B, 1))
    sched = trot_schedule(N * P.dt + 1.0, phase0=1.5 * P.dt)           # stance at nodes 0, 1; LF_RH from node 2
    nev, ev, md = zip(*[sched] * B)
    modes = [LR.node_mode(sched[1][:sched[0]], sched[2], k * P.dt) for k in range(N)]
    assert modes == [15, 15, 9]
    XU = [moving_iterate(P, rng, modes) for _ in range(B)]
    X, U = np.array([a for a, _ in XU]), np.array([b for _, b in XU])
    lo, up = LR.ARM_LOWER, LR.ARM_UPPER
    X[0, :, 24] = up[0] - 5e-4; X[0, :, 25] = lo[1] + 2e-4                 # inside the delta band
    X[1, :, 26] = up[2]; X[1, :, 27] = lo[3]                               # exactly on the limits
    X[2, :, 24] = up[0] + 0.02; X[2, :, 28] = lo[4] - 0.01                 # beyond
    U[0, :, 24] = P.arm_vel_upper[0] + 0.05; U[1, :, 26] = P.arm_vel_lower[2] - 0.2; U[2, :, 29] = P.arm_vel_upper[5] - 4e-4; U[3, :, 27] = P.arm_vel_lower[3] + 3e-4
    for i in range(B):
        for k in range(N):
            st = [c for c in range(4) if LR.contact_flags(modes[k])[c]]
            U[i, k, 3 * st[0]:3 * st[0] + 3] = [4.0, -1.0 - i, 3.0 + i]     # h = 0.7 f_z - sqrt(f_x^2 + f_y^2 + 25) < 0 < delta: quadratic branch
            if i == 3:
                U[i, k, 3 * st[-1] + 2] = -6.0                             # pulling on the ground
            if i == 2:
                f = U[i, k, 3 * st[-1]:3 * st[-1] + 3]                      # h a hair above / below delta on the last stance foot
                f[2] = (np.sqrt(f[0] ** 2 + f[1] ** 2 + P.friction_regularization) + P.friction_barrier_delta * (1.5 if k % 2 else 0.5)) / P.friction_coefficient
    tt, ts = two_knots(P, rng, B, -0.05, N * P.dt + 0.05)
    return Scenario("barriers", tt, ts, nev, ev, md, grid, X, U, [(i, k) for i in range(B) for k in range(N)] + [(0, N), (2, N)])


def events(P):
    """An event-aligned grid (api.time_grid_with_events) over one whole swing of a trot: a node exactly ON an event time with the short step in front of it and
    the full step behind it (the product keeps ONE node per event where upstream has a zero-length (pre, post) pair -- DESIGN.md section 8 (1), identical for this
    robot's identity jump map; the reference follows that choice: the node on the event takes the mode that starts there), a swing foot at the first node after
    lift-off, at mid swing and at the last node before touch-down."""
    B = 2
    rng = np.random.default_rng(4104)
    horizon = 0.45
    nev, ev, md = trot_schedule(horizon + 1.0, phase0=3 * P.dt + 0.0025)
    N, g = api.time_grid_with_events(0.0, horizon, P.dt, ev[:nev])
    on = [int(np.flatnonzero(g == e)[0]) for e in ev[:2]]                  # the nodes ON lift-off and ON touch-down of LF / RH's ... RF / LH's swing (mode 9)
    assert g[on[0]] - g[on[0] - 1] < 0.25 * P.dt and on[1] - on[0] > 6
    mid = int(np.argmin(np.abs(g - 0.5 * (ev[0] + ev[1]))))
    modes = [LR.node_mode(ev[:nev], md, t) for t in g[:-1]]
    assert modes[on[0] - 1] == 15 and modes[on[0]] == 9 and modes[on[1] - 1] == 9 and modes[on[1]] == 6
    XU = [moving_iterate(P, rng, modes) for _ in range(B)]
    tt, ts = two_knots(P, rng, B, -0.05, horizon + 0.05)
    nodes = [on[0] - 1, on[0], on[0] + 1, mid, on[1] - 1, on[1]]
    return Scenario("events", tt, ts, [nev] * B, [ev] * B, [md] * B, np.tile(g, (B, 1)), np.array([a for a, _ in XU]), np.array([b for _, b in XU]),
                    [(i, k) for i in range(B) for k in nodes] + [(0, N)], uniform=False)


# the product's task file sets positionErrorGain 0, where a wrong sign or a missing z row of that term cannot show: the event scenario runs a second time with it on
POSITION_ERROR_GAIN = 5.0
BUILDERS = {"all_modes": all_modes, "quaternion_branches": quaternion_branches, "barriers": barriers, "events": events, "events_with_position_error_gain": events}
_cache = {}


def interface_of(interface, name):
    """the interface scenario `name` is solved with: the given one, or a second one on the same library with positionErrorGain switched on"""
    if not name.endswith("_with_position_error_gain"):
        return interface
    key = ("gain_interface", id(interface))
    if key not in _cache:
        itf = api.QMInterface(lib=interface.lib)
        itf.problem.settings.position_error_gain = POSITION_ERROR_GAIN
        _cache[key] = itf
    return _cache[key]


def params(interface, name=""):
    key = "P_gain" if name.endswith("_with_position_error_gain") else "P"
    if key not in _cache:
        _cache[key] = LR.Params(interface.problem.settings)
        if key == "P_gain":
            _cache[key].position_error_gain = POSITION_ERROR_GAIN
    return _cache[key]


def scenario(interface, name):
    """scenario `name` with the reference's blocks of its checked nodes: (Scenario, {(i, k): blocks}, seconds the reference took); built once per process"""
    if name not in _cache:
        P = params(interface, name)
        sc = BUILDERS[name](P)
        sc.name = name
        t0 = time.perf_counter()
        ref = {(i, k): LR.lq_node(P, **sc.node(i, k)) for i, k in sc.checks}
        _cache[name] = (sc, ref, time.perf_counter() - t0)
    return _cache[name]


def worst(sc, ref, lq_of):
    """{block: worst deviation over the checked nodes} of lq_of(i, k) -> blocks against the reference, on the scale of the bar; nc must be equal"""
    out = {}
    for (i, k), r in ref.items():
        g = lq_of(i, k)
        assert g["nc"] == r["nc"], (sc.name, i, k, g["nc"], r["nc"])
        for key, d in LR.deviations(g, r, k == sc.N).items():
            assert np.isfinite(d), (sc.name, key, d, "instance", i, "node", k)          # a NaN block must not slip through the comparison below
            if d > out.get(key, (-1.0,))[0]:
                out[key] = (d, i, k)
    seen = set(LR.TERMINAL_BLOCKS if all(k == sc.N for _, k in ref) else LR.BLOCKS)
    assert set(out) == seen, (sc.name, sorted(out))
    return out


BAR = 1e-10      # the project's LQ-block bar: |got - ref|_inf <= 1e-10 max(1, |ref|_inf) per block


def assert_blocks(sc, ref, lq_of, who):
    w = worst(sc, ref, lq_of)
    print(who, sc.name, {k: f"{d:.1e}" for k, (d, _, _) in w.items()})
    for key, (d, i, k) in w.items():
        assert d <= BAR, (who, sc.name, key, d, "instance", i, "node", k)
    return w


def solve_args(sc):
    """keyword arguments of harness.MpcBatch / the emulated solve: one SQP iteration from the warm start, no line search"""
    return dict(warm=(sc.X, sc.U), line_search=False, time_grid=None if sc.uniform else sc.grid)
