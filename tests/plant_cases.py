"""The cases of the plant step (include/qmgpu.h: qmgpu_plant_step_batch) that test_emu_plant.py runs on the host emulation build and test_gpu_plant.py on the GPU:
seeded robots in motion, the call through api.GpuSolver.plant_step, the comparison with plant_reference.py under its tolerance rule, and the oracle-free checks
(pinned feet at rest and the end-effector slots, against tests/urdf_model.fk).  A Runner hides where the arrays live: numpy for the emulated library, torch on the GPU.

Pinned feet: the step imposes Jc(q) v+ = 0 with the Jacobian of the configuration q the last substep STARTS from, so the velocity checked is d/de fk(q + e v+), the
complex step at q = q+ - h v+ along v+.  (At q+ itself the same feet move by h (dJc/dq v+) v+, first order in h: that is the drift DESIGN.md section 4.13 states.)

Oracle-free bounds: |value| <= C eps sum|terms|.  C per class is the next power of two at or above twice the worst ratio measured on the host emulation build
(profiles/plant_parity.json, "oracle_free_worst"): foot velocity 10.8 -> 32, end-effector position 1.6 -> 4, quaternion 14.7 -> 32.
With PLANT_RECORD set to a file path every comparison adds its figures there."""
import json
import os

import numpy as np

import lq_reference as LR
import plant_reference as PR
import support as S
import urdf_model as UM
from qm_door_amd import abi, api

RECORD = os.environ.get("PLANT_RECORD") or None
EPS = PR.EPS
C_FREE = {"foot_vel": 32.0, "ee_pos": 4.0, "ee_quat": 32.0}
OUTPUTS = ("rbd_next", "contact_force", "tau_applied", "status")


class Runner:
    def __init__(self, itf, orc, section, to_dev=None, to_host=None, make_solver=None):
        self.itf, self.orc, self.section = itf, orc, section
        self.to_dev = to_dev or (lambda a: np.ascontiguousarray(a))
        self.to_host = to_host or (lambda a: np.array(a))
        self.make_solver = make_solver or (lambda B, N=4, dtype="f64", itf=None: api.GpuSolver(itf or self.itf, max_batch=B, max_nodes=N, dtype=dtype))
        self.solvers = {}

    def solver(self, B):
        if B not in self.solvers:
            self.solvers[B] = self.make_solver(B)
        return self.solvers[B]

    def call(self, c, rows=None, sol=None, in_place=False, zero_gains=False, **change):
        """one plant call on instances `rows` (default: all) of case c (dict); returns the outputs as numpy arrays.  Outputs are pre-filled with NaN / -1."""
        c = dict(c, **change)
        B0 = c["rbd"].shape[0]
        rows = list(range(B0)) if rows is None else rows
        B = len(rows)
        pick = lambda a: None if a is None else self.to_dev(np.ascontiguousarray(np.asarray(a)[rows]))  # noqa: E731
        gains = {k: pick(c.get(k)) for k in ("pos_des", "vel_des", "kp", "kd")}
        if zero_gains:
            gains = {k: self.to_dev(np.zeros((B, 18))) for k in gains}
        rbd = pick(c["rbd"])
        out = dict(rbd_next=rbd if in_place else self.to_dev(np.full((B, 55), np.nan)), contact_force=self.to_dev(np.full((B, 12), np.nan)),
                   tau_applied=self.to_dev(np.full((B, 18), np.nan)), status=self.to_dev(np.full(B, -1, dtype=np.int32)))
        sol = sol or self.solver(max(B, 5))
        a = sol.plant_args(B, rbd, pick(c["tau_ff"]), pick(c["mode"].astype(np.int32)), pick(c["dt"]), out["rbd_next"], substeps=c.get("substeps", 1),
                           clamp_effort=c.get("clamp", False), ee_force=pick(c.get("ee_force")), contact_force=out["contact_force"], tau_applied=out["tau_applied"],
                           status=out["status"], **gains)
        sol.plant_step(a)
        sol.synchronize()
        return {k: self.to_host(v) for k, v in out.items()}


def standing_torque(orc, problem, rbd, mode, ee_force=None):
    """(nle - Jc' F0)_j with F0 the weight shared by the stance feet: a feed-forward torque near the one that holds the robot"""
    M, nle, Jf = PR.model_terms(orc, rbd, ee_force)
    F0 = S.nominal_input(problem.model.total_mass, mode, problem.settings.gravity)[:12]
    return (nle - Jf.T @ F0)[6:]


def make_case(itf, orc, B, mode, seed, dt=0.002, moving=True, **kw):
    """B robots near the nominal stance, every velocity non-zero (moving), a feed-forward torque near the holding one plus a seeded offset"""
    rng = np.random.default_rng(seed)
    x = S.perturbed_states(itf.initial_state, B, seed=seed)
    vel = np.c_[rng.uniform(-0.3, 0.3, (B, 6)), rng.uniform(-0.5, 0.5, (B, 18))] * (1.0 if moving else 0.0)
    vel[vel == 0.0] += 0.01 if moving else 0.0
    rbd = np.array([S.rbd_from_state(orc, x[i], vel[i]) for i in range(B)])
    modes = np.broadcast_to(np.asarray(mode, dtype=np.int32), (B,)).copy()
    tau = np.array([standing_torque(orc, itf.problem, rbd[i], int(modes[i]), None) for i in range(B)]) + rng.uniform(-1, 1, (B, 18)) * (0.5 if moving else 0.0)
    c = dict(rbd=rbd, tau_ff=tau, mode=modes, dt=np.full(B, dt), substeps=1)
    c.update(kw)
    return c


def with_gains(c, seed=3):
    rng = np.random.default_rng(seed)
    B = c["rbd"].shape[0]
    return dict(c, pos_des=c["rbd"][:, 6:24] + rng.uniform(-0.05, 0.05, (B, 18)), vel_des=rng.uniform(-0.3, 0.3, (B, 18)),
                kp=np.tile(np.r_[np.full(12, 20.0), np.full(6, 5.0)], (B, 1)), kd=np.tile(np.r_[np.full(12, 3.0), np.full(6, 0.5)], (B, 1)))


def reference(runner, c, i, bounds=True):
    g = lambda k: None if c.get(k) is None else c[k][i]  # noqa: E731
    return PR.step(runner.orc, runner.itf.problem, c["rbd"][i], c["tau_ff"][i], int(c["mode"][i]), float(c["dt"][i]), substeps=c.get("substeps", 1),
                   clamp_effort=c.get("clamp", False), pos_des=g("pos_des"), vel_des=g("vel_des"), kp=g("kp"), kd=g("kd"), ee_force=g("ee_force"), bounds=bounds, seed=100 + i)


def record(section, name, rec):
    if not RECORD:
        return
    try:
        allrec = json.load(open(RECORD))
    except (OSError, ValueError):
        allrec = {}
    allrec.setdefault(section, {})[name] = rec
    free = [r["oracle_free"] for s in allrec.values() if isinstance(s, dict) for r in s.values() if isinstance(r, dict) and "oracle_free" in r]
    if free:
        allrec["oracle_free_worst"] = {k: max(f[k] for f in free) for k in C_FREE}
        allrec["C_oracle_free"] = C_FREE
    os.makedirs(os.path.dirname(os.path.abspath(RECORD)), exist_ok=True)
    json.dump(allrec, open(RECORD, "w"), indent=1)


def oracle_free_ratios(got, c, i):
    """worst |value| / (eps sum|terms|) of: the velocities of the pinned feet at (q+, v+), by complex step through urdf_model.fk; the end-effector slots against fk(q+)"""
    q, v = PR.coordinates(got["rbd_next"][i])
    flags = S.contact_flags(int(c["mode"][i]))
    worst = dict(foot_vel=0.0, ee_pos=0.0, ee_quat=0.0)
    if any(flags):
        q_start = q - (float(c["dt"][i]) / c.get("substeps", 1)) * v
        fv, mag = PR.foot_velocities(q_start, v), PR.foot_velocity_magnitude(q_start, v)
        for f in range(4):
            if flags[f]:
                worst["foot_vel"] = max(worst["foot_vel"], float((np.abs(fv[f]) / (EPS * mag[f])).max()))
    pose = UM.fk(q)
    R0, p = pose["base"][0].real, q[0:3]
    ee, Ree = pose[UM.EE_LINK][1].real, pose[UM.EE_LINK][0].real
    ee_mag = np.abs(p) + np.abs(R0) @ np.abs(R0.T @ (ee - p))
    worst["ee_pos"] = float((np.abs(got["rbd_next"][i, 48:51] - ee) / (EPS * ee_mag)).max())
    qt = np.real(LR.quaternion_of(Ree[None])).reshape(4)
    import taskspace_reference as TR
    qmag = TR.quaternion_mag(Ree, np.abs(R0) @ np.abs(R0.T @ Ree), qt)
    worst["ee_quat"] = float((np.abs(got["rbd_next"][i, 51:55] - qt) / (EPS * qmag)).max())
    return worst


def check_accuracy(runner, name, c, got=None, free=True):
    """every instance of case c against the refined reference under the tolerance rule, the status words exact, and the oracle-free checks; every figure is printed and
    recorded before anything is asserted"""
    got = runner.call(c) if got is None else got
    B = c["rbd"].shape[0]
    rows = []
    for i in range(B):
        ref = reference(runner, c, i)
        assert ref["bound"] is not None, (name, i, "the reference failed a pivot")
        err = PR.errors(got["rbd_next"][i], got["contact_force"][i], got["tau_applied"][i], int(c["mode"][i]), ref)
        rows.append(dict(i=i, err=err, bound=ref["bound"], parts=ref["parts"], status=[int(got["status"][i]), int(ref["status"])],
                         oracle_free=oracle_free_ratios(got, c, i) if free else None, iterations=ref["last"]["sol"]["iterations"]))
    rec = dict(instances=B, mode=sorted({int(m) for m in c["mode"]}), substeps=c.get("substeps", 1),
               err={k: max(r["err"][k] for r in rows) for k in PR.KEYS}, bound={k: min(r["bound"][k] for r in rows) for k in PR.KEYS},
               e_np={k: max(r["parts"][k]["e_np"] for r in rows) for k in PR.KEYS}, e_in={k: max(r["parts"][k]["e_in"] for r in rows) for k in PR.KEYS},
               floor={k: max(r["parts"][k]["floor"] for r in rows) for k in PR.KEYS})
    if free:
        rec["oracle_free"] = {k: max(r["oracle_free"][k] for r in rows) for k in C_FREE}
    print(name, runner.section, json.dumps(rec))
    record(runner.section, name, rec)
    assert all(np.isfinite(got[k]).all() for k in ("rbd_next", "contact_force", "tau_applied")), name
    for r in rows:
        assert r["status"][0] == r["status"][1], (name, r)
        for k in PR.KEYS:
            assert r["err"][k] <= r["bound"][k], (name, k, r)
        if free:
            for k in C_FREE:
                assert r["oracle_free"][k] <= C_FREE[k], (name, k, r)
    for i in range(B):
        flags = S.contact_flags(int(c["mode"][i]))
        for f in range(4):
            assert flags[f] or not got["contact_force"][i, 3 * f: 3 * f + 3].any(), (name, i, f)
    return got


def same_bits(a, b, keys=OUTPUTS):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


# ------------------------------------------------------------------------------------------------ the cases of the issue's table
def case_a(runner):
    for B in (1, 5):
        check_accuracy(runner, f"a_stance_B{B}", make_case(runner.itf, runner.orc, B, 15, seed=40 + B))


def swing_case(runner, mode, seed):
    """mode 9 or 6 with the first swing foot moving at 0.5 m/s: its leg's joint rates are solved from the foot Jacobian's own 3 x 3 block"""
    c = make_case(runner.itf, runner.orc, 5, mode, seed)
    foot = [f for f in range(4) if not S.contact_flags(mode)[f]][0]
    for i in range(5):
        q, v = PR.coordinates(c["rbd"][i])
        _, _, Jf = PR.model_terms(runner.orc, c["rbd"][i])
        Jrow = Jf[3 * foot: 3 * foot + 3]
        cols = [k for k in range(6, 24) if np.abs(Jrow[:, k]).max() > 0]
        assert len(cols) == 3
        target = np.array([0.3, 0.0, -0.4])            # 0.5 m/s, forward and down
        rest = Jrow @ v - Jrow[:, cols] @ v[cols]
        v[cols] = np.linalg.solve(Jrow[:, cols], target - rest)
        c["rbd"][i] = PR.state_record(q, v)
        assert abs(np.linalg.norm(PR.foot_velocities(q, v)[foot]) - 0.5) < 1e-9
    return c, foot


def case_b(runner):
    for mode, nxt, seed in ((9, 15, 51), (6, 15, 52)):
        c, foot = swing_case(runner, mode, seed)
        got = check_accuracy(runner, f"b_swing_mode{mode}", c)
        # touchdown: the foot is in contact in the next call; its velocity is zero afterwards (the inelastic contact takes the 0.5 m/s out in one step)
        for i in range(5):
            q, v = PR.coordinates(got["rbd_next"][i])
            assert np.linalg.norm(PR.foot_velocities(q, v)[foot]) > 0.1, (mode, i)
        td = dict(c, rbd=got["rbd_next"], mode=np.full(5, nxt, dtype=np.int32))
        check_accuracy(runner, f"b_touchdown_mode{mode}", td)


def case_c(runner):
    check_accuracy(runner, "c_three_feet", make_case(runner.itf, runner.orc, 5, 13, seed=53))


def case_d(runner):
    c = make_case(runner.itf, runner.orc, 5, 0, seed=54)
    got = check_accuracy(runner, "d_flight", c)
    assert not got["contact_force"].any() and not (got["status"] & (PR.PULL | PR.FRICTION)).any()


def case_e(runner):
    """three calls of dt / 3 give the same bits as one call with substeps = 3 (the forces are the last substep's in both)"""
    c = with_gains(make_case(runner.itf, runner.orc, 5, 15, seed=55, dt=0.003))
    one = runner.call(c, substeps=3)
    third = c["dt"] / 3.0
    assert np.array_equal(third, c["dt"] / np.float64(3))
    step = dict(c, dt=third)
    st = 0
    for _ in range(3):
        got = runner.call(step)
        st = st | got["status"]
        step = dict(step, rbd=got["rbd_next"])
    assert same_bits(one, got, ("rbd_next", "contact_force", "tau_applied")) and np.array_equal(one["status"], st)
    check_accuracy(runner, "e_substeps3", dict(c, substeps=3), got=one)


def case_f(runner):
    c = make_case(runner.itf, runner.orc, 5, 15, seed=56)
    assert same_bits(runner.call(c), runner.call(c, zero_gains=True))
    check_accuracy(runner, "f_gains", with_gains(c))


def case_g(runner):
    c = make_case(runner.itf, runner.orc, 5, 15, seed=57)
    lim = PR.effort_limits(runner.itf.problem)
    c["tau_ff"][:, 1] = 3.0 * lim[1]; c["tau_ff"][:, 14] = -2.0 * lim[14]
    got = check_accuracy(runner, "g_clamp", dict(c, clamp=True))
    assert (got["tau_applied"][:, 1] == lim[1]).all() and (got["tau_applied"][:, 14] == -lim[14]).all() and (np.abs(got["tau_applied"]) <= lim).all()
    free = runner.call(c)
    assert (free["tau_applied"][:, 1] == 3.0 * lim[1]).all() and not same_bits(free, got, ("rbd_next",))


def case_h(runner):
    c = make_case(runner.itf, runner.orc, 5, 15, seed=58)
    rng = np.random.default_rng(58)
    force = rng.uniform(-20, 20, (5, 3))
    got = check_accuracy(runner, "h_ee_force", dict(c, ee_force=force))
    assert not same_bits(got, runner.call(c), ("rbd_next",))


def case_i(runner):
    c = with_gains(make_case(runner.itf, runner.orc, 5, 9, seed=59))
    assert same_bits(runner.call(c), runner.call(c, in_place=True))


def case_j(runner):
    """bit 0.  (1) A doctored problem -- every mass and inertia negated -- fails M's first pivot on the reference too (numpy's Cholesky refuses it): the state comes back
    unchanged.  (2) One instance of a healthy batch whose gain overflows the joint law (a result that is not finite): that instance alone is flagged, its state comes
    back unchanged and finite, its neighbours keep their bits."""
    c = make_case(runner.itf, runner.orc, 5, 15, seed=60)
    bad = api.QMInterface(lib=runner.itf.lib)
    for b in range(abi.NB):
        bad.problem.model.mass[b] = -bad.problem.model.mass[b]
        for e in range(6):
            bad.problem.model.inertia[b][e] = -bad.problem.model.inertia[b][e]
    ref = PR.step(S.Oracle(bad.problem), bad.problem, c["rbd"][0], c["tau_ff"][0], 15, 0.002, bounds=False)
    assert ref["status"] & PR.FAILED and np.array_equal(ref["rbd_next"], c["rbd"][0])
    sol = runner.make_solver(5, itf=bad)
    got = runner.call(c, sol=sol)
    sol.close()
    assert (got["status"] & PR.FAILED).all() and np.array_equal(got["rbd_next"], c["rbd"]) and not got["contact_force"].any() and not got["tau_applied"].any()
    healthy = runner.call(c, pos_des=np.zeros((5, 18)), kp=np.zeros((5, 18)))
    kp = np.zeros((5, 18)); kp[2, 4] = 1e308
    pd = np.zeros((5, 18)); pd[2, 4] = 1e3
    got = runner.call(c, pos_des=pd, kp=kp)
    assert got["status"][2] & PR.FAILED and np.array_equal(got["rbd_next"][2], c["rbd"][2]) and np.isfinite(got["rbd_next"]).all() and not got["contact_force"][2].any()
    for i in (0, 1, 3, 4):
        assert not got["status"][i] & PR.FAILED and all(np.array_equal(got[k][i], healthy[k][i]) for k in OUTPUTS), i


def case_k(runner):
    """the invalid-argument list"""
    import pytest
    c = with_gains(make_case(runner.itf, runner.orc, 5, 15, seed=61))
    sol = runner.make_solver(5)
    d = runner.to_dev
    base = dict(batch=5, rbd=d(c["rbd"]), tau_ff=d(c["tau_ff"]), mode=d(c["mode"]), dt=d(c["dt"]), rbd_next=d(np.zeros((5, 55))), substeps=1, pos_des=d(c["pos_des"]),
                vel_des=d(c["vel_des"]), kp=d(c["kp"]), kd=d(c["kd"]))

    def refused(s, **change):
        kw = dict(base); kw.update(change)
        with pytest.raises(abi.QmGpuError) as e:
            s.plant_step(s.plant_args(**kw))
        assert e.value.status == abi.ERR_INVALID_ARGUMENT and str(e.value), change
    refused(sol, batch=6); refused(sol, batch=0); refused(sol, substeps=0); refused(sol, substeps=-1)
    for k in ("rbd", "tau_ff", "mode", "dt", "rbd_next"):
        refused(sol, **{k: None})
    refused(sol, pos_des=None); refused(sol, vel_des=None)
    f32 = runner.make_solver(5, dtype="f32")
    refused(f32)
    f32.close()
    assert runner.itf.lib.qmgpu_plant_step_batch(sol.handle, None) == abi.ERR_INVALID_ARGUMENT
    sol.plant_step(sol.plant_args(**dict(base, pos_des=None, kp=None, vel_des=None, kd=None)))     # all four gains absent: accepted
    sol.synchronize()
    sol.close()


def case_l(runner):
    c = with_gains(make_case(runner.itf, runner.orc, 5, np.array([15, 9, 6, 13, 0]), seed=62), seed=5)
    full = runner.call(c, substeps=2)
    for i in range(5):
        one = runner.call(c, rows=[i], substeps=2)
        assert all(np.array_equal(one[k][0], full[k][i]) for k in OUTPUTS), i


def case_m(runner):
    c = with_gains(make_case(runner.itf, runner.orc, 5, np.array([15, 9, 6, 13, 0]), seed=63))
    sol = runner.solver(5)
    first = runner.call(c, sol=sol)
    sol.debug_poison()
    assert same_bits(first, runner.call(c, sol=sol))


def case_n(runner, N=4):
    """a solve and a WBC call behind a plant call are bit-identical to the same calls without it"""
    itf, orc, d, B = runner.itf, runner.orc, runner.to_dev, 2
    x0 = S.perturbed_states(itf.initial_state, B, seed=7)
    tgt = S.nominal_target(orc, itf.initial_state)
    nev, ev, md = S.trot_schedule(1.0, phase0=0.03)
    rbd = np.array([S.rbd_from_state(orc, x0[i]) for i in range(B)])
    c = make_case(itf, orc, B, 15, seed=64)

    def cycle(with_plant):
        sol = runner.make_solver(B, N)
        if with_plant:
            runner.call(c, sol=sol)
        o = dict(T=d(np.zeros((B, N + 1))), X=d(np.zeros((B, N + 1, 30))), U=d(np.zeros((B, N, 30))), M=d(np.zeros((B, N + 1), dtype=np.int32)), S=d(np.zeros((B, abi.NSTATS))))
        a = sol.mpc_args(B, N, d(x0), d(np.zeros((B, 1))), d(np.tile(tgt, (B, 1, 1))), d(np.full(B, nev, dtype=np.int32)), d(np.tile(ev, (B, 1))), d(np.tile(md, (B, 1))),
                         o["T"], o["X"], o["U"], o["M"], o["S"], t0=d(np.zeros(B)))
        w = dict(out=d(np.zeros((B, 54))), status=d(np.zeros(B, dtype=np.int32)), il=d(np.zeros((B, 30))))
        wa = sol.wbc_args(B, d(rbd), d(np.full(B, 0.002)), d(np.full(B, 20.0)), w["il"], w["out"], w["status"])
        sol.cycle(a, d(np.zeros(B)), wa)
        sol.synchronize()
        res = {k: runner.to_host(v) for k, v in {**o, **w}.items()}
        sol.close()
        return res
    plain, behind = cycle(False), cycle(True)
    assert all(np.array_equal(plain[k], behind[k]) for k in plain), [k for k in plain if not np.array_equal(plain[k], behind[k])]
    assert np.isfinite(plain["out"]).all() and plain["out"][:, 36:].any()


def rest_case(runner):
    """a standing robot at rest under the torque that balances it (tau_j = (nle - Jc' F0)_j, F0 a force split that carries the base rows of nle) stays at rest: v+ is the
    rounding of b + Jc' F alone, h |M^-1| TERMS eps sum|terms| -- below 1e-10 for h = 2 ms, |M^-1| <= 1e3, sum|terms| <= 1e3"""
    itf, orc = runner.itf, runner.orc
    c = make_case(itf, orc, 5, 15, seed=65, moving=False)
    for i in range(5):
        M, nle, Jf = PR.model_terms(orc, c["rbd"][i])
        F0 = np.linalg.lstsq(Jf[:, :6].T, nle[:6], rcond=None)[0]
        c["tau_ff"][i] = (nle - Jf.T @ F0)[6:]
    got = runner.call(c)
    assert not got["status"].any(), got["status"]
    for i in range(5):
        _, v = PR.coordinates(got["rbd_next"][i])
        assert np.abs(v).max() <= 1e-10 and np.abs(got["rbd_next"][i, :24] - c["rbd"][i, :24]).max() <= 1e-12, (i, np.abs(v).max())


def lock_step(runner, ticks=20, stance_ticks=5, dt=0.002, N=8):
    """batch 2, stance for 5 ticks, then trot; 20 ticks of 2 ms with substeps = 2: MPC once, then per tick policy evaluation -> WBC -> plant.  The plant's input of every tick
    goes to the reference; the single-step outputs are compared by the tolerance rule, so no error accumulates across ticks.  No status bit 0; the base height stays within
    5 cm of its start over the stance ticks."""
    itf, orc, d, h, B = runner.itf, runner.orc, runner.to_dev, runner.to_host, 2
    x0 = S.perturbed_states(itf.initial_state, B, seed=9)
    tgt = S.nominal_target(orc, itf.initial_state)
    nev, ev, md = S.trot_schedule(1.0, phase0=stance_ticks * dt)
    rbd = np.array([S.rbd_from_state(orc, x0[i], np.zeros(24)) for i in range(B)])
    sol = runner.make_solver(B, N)
    o = dict(T=d(np.zeros((B, N + 1))), X=d(np.zeros((B, N + 1, 30))), U=d(np.zeros((B, N, 30))), M=d(np.zeros((B, N + 1), dtype=np.int32)), S=d(np.zeros((B, abi.NSTATS))))
    sol.mpc(sol.mpc_args(B, N, d(x0), d(np.zeros((B, 1))), d(np.tile(tgt, (B, 1, 1))), d(np.full(B, nev, dtype=np.int32)), d(np.tile(ev, (B, 1))), d(np.tile(md, (B, 1))),
                         o["T"], o["X"], o["U"], o["M"], o["S"], t0=d(np.zeros(B))))
    xd, ud, pm = d(np.zeros((B, 30))), d(np.zeros((B, 30))), d(np.zeros(B, dtype=np.int32))
    il, out, wst = d(np.zeros((B, 30))), d(np.zeros((B, 54))), d(np.zeros(B, dtype=np.int32))
    kp = np.zeros((B, 18)); kd = np.tile(np.r_[np.full(12, 3.0), np.full(6, 0.5)], (B, 1))      # QMController::updateControlLaw: legs (0, 3), arm (kp_arm_wbc 0, kd_arm_wbc 0.5)
    height0, worst, modes_seen = rbd[:, 5].copy(), {k: 0.0 for k in PR.KEYS}, set()
    for k in range(ticks):
        t = k * dt
        sol.policy_eval(B, N, o["T"], o["X"], o["U"], o["M"], d(np.full(B, t)), xd, ud, pm)
        sol.wbc(sol.wbc_args(B, d(rbd), d(np.full(B, dt)), d(np.full(B, 20.0 + t)), il, out, wst, xd, ud, pm))
        sol.synchronize()
        xdh, udh, mode, tau = h(xd), h(ud), h(pm), h(out)[:, 36:]
        vel_des = udh[:, 12:30].copy(); vel_des[:, 12:] = 0.0
        c = dict(rbd=rbd, tau_ff=tau, mode=mode, dt=np.full(B, dt), substeps=2, pos_des=xdh[:, 12:30], vel_des=vel_des, kp=kp, kd=kd)
        got = runner.call(c, sol=sol)
        assert not (got["status"] & PR.FAILED).any(), (k, got["status"])
        for i in range(B):
            ref = reference(runner, c, i)
            err = PR.errors(got["rbd_next"][i], got["contact_force"][i], got["tau_applied"][i], int(mode[i]), ref)
            for key in PR.KEYS:
                worst[key] = max(worst[key], err[key] / ref["bound"][key])
                assert err[key] <= ref["bound"][key], (k, i, key, err, ref["bound"])
        modes_seen |= {int(m) for m in mode}
        rbd = got["rbd_next"]
        if k < stance_ticks:
            assert (np.abs(rbd[:, 5] - height0) <= 0.05).all(), (k, rbd[:, 5], height0)
    rec = dict(ticks=ticks, worst_error_over_bound=worst, modes=sorted(modes_seen), height_start=height0.tolist(), height_end=rbd[:, 5].tolist())
    print("lock_step", runner.section, json.dumps(rec))
    record(runner.section, "lock_step", rec)
    assert 15 in modes_seen and len(modes_seen) > 1, modes_seen
    sol.close()


CASES = dict(a=case_a, b=case_b, c=case_c, d=case_d, e=case_e, f=case_f, g=case_g, h=case_h, i=case_i, j=case_j, k=case_k, l=case_l, m=case_m, n=case_n, rest=rest_case)
