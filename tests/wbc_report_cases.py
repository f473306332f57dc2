"""The cases of the WBC solution report (include/qmgpu.h: qmgpu_wbc_report_batch) that test_emu_wbc_report.py runs on the host emulation build and
test_gpu_wbc_report.py on the GPU: seeded robots in motion, the call through api.GpuSolver.wbc_report, the comparison with wbc_report_reference.py under its tolerance
rule, the oracle-free checks and the contracts.  A Runner hides where the arrays live: numpy for the emulated library, torch on the GPU.  The reference's task data of a
set of inputs are computed once (TICKS) and shared by every case that evaluates those inputs.
With WBC_REPORT_RECORD set to a file path every comparison adds its figures there."""
import json
import os

import numpy as np

import support as S
import urdf_model as UM
import wbc_report_reference as WR
from qm_door_amd import abi, api

RECORD = os.environ.get("WBC_REPORT_RECORD") or None
EPS = WR.EPS
MODES = np.array([15, 9, 6, 0, 10, 5, 13, 7, 14, 11], dtype=np.int32)     # the contact modes of gait.info: those support.wbc_stress_batch draws from
ACTIVE_TOL = 1e-6
OUTPUTS = ("eq_residual", "ineq_margin", "tau", "rows", "summary")
SHAPES = dict(eq_residual=(WR.LEVELS, WR.EQ_ROWS), ineq_margin=(WR.INEQ_ROWS,), tau=(18,), rows=(4,), summary=(WR.NSUM,))
TICKS = {}


class Runner:
    def __init__(self, itf, orc, section, to_dev=None, to_host=None, make_solver=None, own_solve=True):
        """own_solve: the x of a solved tick comes from qmgpu_wbc_solve_batch of the library under test (the GPU tier).  False (the emulation tier): from the oracle's
        WBC update of the same tick -- wbc_kernel on host threads costs over a second per robot, and the report is compared with the reference AT THE x IT WAS GIVEN
        either way; a solve handed a solver of its own (the contracts) is always the library's."""
        self.itf, self.orc, self.section, self.own_solve = itf, orc, section, own_solve
        self.to_dev = to_dev or (lambda a: np.ascontiguousarray(a))
        self.to_host = to_host or (lambda a: np.array(a))
        self.make_solver = make_solver or (lambda B, N=4, dtype="f64": api.GpuSolver(self.itf, max_batch=B, max_nodes=N, dtype=dtype))
        self.solvers, self.solutions = {}, {}

    def solver(self, B):
        B = max(B, 8)
        if B not in self.solvers:
            self.solvers[B] = self.make_solver(B)
        return self.solvers[B]

    def _tick_arrays(self, inp, rows):
        pick = lambda a, dt=np.float64: self.to_dev(np.ascontiguousarray(np.asarray(a)[rows], dtype=dt))  # noqa: E731
        return dict(rbd=pick(inp["rbd"]), period=pick(inp["period"]), time=pick(inp["t"]), state_desired=pick(inp["xd"]), input_desired=pick(inp["u"]),
                    mode=pick(inp["mode"], np.int32))

    def solve(self, inp, variant, rows=None, ee_force=None, sol=None):
        """qmgpu_wbc_solve_batch of the tick: (out [B][54], status [B]); the caller's input_last is not touched (the solve gets a copy)"""
        rows = list(range(inp["rbd"].shape[0])) if rows is None else rows
        B = len(rows)
        if not self.own_solve and sol is None:
            r = self.orc.wbc_batch(inp["xd"][rows], inp["u"][rows], inp["rbd"][rows], inp["mode"][rows], inp["period"][rows], inp["t"][rows], inp["il"][rows], variant,
                                   ee_force=None if ee_force is None else ee_force[rows])
            return r["out"], r["status"]
        t = self._tick_arrays(inp, rows)
        il, out, st = self.to_dev(np.ascontiguousarray(inp["il"][rows])), self.to_dev(np.zeros((B, 54))), self.to_dev(np.zeros(B, dtype=np.int32))
        sol = sol or self.solver(B)
        sol.wbc(sol.wbc_args(B, t["rbd"], t["period"], t["time"], il, out, st, t["state_desired"], t["input_desired"], t["mode"], variant=variant,
                             ee_force=None if ee_force is None else self.to_dev(np.ascontiguousarray(ee_force[rows]))))
        sol.synchronize()
        return self.to_host(out), self.to_host(st)

    def solved(self, key, inp, variant):
        """solve() of all of `inp`, once per (key, variant): the cases that evaluate the same ticks share the solver's x"""
        if (key, variant) not in self.solutions:
            self.solutions[(key, variant)] = self.solve(inp, variant)
        return self.solutions[(key, variant)]

    def call(self, inp, variant, x, rows=None, ee_force=None, skip=(), active_tol=ACTIVE_TOL, sol=None, keep=None):
        """one report call on instances `rows` (default: all) at x [B0][36 or 54]; returns the outputs as numpy arrays (those in `skip` passed as NULL and absent).
        Outputs are pre-filled with NaN / -1.  keep (dict): receives the device arrays of input_last and x."""
        rows = list(range(inp["rbd"].shape[0])) if rows is None else rows
        B = len(rows)
        t = self._tick_arrays(inp, rows)
        il, xd = self.to_dev(np.ascontiguousarray(inp["il"][rows])), self.to_dev(np.ascontiguousarray(np.asarray(x)[rows]))
        out = {k: self.to_dev(np.full((B,) + SHAPES[k], -1, dtype=np.int32) if k == "rows" else np.full((B,) + SHAPES[k], np.nan)) for k in OUTPUTS if k not in skip}
        sol = sol or self.solver(B)
        a = sol.wbc_report_args(B, t["rbd"], t["period"], t["time"], il, xd, t["state_desired"], t["input_desired"], t["mode"], variant=variant,
                                ee_force=None if ee_force is None else self.to_dev(np.ascontiguousarray(ee_force[rows])), active_tol=active_tol, **out)
        sol.wbc_report(a)
        sol.synchronize()
        if keep is not None:
            keep.update(il=self.to_host(il), x=self.to_host(xd))
        return {k: self.to_host(v) for k, v in out.items()}


def make_inputs(itf, modes, times, seed, period=0.002):
    """one robot per entry of modes / times near the nominal stance, IN MOTION (measured twist and joint rates, desired joint rates), a non-zero input_last that differs
    from the desired input (so (v_des - input_last) / period is a non-zero joint acceleration), planned forces near the weight shared by the stance feet"""
    rng = np.random.default_rng(seed)
    B = len(modes)
    x_nom, m = itf.initial_state, itf.robot_mass
    xd = x_nom[None, :] + rng.uniform(-1, 1, (B, 30)) * 0.03
    xm = x_nom[None, :] + rng.uniform(-1, 1, (B, 30)) * 0.02
    vm = np.c_[rng.uniform(-0.3, 0.3, (B, 6)), rng.uniform(-0.5, 0.5, (B, 18))]
    u = np.array([S.nominal_input(m, md) for md in modes])
    u[:, :12] += rng.uniform(-1, 1, (B, 12)) * 2.0 * (u[:, :12] != 0)
    u[:, 12:] = rng.uniform(-1, 1, (B, 18)) * 0.1
    il = u + rng.uniform(-1, 1, (B, 30)) * 0.002
    rbd = np.zeros((B, 55))
    rbd[:, 0:3] = xm[:, 9:12]; rbd[:, 3:6] = xm[:, 6:9]; rbd[:, 6:24] = xm[:, 12:30]; rbd[:, 24:48] = vm
    return dict(xd=xd, u=u, rbd=rbd, mode=np.asarray(modes, dtype=np.int32), t=np.asarray(times, dtype=np.float64), il=il, period=np.full(B, period))


def modes_inputs(itf):
    """every contact mode on both sides of t = 10 s: twenty robots (each variant evaluates them: forty instances)"""
    return make_inputs(itf, np.r_[MODES, MODES], np.r_[np.full(len(MODES), 5.0), np.full(len(MODES), 20.0)], seed=71)


def ticks(runner, key, inp, variant):
    """the reference's task data of every instance of `inp` (and of its perturbed draws), computed once per (key, variant)"""
    if (key, variant) not in TICKS:
        TICKS[(key, variant)] = [WR.tick_data(runner.orc, inp, i, variant, seed=i) for i in range(inp["rbd"].shape[0])]
    return TICKS[(key, variant)]


def record(section, name, rec):
    if not RECORD:
        return
    try:
        allrec = json.load(open(RECORD))
    except (OSError, ValueError):
        allrec = {}
    allrec.setdefault(section, {})[name] = rec
    worst = [v for s in allrec.values() if isinstance(s, dict) for r in s.values() if isinstance(r, dict) for v in r.get("worst_fraction_of_bound", {}).values()]
    if worst:
        allrec["worst_fraction_of_bound"] = max(worst)
    os.makedirs(os.path.dirname(os.path.abspath(RECORD)), exist_ok=True)
    json.dump(allrec, open(RECORD, "w"), indent=1)


def check(runner, name, tk, x, got, rows=None):
    """every instance of `got` against the reference at x under the tolerance rule; every figure is printed and recorded before anything is asserted.  Returns the references."""
    rows = list(range(len(tk))) if rows is None else rows
    refs = [WR.report(tk[i], np.asarray(x)[i][:36], ACTIVE_TOL) for i in rows]
    fr = [WR.fractions({k: got[k][j] for k in OUTPUTS}, ref) for j, ref in enumerate(refs)]
    keys = list(fr[0])
    rec = dict(instances=len(rows), worst_fraction_of_bound={k: max(f[k] for f in fr) for k in keys}, separated=int(sum(r["separated"] for r in refs)),
               smallest_bound={k: float(min(r["tol"][k][r["tol"][k] > 0].min() for r in refs)) for k in ("eq_residual", "ineq_margin", "tau")})
    print(name, runner.section, json.dumps(rec))
    record(runner.section, name, rec)
    assert all(np.isfinite(got[k]).all() for k in ("eq_residual", "ineq_margin", "tau")), name
    for j, (f, ref) in enumerate(zip(fr, refs)):
        assert ref["separated"], (name, rows[j], "a margin lies within its tolerance of an active_tol threshold")
        for k in keys:
            assert f[k] <= 1.0, (name, rows[j], k, f)
    return refs


# ------------------------------------------------------------------------------------------------ the cases of the issue's list
def case_modes_variants(runner):
    inp = modes_inputs(runner.itf)
    for variant in (0, 1):
        out, _ = runner.solved("modes", inp, variant)
        assert np.isfinite(out).all()
        check(runner, f"modes_variants_v{variant}", ticks(runner, "modes", inp, variant), out, runner.call(inp, variant, out))


def case_arbitrary_x(runner):
    inp = modes_inputs(runner.itf)
    B = inp["rbd"].shape[0]
    x = np.random.default_rng(72).uniform(-1, 1, (B, 36)) * np.r_[np.full(24, 10.0), np.full(12, 100.0)]
    for variant in (0, 1):
        got = runner.call(inp, variant, x)
        check(runner, f"arbitrary_x_v{variant}", ticks(runner, "modes", inp, variant), x, got)
        assert (got["summary"][:, 0] > 1.0).all() and (got["summary"][:, 3] > 1.0).all()     # nothing like a solution: large residuals


def binding_inputs(runner, want=3, look=64):
    """instances of support.wbc_fast_robots_batch whose torque limits cannot hold: the first `want` of the first `look` for which the ORACLE's solution violates a row
    beyond the active_tol band.  The batch's `velocity` scales measured rates of +-0.1, so joint rates are velocity / 10 rad/s: at its default velocity = 150 (15 rad/s)
    every limit still holds (the first level is feasible, only its starting point is rejected); at velocity = 300 (30 rad/s), used here, a few robots per hundred
    end with a dozen and more limits exceeded by newton metres."""
    b = S.wbc_fast_robots_batch(runner.itf, 0, B=512, velocity=300.0)
    inp = {k: np.asarray(v)[:look] for k, v in dict(xd=b["xd"], u=b["u"], rbd=b["rbd"], mode=b["mode"], t=b["t"], il=b["il"], period=np.full(512, 0.002)).items()}
    ref = runner.orc.wbc_batch(inp["xd"], inp["u"], inp["rbd"], inp["mode"], 0.002, inp["t"], inp["il"], 0)
    chosen = []
    for i in range(look):
        T = runner.orc.wbc_task(0, inp["xd"][i], inp["u"][i], inp["rbd"][i], int(inp["mode"][i]), 0.002, float(inp["t"][i]), inp["il"][i])
        if (T["f"] - T["D"] @ ref["out"][i, :36] < -1e-3).any():
            chosen.append(i)
    assert len(chosen) >= want, chosen
    return {k: np.asarray(v)[chosen[:want]] for k, v in inp.items()}


def case_binding_limits(runner):
    inp = binding_inputs(runner)
    out, _ = runner.solve(inp, 0)
    got = runner.call(inp, 0, out)
    refs = check(runner, "binding_limits", ticks(runner, "binding", inp, 0), out, got)
    for j, ref in enumerate(refs):
        assert got["summary"][j, 8] > 0 and got["summary"][j, 9] > 0 and got["summary"][j, 6] < 0, (j, got["summary"][j])
        neg = ref["ineq_margin"] < 0
        assert neg.any() and (np.abs(got["ineq_margin"][j][neg] - ref["ineq_margin"][neg]) <= ref["tol"]["ineq_margin"][neg]).all(), j


def torque_identity(runner, name, got, refs, limits):
    """margin_i = limit_i - tau_i and margin_{18+i} = limit_i + tau_i: each side is a three-term sum of limit, nle and the row product in another order, so they agree
    within the bounds of the two rows involved (the margin's and the torque's)"""
    for j, ref in enumerate(refs):
        room = ref["tol"]["ineq_margin"][:36] + np.r_[ref["tol"]["tau"], ref["tol"]["tau"]]
        diff = np.abs(got["ineq_margin"][j, :36] - np.r_[limits - got["tau"][j], limits + got["tau"][j]])
        assert (diff <= room).all(), (name, j, float((diff / room).max()))


def case_oracle_free(runner):
    """what the report must say whatever the oracle says: friction rows from x and mu, swing zero-force rows, the torque rows against the URDF's limits, tau against the solve"""
    itf = runner.itf
    inp = modes_inputs(itf)
    mu = itf.problem.settings.wbc_friction_coefficient
    limits = urdf_limits()
    for variant in (0, 1):
        out, _ = runner.solved("modes", inp, variant)
        got = runner.call(inp, variant, out)
        refs = [WR.report(t, out[i, :36], ACTIVE_TOL) for i, t in enumerate(ticks(runner, "modes", inp, variant))]     # for the bounds only
        torque_identity(runner, "oracle_free", got, refs, limits)
        for i in range(inp["rbd"].shape[0]):
            flags = S.contact_flags(int(inp["mode"][i]))
            F = out[i, 24:36].reshape(4, 3)
            row, zero_row = 36, 6 + 3 * sum(flags)
            for c in range(4):
                if flags[c]:
                    fx, fy, fz = F[c]
                    want = np.array([fz, mu * fz - fx, mu * fz + fx, mu * fz - fy, mu * fz + fy])
                    room = WR.FACTOR * 3 * EPS * np.array([abs(fz), mu * abs(fz) + abs(fx), mu * abs(fz) + abs(fx), mu * abs(fz) + abs(fy), mu * abs(fz) + abs(fy)])
                    assert (np.abs(got["ineq_margin"][i, row:row + 5] - want) <= room).all(), (variant, i, c)
                    row += 5
            for c in range(4):
                if not flags[c]:
                    assert np.array_equal(got["eq_residual"][i, 0, zero_row:zero_row + 3], F[c]), (variant, i, c)      # 1 * F - 0: exact
                    zero_row += 3
            assert not got["ineq_margin"][i, row:].any()                                                                   # the all-zero rows and the rows beyond m_0
            assert (np.abs(got["tau"][i] - out[i, 36:]) <= refs[i]["tol"]["tau"]).all(), (variant, i)


def urdf_limits():
    """effort limits of the 18 joints parsed from the URDF by tests/urdf_model.py, the first leg's three applied to every leg (WbcBase.cpp:599-600)"""
    import xml.etree.ElementTree as ET
    effort = {j.get("name"): float(j.find("limit").get("effort")) for j in ET.parse(UM.URDF).getroot().findall("joint") if j.find("limit") is not None}
    lim = np.array([effort[name] for name in UM.JOINT_ORDER])
    return np.r_[np.tile(lim[:3], 4), lim[12:18]]


def case_ee_force(runner):
    """a non-NULL external force on the end-effector (the oracle's wbc_task takes none): at the solver's own x under that force the equations of motion hold, tau is the
    solver's, the torque rows keep their identity; the same tick evaluated without the force does not"""
    inp = make_inputs(runner.itf, np.array([15, 9, 6, 13, 0], dtype=np.int32), np.full(5, 20.0), seed=75)
    force = np.random.default_rng(75).uniform(-20, 20, (5, 3))
    force[np.abs(force) < 5.0] += 10.0
    out, _ = runner.solve(inp, 0, ee_force=force)
    got = runner.call(inp, 0, out, ee_force=force)
    bare = runner.call(inp, 0, out)
    refs = [WR.report(t, out[i, :36], ACTIVE_TOL) for i, t in enumerate(ticks(runner, "ee_force", inp, 0))]                # the force-free reference: for the bounds only
    torque_identity(runner, "ee_force", got, refs, urdf_limits())
    worst = []
    for i, ref in enumerate(refs):
        bound = ref["tol"]["eq_residual"][0, :6].max()                      # the bound of the equation-of-motion rows of this instance
        worst.append((float(got["summary"][i, 3]), float(bound), float(np.abs(got["eq_residual"][i, 0] - bare["eq_residual"][i, 0]).max())))
    print("ee_force", runner.section, json.dumps(dict(level0_inf_norm_bound_difference=worst)))
    record(runner.section, "ee_force", dict(level0_inf_norm_bound_difference=worst))
    for i, ref in enumerate(refs):
        assert (np.abs(got["tau"][i] - out[i, 36:]) <= ref["tol"]["tau"]).all(), i
        assert worst[i][0] <= worst[i][1], (i, worst[i])
        assert worst[i][2] > worst[i][1] and np.abs(got["tau"][i] - bare["tau"][i]).max() > ref["tol"]["tau"].max(), (i, worst[i])


def same_bits(a, b, keys=OUTPUTS):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys if k in a and k in b)


def case_contracts(runner):
    import pytest
    itf = runner.itf
    modes = np.resize(MODES, 65)
    inp = make_inputs(itf, modes, np.where(np.arange(65) % 3 == 0, 5.0, 20.0), seed=76)
    x = np.random.default_rng(76).uniform(-1, 1, (65, 36)) * np.r_[np.full(24, 10.0), np.full(12, 100.0)]
    sol = runner.solver(65)
    keep = {}
    full = runner.call(inp, 0, x, sol=sol, keep=keep)
    assert np.array_equal(keep["il"], inp["il"]) and np.array_equal(keep["x"], x)                    # input_last and x are unchanged by the call
    assert all(np.isfinite(full[k]).all() for k in ("eq_residual", "ineq_margin", "tau")) and (full["rows"] >= 0).all()
    for i in (0, 7, 64):                                                                             # batch = 1: an instance alone, bit for bit
        one = runner.call(inp, 0, x, rows=[i], sol=sol)
        assert all(np.array_equal(one[k][0], full[k][i]) for k in OUTPUTS), i
    for k in OUTPUTS:                                                                                # every optional output NULL in turn
        part = runner.call(inp, 0, x, skip=(k,), sol=sol)
        assert k not in part and same_bits(part, full)
    wide = np.c_[x, np.full((65, 18), np.nan)]                                                       # x_stride 54 against 36
    assert same_bits(runner.call(inp, 0, wide, sol=sol), full)
    for i in range(65):                                                                              # rows against the host's row map
        assert list(full["rows"][i]) == api.wbc_report_layout(0, int(modes[i]), inp["t"][i] < 10.0, lib=itf.lib)[1], i
    sub = list(range(8))
    first = runner.solve(inp, 0, rows=sub[:2], sol=sol)                                              # a solve, a report, the same solve again
    runner.call(inp, 0, x, sol=sol)
    second = runner.solve(inp, 0, rows=sub[:2], sol=sol)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1]) and first[0][:, 36:].any()

    d = runner.to_dev
    t = runner._tick_arrays(inp, sub)
    base = dict(batch=8, rbd=t["rbd"], period=t["period"], time=t["time"], input_last=d(inp["il"][sub]), x=d(x[sub]), state_desired=t["state_desired"],
                input_desired=t["input_desired"], mode=t["mode"], summary=d(np.zeros((8, 12))))

    def refused(s, **change):
        kw = dict(base); kw.update(change)
        with pytest.raises(abi.QmGpuError) as e:
            s.wbc_report(s.wbc_report_args(**kw))
        assert e.value.status == abi.ERR_INVALID_ARGUMENT and str(e.value), change
    small = runner.make_solver(8)
    refused(small, batch=9); refused(small, batch=0); refused(small, batch=-1)
    for k in ("rbd", "period", "time", "input_last", "x", "state_desired", "input_desired", "mode"):
        refused(small, **{k: None}, **({"x_stride": 36} if k == "x" else {}))
    refused(small, variant=2); refused(small, variant=-1); refused(small, x_stride=35); refused(small, x_stride=0); refused(small, x_stride=55)
    f32 = runner.make_solver(8, dtype="f32")
    refused(f32)
    f32.close()
    assert itf.lib.qmgpu_wbc_report_batch(small.handle, None) == abi.ERR_INVALID_ARGUMENT
    small.wbc_report(small.wbc_report_args(**base))
    small.synchronize()
    small.close()


def lock_step(runner, ticks_=3, B=8, N=8, dt=0.002):
    """three ticks of qmgpu_cycle_batch for eight robots with a report of each tick's out; each tick is compared on its own with the reference at the policy's desired
    state and input, the input_last the tick started from and the tick's own x"""
    itf, orc, d, h = runner.itf, runner.orc, runner.to_dev, runner.to_host
    x0 = S.perturbed_states(itf.initial_state, B, seed=9)
    mv = S.moving_inputs(orc, x0, itf.problem.settings.dt, seed=13)
    tgt = S.nominal_target(orc, itf.initial_state)
    nev, ev, md = S.trot_schedule(1.0, phase0=0.003)
    sol = runner.make_solver(B, N)
    o = dict(T=d(np.zeros((B, N + 1))), X=d(np.zeros((B, N + 1, 30))), U=d(np.zeros((B, N, 30))), M=d(np.zeros((B, N + 1), dtype=np.int32)), S=d(np.zeros((B, abi.NSTATS))))
    xd, ud, pm = d(np.zeros((B, 30))), d(np.zeros((B, 30))), d(np.zeros(B, dtype=np.int32))
    il, out, wst = d(mv["input_last"]), d(np.zeros((B, 54))), d(np.zeros(B, dtype=np.int32))
    rbd, period = d(mv["rbd"]), d(np.full(B, dt))
    rep = dict(eq_residual=d(np.zeros((B, 3, 22))), ineq_margin=d(np.zeros((B, 56))), tau=d(np.zeros((B, 18))), rows=d(np.zeros((B, 4), dtype=np.int32)), summary=d(np.zeros((B, 12))))
    for k in range(ticks_):
        t = k * dt
        time = d(np.full(B, 20.0 + t))
        il_before = d(h(il).copy())
        a = sol.mpc_args(B, N, d(mv["x0"]), d(np.zeros((B, 1))), d(np.tile(tgt, (B, 1, 1))), d(np.full(B, nev, dtype=np.int32)), d(np.tile(ev, (B, 1))), d(np.tile(md, (B, 1))),
                         o["T"], o["X"], o["U"], o["M"], o["S"], t0=d(np.full(B, t)))
        sol.cycle(a, d(np.full(B, t + 0.4 * dt)), sol.wbc_args(B, rbd, period, time, il, out, wst))
        # the desired state and input the cycle handed its WBC: the policy of the solve at the same time
        sol.policy_eval(B, N, o["T"], o["X"], o["U"], o["M"], d(np.full(B, t + 0.4 * dt)), xd, ud, pm)
        sol.wbc_report(sol.wbc_report_args(B, rbd, period, time, il_before, out, xd, ud, pm, variant=0, active_tol=ACTIVE_TOL, **rep))
        sol.synchronize()
        inp = dict(xd=h(xd), u=h(ud), rbd=mv["rbd"], mode=h(pm), t=np.full(B, 20.0 + t), il=h(il_before), period=np.full(B, dt))
        assert np.array_equal(h(il), inp["u"])                                  # the policy evaluated here is the one the cycle's WBC saw (it left it in input_last)
        outh = h(out)
        got = {k_: h(v) for k_, v in rep.items()}
        refs = check(runner, f"lock_step_tick{k}", [WR.tick_data(orc, inp, i, 0, seed=i) for i in range(B)], outh, got)
        for i, ref in enumerate(refs):
            assert (np.abs(got["tau"][i] - outh[i, 36:]) <= ref["tol"]["tau"]).all(), (k, i)
    sol.close()


CASES = dict(modes_variants=case_modes_variants, arbitrary_x=case_arbitrary_x, binding_limits=case_binding_limits, oracle_free=case_oracle_free, ee_force=case_ee_force,
             contracts=case_contracts)
