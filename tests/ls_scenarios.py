"""Scenarios of the line-search pin (ls_reference.py), shared by the CPU tier (test_ls_reference.py: oracle and host-emulated kernels) and the GPU tier
(test_gpu_ls.py).  Every iterate and target is built with the reference's own kinematics and schedule rules (lq_reference, lq_scenarios' helpers) -- no oracle, no
kernel-derived helper.  The constants (target scales, displacements, settings values) were searched with the oracle; what they were chosen for is asserted on the
reference alone (assert_coverage), together with the decision margin of every comparison the reference's filter and convergence test evaluated (assert_margin).

A scenario is a list of cases; a case is one settings variant = one solver handle = one batch of one call (two calls: across_calls).  The instances of a batch are
given as a list of DISTINCT instances and a layout (batch index -> distinct instance); the reference is computed once per distinct instance and process.

Direction of the reference: kkt_reference.solve of lq_reference.lq_node at every node (35 ms per node), except where a case says direction = "dump" (N = 300): there
it is kkt_reference.solve of the solver's own dumped blocks, which test_gpu_lq.py / test_gpu_kkt.py pin.  The Armijo metric is upstream's (ls_reference.armijo_metric) from the same blocks and step."""
import time

import numpy as np

import kkt_reference as KR
import lq_reference as LR
import ls_reference as LSR
from lq_scenarios import ee_pose, pad_schedule, trot_schedule
from qm_door_amd import api

BAR = 1e-10              # the project's LQ bar: |got - ref| <= 1e-10 max(1, |ref|) (merits, Armijo metric)
FP32_BAR = 1e-4          # the project's fp32 bar, relative (merits and violations of the fp32 leg)
MARGIN, FP32_MARGIN = 1e-6, 1e-3
STEP_FACTOR = 10.0       # kkt_scenarios' tolerance rule: 10 x the larger of the oracle's and a plain LU's step error against the refined reference


class Inst:
    def __init__(self, x0, tt, ts, sched, grid, X, U, expect):
        self.x0, self.tt, self.ts, self.grid, self.X, self.U, self.expect = (np.array(x0, float), np.atleast_1d(np.array(tt, float)), np.atleast_2d(np.array(ts, float)),
                                                                            np.array(grid, float), np.array(X, float), np.array(U, float), expect)
        self.sched = sched
        self.nev, self.ev, self.md = sched
        assert np.array_equal(self.X[0], self.x0)

    @property
    def schedule(self):
        return self.ev[:self.nev], self.md[:self.nev + 1]


class Case:
    def __init__(self, name, N, instances, layout=None, settings=None, line_search=True, direction="reference", cus=None):
        self.name, self.N, self.instances, self.settings, self.line_search, self.direction = name, N, instances, dict(settings or {}), line_search, direction
        self.layout = list(range(len(instances))) if layout is None else list(layout)
        self.B, self.cus = len(self.layout), cus
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        pick = lambda attr: [getattr(instances[j], attr) for j in self.layout]  # noqa: E731
        self.x0, self.tt, self.ts, self.grid, self.X, self.U, self.ev = (f64(pick(a)) for a in ("x0", "tt", "ts", "grid", "X", "U", "ev"))
        self.nev, self.md = np.ascontiguousarray(pick("nev"), dtype=np.int32), np.ascontiguousarray(pick("md"), dtype=np.int32)
        assert self.X.shape == (self.B, N + 1, 30) and self.U.shape == (self.B, N, 30) and (self.B <= 8 or cus is not None)


# ------------------------------------------------------------------------------------------------ iterates and targets
_settled = {}


def nominal_knot(P):
    pos, q = ee_pose(P.initial_state)
    return np.r_[P.initial_state, pos, q]


def far_target(P, scale):
    """the target of support.rejected_full_step_batch: base 0.5 m and 0.5 rad, arm joints 0.3 rad, end-effector 0.6 m away, times `scale`"""
    ts = nominal_knot(P)
    ts[6:9] += scale * np.array([0.5, 0.3, 0.05]); ts[9] += scale * 0.5; ts[24:30] += scale * 0.3; ts[30:33] += scale * np.array([0.5, 0.3, 0.2])
    return ts


def held_stance(P, grid, sched):
    """the nominal stance held over the horizon with the weight compensation of every node's mode: a deliberately poor warm start under a trot schedule"""
    N = len(grid) - 1
    X = np.tile(P.initial_state, (N + 1, 1))
    U = np.array([LR.nominal_input(P, LR.node_mode(sched[1][:sched[0]], sched[2], grid[k])) for k in range(N)])
    return X, U


def backoff_instance(P, N, scale, expect, phase0=0.03):
    grid = np.arange(N + 1) * P.dt
    sched = trot_schedule(N * P.dt + 1.0, phase0=phase0)
    X, U = held_stance(P, grid, sched)
    return Inst(P.initial_state, [0.0], far_target(P, scale), sched, grid, X, U, expect)


def balanced_forces(P, x):
    """normal forces of the four stance feet that carry the weight with no moment about the centre of mass (least norm): the standing robot stays where it is"""
    k = LR.kinematics(x[None, 6:30])
    r = (k["feet"][0] - k["com"][0]).real
    A = np.vstack([np.ones(4), r[:, 1], -r[:, 0]])            # sum f_z = m g; moment of f_z e_z about x and about y = 0
    fz = np.linalg.lstsq(A, np.array([LR.MASS * P.gravity, 0.0, 0.0]), rcond=None)[0]
    u = np.zeros(30); u[2:12:3] = fz
    return u


def feasible_instance(P, N, displacement, expect):
    """An all-stance standing robot rolled out through the reference's rk2 (defects and stance rows at rounding level: viol0 < g_min) and a target `displacement`
    (base x, y, yaw and the end-effector with it) away"""
    grid = np.arange(N + 1) * P.dt
    sched = pad_schedule([20 * (N + 1) * P.dt], [15, 15])
    u = balanced_forces(P, P.initial_state)
    X = [P.initial_state.copy()]
    for k in range(N):
        X.append(LR.rk2(X[-1][None, :].astype(complex), u[None, :].astype(complex), P.dt, P.gravity)[0][0].real)
    ts = nominal_knot(P)
    ts[6:8] += displacement * np.array([1.0, 0.6]); ts[9] += displacement; ts[30:32] += displacement * np.array([1.0, 0.6])
    return Inst(P.initial_state, [0.0], ts, sched, grid, np.array(X), np.tile(u, (N, 1)), expect)


def settled_instance(P, N, displacement, expect, iterations=3):
    """The feasible iterate brought to rest: full reference SQP steps (lq_reference blocks, kkt_reference.solve, alpha = 1) from the standing robot towards the nominal
    target, then the inputs rolled out through the reference's rk2 once more, and only then the target moved by `displacement`.  The relaxed barriers on the arm
    joints and the friction cones are not stationary at the standing pose (its first step leaves a violation of 5e-4 whatever the target); at the settled iterate
    the step is the displacement's alone, small enough for v1 < g_min at the task file's g_min."""
    if (N, displacement, iterations) in _settled:
        i = _settled[(N, displacement, iterations)]
        return Inst(i.x0, i.tt, i.ts, i.sched, i.grid, i.X, i.U, expect)
    inst = feasible_instance(P, N, 0.0, expect)
    ev, md = inst.schedule
    X, U = inst.X, inst.U
    for _ in range(iterations):
        d = KR.solve([LR.lq_node(P, **LSR.node_args(inst.grid, X, U, ev, md, inst.tt, inst.ts, k)) for k in range(N + 1)])
        X, U = X + d["dX"], U + d["dU"]
    X = [P.initial_state.copy()]
    for k in range(N):
        X.append(LR.rk2(X[-1][None, :].astype(complex), U[k][None, :].astype(complex), P.dt, P.gravity)[0][0].real)
    ts = nominal_knot(P)
    ts[6:8] += displacement * np.array([1.0, 0.6]); ts[9] += displacement; ts[30:32] += displacement * np.array([1.0, 0.6])
    _settled[(N, displacement, iterations)] = Inst(P.initial_state, [0.0], ts, inst.sched, inst.grid, np.array(X), U, expect)
    return _settled[(N, displacement, iterations)]


def defect_instance(P, N, seed, sigma, expect, target_scale=0.0, grid=None, phase0=0.03):
    """the held stance with seeded defects (states) and perturbed forces and joint rates: an infeasible iterate near its target"""
    rng = np.random.default_rng(seed)
    grid = np.arange(N + 1) * P.dt if grid is None else grid
    sched = trot_schedule(grid[-1] + 1.0, phase0=phase0)
    X, U = held_stance(P, grid, sched)
    X[1:] += sigma * rng.standard_normal(X[1:].shape)
    U += sigma * rng.standard_normal(U.shape) * np.r_[np.full(12, 200.0), np.full(18, 10.0)]
    return Inst(P.initial_state, [0.0], far_target(P, target_scale), sched, grid, X, U, expect)


# ------------------------------------------------------------------------------------------------ the scenarios
SQP5 = dict(sqp_iterations=5)
G_MIN_RAISED = 1e-2      # above the 5e-4 the standing robot's first step leaves as violation (see type3_armijo)


def _backoffs(P, N, scales, expects):
    return [backoff_instance(P, N, s, e) for s, e in zip(scales, expects)]


LADDER = [dict(alpha=1.0), dict(alpha=0.5, first_rejected=True), dict(alpha=0.25, first_rejected=True), dict(alpha_max=0.125, first_rejected=True)]


def backoff_two_trials(P):
    """accepted alpha 1, 1/2, 1/4 and <= 1/8 in one batch, N = 7: 256 threads, two trials side by side, second and third pass of the trial loop"""
    return [Case("backoff_two_trials", 7, _backoffs(P, 7, (0.5, 1.0, 2.0, 4.0), LADDER))]


def backoff_one_trial(P):
    """N = 130: one trial per pass, its slice in LDS; alpha 1/2 (second pass) and <= 1/8 (fourth pass).  Two instances only: the reference takes 7 .. 11 s for each."""
    return [Case("backoff_one_trial", 130, _backoffs(P, 130, (2.0, 6.0), [LADDER[1], LADDER[3]]))]


def backoff_hbm_scratch(P):
    """N = 300: the trial slice in HBM, several nodes per thread; direction from the solver's dumped blocks"""
    e = dict(first_rejected=True, viol0_above_g_min=True)
    return [Case("backoff_hbm_scratch", 300, _backoffs(P, 300, (2.0, 4.0), [dict(e, alpha=0.5), dict(e, alpha=0.25)]), direction="dump")]


def backoff_128_threads(P):
    """B = 300 > 256 CUs: the 128-thread launch, one trial per pass (N = 70) and two trials (N = 7); the rejecting instances at batch indices 0, 150 and 299, every
    other instance a copy of one that accepts the full step"""
    layout = [0] * 300
    layout[0], layout[150], layout[299] = 1, 2, 3
    rej = [dict(alpha=1.0)] + [dict(first_rejected=True)] * 3
    return [Case("backoff_128_threads_N70", 70, _backoffs(P, 70, (0.5, 2.0, 3.0, 6.0), rej), layout=layout, cus=2),
            Case("backoff_128_threads_N7", 7, _backoffs(P, 7, (0.5, 1.0, 2.0, 4.0), rej), layout=layout, cus=2)]


def type1_constraint(P):
    """g_max lowered below the trial's violation: type 1 accepted at once (the violation falls) and rejected, then accepted"""
    return [Case("type1_constraint", 7, [defect_instance(P, 7, 0, 1e-3, dict(alpha=1.0, type=1)), backoff_instance(P, 7, 1.0, dict(alpha=0.5, type=1, trail=[(1.0, 1, False), (0.5, 1, True)]))],
                 settings=dict(g_max=1e-3)),
            # gamma_c raised: a trial whose violation falls, but by less than the factor (1 - gamma_c), is rejected (at the default 1e-6 that band is empty)
            Case("type1_gamma_c", 7, [backoff_instance(P, 7, 0.5, dict(first_rejected=True, type=1, v1_in_gamma_band=True))], settings=dict(g_max=1e-3, gamma_c=0.5))]


SETTLED = 3e-4           # target displacement of the settled iterate at which v1 = 4.9e-7 < g_min = 1e-6 (v1 grows with its square: 5.4e-6 at 1e-3)


def type3_armijo(P):
    """The feasible iterate at rest (settled_instance: viol0 = 1.5e-9) and a target 0.3 mm away, at the task file's g_min = 1e-6: type 3 accepted at alpha = 1;
    with armijo_factor = 0.6 > 1/2 the Armijo inequality fails at alpha = 1 and holds at alpha = 1/2.  Third variant: the standing robot itself (viol0 = 1.6e-16,
    first step leaves 5.5e-4) with g_min raised to 1e-2."""
    t3 = dict(type=3, viol0_below_g_min=True, v1_below_g_min=True)
    return [Case("type3_accepted", 7, [settled_instance(P, 7, SETTLED, dict(t3, alpha=1.0))]),
            Case("type3_rejected_once", 7, [settled_instance(P, 7, SETTLED, dict(t3, alpha=0.5, trail=[(1.0, 3, False), (0.5, 3, True)]))], settings=dict(armijo_factor=0.6)),
            Case("type3_g_min_raised", 7, [feasible_instance(P, 7, 1e-3, dict(t3, alpha=1.0))], settings=dict(g_min=G_MIN_RAISED))]


def type2_either_clause(P):
    """type 2 accepted by the merit clause only (feasible iterate: the violation can only rise) and by the violation clause only (defects near the target: the
    cost rises); g_max raised so that neither is type 1"""
    return [Case("type2_either_clause", 7, [feasible_instance(P, 7, 1e-3, dict(alpha=1.0, type=2, clauses=(True, False))),
                                          defect_instance(P, 7, 0, 1e-3, dict(alpha=1.0, type=2, clauses=(False, True)))], settings=dict(g_max=1e3))]


def alpha_min_stops(P):
    """alpha_min 0.3: an instance that needs alpha = 1/4 stops after two trials: type 4, alpha 0, the iterate untouched.  alpha_min 0.6: an instance whose alpha = 1/2
    trial would be accepted (backoff_two_trials, instance 1) must not take it: that trial is evaluated side by side but lies behind the end of the sequential loop."""
    stop = dict(alpha=0.0, type=4, untouched=True)
    return [Case("alpha_min_0.3", 7, [backoff_instance(P, 7, 2.0, dict(stop, trials=2))], settings=dict(alpha_min=0.3)),
            Case("alpha_min_0.6", 7, [backoff_instance(P, 7, 1.0, dict(stop, trials=1))], settings=dict(alpha_min=0.6))]


DENSE_Q = (6, 7, 0.3)    # Q[6][7] = Q[7][6] = 0.3 sqrt(Q[6][6] Q[7][7]): one off-diagonal entry of the symmetric weight, Q stays positive definite


def dense_weights(P):
    """one off-diagonal entry of Q: the dense forms of the node evaluation, behind a rejected step"""
    return [Case("dense_weights", 7, _backoffs(P, 7, (1.0, 2.0), [dict(first_rejected=True)] * 2), settings=dict(dense_q=DENSE_Q))]


def line_search_off(P):
    """type 0 and alpha 1 on an instance the filter rejects (backoff_two_trials, instance 2)"""
    return [Case("line_search_off", 7, [backoff_instance(P, 7, 2.0, dict(alpha=1.0, type=0))], line_search=False)]


def convergence_reasons(P):
    """sqp_iterations = 5, the outcome of the first iteration: each reason on its own, no reason (the call runs on), and the two precedences; all but reason 2 alone
    on the settled iterate at the task file's g_min, steered by alpha_min, cost_tol and delta_tol.  The instance that runs on is solved a second time with
    sqp_iterations = 1, where its first iteration is the call's outcome and is checked in full."""
    near, far = (lambda e: [settled_instance(P, 7, SETTLED, e)]), (lambda e: [settled_instance(P, 7, 1e-3, e)])  # noqa: E731
    return [Case("reason_2", 7, [backoff_instance(P, 7, 1.0, dict(reason=2, holds={2}, holds_not={3}))], settings=dict(SQP5, alpha_min=0.6)),
            Case("reason_3", 7, near(dict(reason=3, holds={3}, holds_not={2, 4})), settings=dict(SQP5, cost_tol=1e3)),
            Case("reason_4", 7, far(dict(reason=4, holds={4}, holds_not={2, 3})), settings=dict(SQP5, delta_tol=1e3)),
            Case("reason_0", 7, far(dict(reason=0, holds=set(), holds_not={1, 2, 3, 4})), settings=dict(SQP5)),
            Case("reason_0_first_iteration", 7, far(dict(reason=1, alpha=1.0, type=2))),
            Case("reason_2_over_3", 7, near(dict(reason=2, holds={2, 3}, alpha=0.0, type=4)), settings=dict(SQP5, armijo_factor=0.9, alpha_min=0.3)),
            Case("reason_3_over_4", 7, near(dict(reason=3, holds={3, 4}, holds_not={2})), settings=dict(SQP5, cost_tol=1e3, delta_tol=1e3))]


def across_calls(P):
    """trot with events inside the horizon, defects in the warm start: call A (one iteration), call B warm-started at A's result"""
    return [Case("across_calls_N7", 7, [defect_instance(P, 7, 5, 1e-3, {}, 0.25), defect_instance(P, 7, 6, 1e-2, {}, 1.0)]),
            Case("across_calls_N130", 130, [defect_instance(P, 130, 7, 1e-3, {}, 0.25)])]


BUILDERS = {f.__name__: f for f in (backoff_two_trials, backoff_one_trial, backoff_hbm_scratch, backoff_128_threads, type1_constraint, type3_armijo, type2_either_clause,
                                    alpha_min_stops, dense_weights, line_search_off, convergence_reasons, across_calls)}
FP32_SCENARIOS = ("backoff_two_trials", "type1_constraint")
_cache = {}


# ------------------------------------------------------------------------------------------------ settings variants, reference, conditions
def interface_of(interface, case):
    """a second interface on the same library with the case's settings (a settings update before the handle is made)"""
    key = ("itf", id(interface.lib), case.name)
    if key not in _cache:
        itf = api.QMInterface(lib=interface.lib)
        for name, value in case.settings.items():
            if name == "dense_q":
                i, j, f = value
                itf.problem.settings.Q[i * 30 + j] = itf.problem.settings.Q[j * 30 + i] = f * np.sqrt(itf.problem.settings.Q[i * 31] * itf.problem.settings.Q[j * 31])
            else:
                setattr(itf.problem.settings, name, value)
        _cache[key] = itf
    return _cache[key]


def base_params(interface):
    if "P" not in _cache:
        _cache["P"] = LSR.Params(interface.problem.settings)
    return _cache["P"]


def cases(interface, name):
    if ("cases", name) not in _cache:
        _cache[("cases", name)] = BUILDERS[name](base_params(interface))
    return _cache[("cases", name)]


def reference_blocks(P, inst):
    ev, md = inst.schedule
    return [LR.lq_node(P, **LSR.node_args(inst.grid, inst.X, inst.U, ev, md, inst.tt, inst.ts, k)) for k in range(len(inst.grid))]


def reference_of(P, case, inst, blocks=None, iteration_index=0):
    """the reference's iteration of one instance: direction (from `blocks`, by default the reference's own), Armijo metric, line search, convergence"""
    ev, md = inst.schedule
    t0 = time.perf_counter()
    blocks = reference_blocks(P, inst) if blocks is None else blocks
    d = KR.solve(blocks)
    armijo = LSR.armijo_metric(blocks, d["dX"], d["dU"])
    it = LSR.iteration(P, inst.grid, inst.X, inst.U, ev, md, inst.tt, inst.ts, d["dX"], d["dU"], armijo, case.line_search, iteration_index)
    it.update(d=d, armijo=armijo, armijo_unprojected=LSR.armijo_metric(blocks, d["dX"], d["dU"], projected=False), e_lu=(KR.rel_err(d["dX_lu"], d["dX"]), KR.rel_err(d["dU_lu"], d["dU"])), seconds=time.perf_counter() - t0)
    return it


def references(interface, case, blocks_of=None):
    """[reference of every DISTINCT instance], once per process (direction "dump": per caller, from blocks_of(distinct index) -> blocks of a batch index holding it)"""
    P = LSR.Params(interface_of(interface, case).problem.settings)
    if case.direction == "dump":
        return [reference_of(P, case, inst, blocks_of(case.layout.index(j))) for j, inst in enumerate(case.instances)]
    key = ("ref", id(interface.lib), case.name, tuple(sorted(case.settings.items())))
    if key not in _cache:
        _cache[key] = [reference_of(P, case, inst) for inst in case.instances]
    return _cache[key]


def assert_coverage(case, inst, r, P):
    """the reference reaches what the instance was chosen for; P: the reference's parameters of the case (its own g_min, gamma_c)"""
    e, ls, tag = inst.expect, r["ls"], (case.name, inst.expect)
    trail = [(a, k, ok) for a, k, ok, *_ in ls["trail"]]
    if "alpha" in e:
        assert ls["alpha"] == e["alpha"], (tag, trail)
    if "alpha_max" in e:
        assert 0.0 < ls["alpha"] <= e["alpha_max"], (tag, trail)
    if "type" in e:
        assert ls["type"] == e["type"], (tag, trail)
    if e.get("first_rejected"):
        assert not trail[0][2] and ls["alpha"] > 0.0, (tag, trail)
    if "trail" in e:
        assert trail == e["trail"], (tag, trail)
    if "trials" in e:
        assert len(trail) == e["trials"] and not any(ok for _, _, ok in trail), (tag, trail)
    if "clauses" in e:
        assert tuple(ls["trail"][-1][5:7]) == e["clauses"], (tag, ls["trail"][-1])
    if e.get("viol0_above_g_min"):
        assert r["base"][1] > P.g_min, (tag, r["base"])
    if e.get("viol0_below_g_min"):
        assert r["base"][1] < P.g_min, (tag, r["base"])
    if e.get("v1_below_g_min"):
        assert all(v1 < P.g_min for _, _, _, _, v1, *_ in ls["trail"]), (tag, ls["trail"])
    if e.get("v1_in_gamma_band"):
        assert (1.0 - P.gamma_c) * r["base"][1] <= ls["trail"][0][4] < r["base"][1], (tag, ls["trail"][0], r["base"])
    if "reason" in e:
        assert r["reason"] == e["reason"], (tag, r["reason"], r["conditions"])
    assert all(r["conditions"][c] for c in e.get("holds", ())) and not any(r["conditions"][c] for c in e.get("holds_not", ())), (tag, r["conditions"])
    if e.get("untouched"):
        assert np.array_equal(r["X"], inst.X) and np.array_equal(r["U"], inst.U)


def case_params(interface, case):
    return LSR.Params(interface_of(interface, case).problem.settings)


def assert_conditions(interface, case, refs, margin=MARGIN):
    """coverage and margin of every distinct instance of a case"""
    P = case_params(interface, case)
    for inst, r in zip(case.instances, refs):
        assert_coverage(case, inst, r, P)
        assert_margin(case, r, margin)


def assert_margin(case, r, margin=MARGIN):
    m = LSR.margin(r["comparisons"])
    assert m >= margin, (case.name, m, [c for c in r["comparisons"] if LSR.margin([c]) < margin])
    return m


# ------------------------------------------------------------------------------------------------ solving a case, checking an outcome
def solve_device(G, interface, case, dtype="f64", warm=None, debug=False):
    """one call of the case on the harness' device (the GPU tier): (out, solver)"""
    sol = G.make_solver(interface_of(interface, case), case.B, case.N, dtype=dtype)
    if debug:
        sol.enable_debug(True)
    X, U = (case.X, case.U) if warm is None else warm
    mb = G.MpcBatch(case.x0, case.tt, case.ts, case.nev, case.ev, case.md, case.N, warm=(X, U), line_search=case.line_search)
    sol.mpc(mb.args)
    return mb.results(), sol


def host_sized(case):
    """the case as the host emulation runs it: the 300-instance batch at N = 7 as it is (rejecting instances at 0, 150, 299); the one at N = 70
    (21,300 nodes: more than ten minutes on host threads, profiles/ls_reference.md) cut to 8 instances with the rejecting ones at 0, 4 and 7 -- with QMGPU_EMU_CUS = 2
    still a batch beyond the CUs, so the 128-thread one-trial launch is taken; the device runs all 300"""
    if case.B <= 8 or case.N <= 7:
        return case
    layout = [0] * 8
    layout[0], layout[4], layout[7] = 1, 2, 3
    return Case(case.name, case.N, case.instances, layout=layout, settings=case.settings, line_search=case.line_search, direction=case.direction, cus=case.cus)


def solve_host(emu_interface, case, dtype="f64", warm=None, debug=False):
    """the same call on the host-emulated kernels (the CPU tier); case.cus: the emulated device's CU count while the handle is made"""
    import os
    from qm_door_amd import abi
    B, N = case.B, case.N
    if case.cus is not None:
        os.environ["QMGPU_EMU_CUS"] = str(case.cus)
    try:
        sol = api.GpuSolver(interface_of(emu_interface, case), max_batch=B, max_nodes=N, dtype=dtype)
    finally:
        os.environ.pop("QMGPU_EMU_CUS", None)
    if debug:
        sol.enable_debug(True)
    X, U = (case.X, case.U) if warm is None else warm
    oT, oX, oU, oM, oS = np.zeros((B, N + 1)), np.zeros((B, N + 1, 30)), np.zeros((B, N, 30)), np.zeros((B, N + 1), dtype=np.int32), np.zeros((B, abi.NSTATS))
    sol.mpc(sol.mpc_args(B, N, case.x0, case.tt, case.ts, case.nev, case.ev, case.md, oT, oX, oU, oM, oS, t0=np.zeros(B), warm_x=np.ascontiguousarray(X), warm_u=np.ascontiguousarray(U),
                         line_search=case.line_search))
    return dict(T=oT, X=oX, U=oU, mode=oM, stats=oS), sol


def dump_blocks(sol, case):
    return lambda i: [sol.debug_lq(i, k) for k in range(case.N + 1)]


def violation_bound(ref):
    """allowed |got - ref| of a violation: 10 x the reference's own relative error times ref, never less than the LQ bar where ref >= 1e-3, and never less than 10 x
    the reference's absolute error at the feasible iterate, where the violation is rounding (profiles/ls_reference.md)"""
    rel = max(VIOLATION_REL, BAR) if ref >= 1e-3 else VIOLATION_REL
    return max(rel * ref, VIOLATION_FLOOR)


# Measured by test_ls_reference.py::test_violation_of_the_reference_in_50_digits (float64 reference against the same sums in 50 digits): see VIOLATION_ERRORS
#   standing iterate of type3_armijo: |v64 - v50| = 6.4e-20 at v50 = 1.589e-16;  accepted trial of backoff_two_trials' instance 1 (trot, violation 0.265): relative error 8.2e-17
VIOLATION_ERRORS = dict(feasible_abs=7e-20, backoff_rel=1e-16)
# The error at the feasible iterate is that small only because its x_next came out of the reference's own rk2: the defect cancels exactly.  The violation there IS the
# rounding of the implementation that forms it (1.6e-16), so another correct fp64 order of operations differs from it at that size: one rounding eps |x|_inf per entry
# of the 30 defects of the N = 7 nodes, dt-scaled: eps * 1.6 * sqrt(30 * 7 * 0.015).  The floor is the larger of the two.
ROUNDING_FLOOR = float(np.finfo(np.float64).eps * 1.6 * np.sqrt(30 * 7 * 0.015))
VIOLATION_REL, VIOLATION_FLOOR = 10.0 * VIOLATION_ERRORS["backoff_rel"], max(10.0 * VIOLATION_ERRORS["feasible_abs"], ROUNDING_FLOOR)


def check_outcome(case, refs, out, who, e_orc=(0.0, 0.0), fp32=False, worst=None):
    """The outcome of one call against the reference, instance by instance: alpha, step type, iteration count and convergence reason exactly; the step against
    alpha d_ref under kkt_scenarios' tolerance rule (10 x the larger of e_orc -- the oracle's step error against the same reference, measured by the CPU tier -- and
    a plain LU's); merits and the Armijo metric under the LQ bar; violations under violation_bound.  fp32: the discrete outcomes, merits and violations at 1e-4.
    worst: dict collecting the worst deviation per quantity on the scale of its bar."""
    eps = np.finfo(np.float64).eps
    worst = {} if worst is None else worst
    tol = [STEP_FACTOR * max(e_orc[j], max(r["e_lu"][j] for r in refs)) for j in (0, 1)]
    assert (out["stats"][:, 7] == 0).all(), (who, case.name)
    if fp32:     # the fp32 build forms the uniform grid t0 + k dt in fp32: equal to fp32 rounding
        assert np.abs(out["T"] - case.grid).max() <= 4 * np.finfo(np.float32).eps * np.abs(case.grid).max(), (who, case.name)
    else:
        assert np.array_equal(out["T"], case.grid), (who, case.name)

    def note(key, dev):
        assert np.isfinite(dev), (who, case.name, key)
        worst[key] = max(worst.get(key, 0.0), float(dev))

    for i, j in enumerate(case.layout):
        r, st, tag = refs[j], out["stats"][i], (who, case.name, "instance", i)
        ls = r["ls"]
        if r["reason"] == 0:                                              # the call ran on: its statistics are a later iteration's
            assert st[8] >= 2, (tag, st)
            continue
        assert (st[4], st[5], st[8], st[9]) == (ls["alpha"], ls["type"], 1, r["reason"]), (tag, st, ls["alpha"], ls["type"], r["reason"])
        if fp32:
            for key, got, ref in (("merit0", st[0], r["base"][0]), ("viol0", st[1], r["base"][1]), ("merit1", st[2], ls["merit"]), ("viol1", st[3], ls["violation"])):
                note(key, abs(got - ref) / abs(ref) / FP32_BAR)
                assert abs(got - ref) <= FP32_BAR * abs(ref), (tag, key, got, ref)
            continue
        a, d = ls["alpha"], r["d"]
        Xo, Uo, X, U = out["X"][i], out["U"][i], case.X[i], case.U[i]
        if a == 0.0:
            assert np.array_equal(Xo, X) and np.array_equal(Uo, U), tag      # no trial accepted: the iterate, bit for bit
        for jj, (got, ref, lo, hi) in enumerate(((Xo - X, a * d["dX"], X, Xo), (Uo - U, a * d["dU"], U, Uo))):
            err, scale, allow = np.abs(got - ref).max(), np.abs(ref).max(), 2 * eps * max(np.abs(lo).max(), np.abs(hi).max())
            if scale > 0:
                note(("dX", "dU")[jj], max(err - allow, 0.0) / scale / tol[jj])
            assert err <= tol[jj] * scale + allow, (tag, ("dX", "dU")[jj], err / max(scale, 1e-300), tol[jj])
        for key, got, ref in (("merit0", st[0], r["base"][0]), ("merit1", st[2], ls["merit"]), ("armijo", st[6], r["armijo"])):
            note(key, abs(got - ref) / max(1.0, abs(ref)) / BAR)
            assert abs(got - ref) <= BAR * max(1.0, abs(ref)), (tag, key, got, ref)
        if r["base"][1] < 1e-12:                                          # e = 0 to rounding (the standing iterate): the issue's form, sum q.dx + r.du, holds as well (the forms differ by O(|r| |e|)): the issue's form of the metric, sum q.dx + r.du, holds as well
            assert abs(st[6] - r["armijo_unprojected"]) <= BAR * max(1.0, abs(r["armijo_unprojected"])), (tag, st[6], r["armijo_unprojected"])
        for key, got, ref in (("viol0", st[1], r["base"][1]), ("viol1", st[3], ls["violation"])):
            note(key, abs(got - ref) / violation_bound(ref))
            assert abs(got - ref) <= violation_bound(ref), (tag, key, got, ref, violation_bound(ref))
    return worst


def check_across_calls(case, refs, out_a, out_b, who, worst=None):
    """call B's baseline (lq_node_kernel's node metrics, summed) against call A's accepted trial (the value-only node evaluation): the same iterate, two code paths"""
    worst = {} if worst is None else worst
    for i, j in enumerate(case.layout):
        a, b, ls = out_a["stats"][i], out_b["stats"][i], refs[j]["ls"]
        assert a[4] > 0.0, (who, case.name, i)
        for key, got, ref, bound in (("merit", b[0], a[2], BAR * max(1.0, abs(a[2]))), ("viol", b[1], a[3], violation_bound(a[3])),
                                     ("merit_ref", b[0], ls["merit"], BAR * max(1.0, abs(ls["merit"]))), ("viol_ref", b[1], ls["violation"], violation_bound(ls["violation"]))):
            worst["across_" + key] = max(worst.get("across_" + key, 0.0), abs(got - ref) / bound)
            assert abs(got - ref) <= bound, (who, case.name, i, key, got, ref, bound)
    return worst
