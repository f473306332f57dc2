"""A numpy-only reference for the planned task-space trajectories (qmgpu_mpc_taskspace_batch): per node the four foot positions, the end-effector position and
quaternion and the centre of mass; per intermediate node the foot velocities, the base twist and the centre of pressure; per event of the mode schedule the flags and
positions of the feet that land there.

Rule of lq_reference.py: nothing of support.Oracle, nothing under oracle/, no kernel-derived helper; the robot comes from lq_reference's own URDF parse.  Built from
lq_reference's kinematics and flow (feet, foot Jacobians, CoM, EE pose, foot velocities, the base velocity the momentum implies), quaternion_of, contact_flags and
time_segment; the gravity passed to flow does not enter any value returned here.

Conventions (include/qmgpu.h): world axes; foot index c in contact order (LF, RF, LH, RH); quaternion x y z w.  cop = (sum_c fz_c p_c) / s with
s = ((fz_0 + fz_1) + fz_2) + fz_3 added in this order if s > 0, three zeros otherwise.  Foot c lands at event e if time_grid[0] < t_e < time_grid[N] (both strict),
the foot is off the ground in modes[e] and on it in modes[e + 1]; its foothold is its position at the state interpolated linearly from X at t_e.

Magnitudes.  Next to every value the reference returns the sum of the magnitudes of the terms the value was formed from, one level down (metrics_reference.py states
the rule): a position p_base + R_base c is given |p_base| + |R_base| |c|; a velocity J v is given |J| |v| with |v| the magnitude of the generalised velocity; the
quaternion entries the magnitudes of the entries of R_ee = R_base R_arm they combine, each entry the three products it is; cop = n / s is given sum_c |fz_c| mag(p_c) / |s| + |cop| sum_c |fz_c| / |s|, which includes
sum_c |fz_c p_c| / |s|; a foothold the magnitude of the interpolated state carried through the foot Jacobian.  They are the scale of the tolerance rule
    |kernel - reference| <= C * eps * magnitude
with one C per output class, set in test_emu_taskspace.py from ratios measured on the host build (profiles/taskspace_parity.json)."""
import numpy as np

import lq_reference as LR
import urdf_model as UM

EPS = np.finfo(np.float64).eps
MAX_EVENTS = 40
CLASSES = ("feet_pos", "ee_pos", "ee_quat", "com", "feet_vel", "base_twist", "cop", "foothold_pos")
NODE_OUTPUTS = ("feet_pos", "ee_pos", "ee_quat", "com")
STEP_OUTPUTS = ("feet_vel", "base_twist", "cop")


def _positions(X):
    """feet [n, 4, 3], ee [n, 3], Ree [n, 3, 3], com [n, 3] of the states X [n, 30], their magnitudes, and the foot Jacobians [n, 4, 24, 3]"""
    q = np.asarray(X, float)[:, 6:30]
    kin = LR.kinematics(q)
    R0 = UM.fk(q)["base"][0].real                                              # [n, 3, 3]
    p = q[:, 0:3]

    def mag(world):                                                            # world [n, ..., 3] -> |p| + |R0| |R0^T (world - p)|
        rel = world - p.reshape((len(p),) + (1,) * (world.ndim - 2) + (3,))
        local = np.einsum("nji,n...j->n...i", R0, rel)
        return np.abs(p).reshape((len(p),) + (1,) * (world.ndim - 2) + (3,)) + np.einsum("nij,n...j->n...i", np.abs(R0), np.abs(local))
    feet, ee, com, Ree = kin["feet"].real, kin["ee"].real, kin["com"].real, kin["Ree"].real
    # R_ee = R_base R_arm: an entry is three products, given their magnitudes
    Ree_mag = np.einsum("nij,njk->nik", np.abs(R0), np.abs(np.einsum("nji,njk->nik", R0, Ree)))
    return dict(feet=feet, ee=ee, com=com, Ree=Ree, Ree_mag=Ree_mag, J=kin["Jfeet"].real, feet_mag=mag(feet), ee_mag=mag(ee), com_mag=mag(com))


def quaternion_mag(R, Rm, qt):
    """magnitude of each entry of quaternion_of(R) (one rotation), Rm the magnitudes of R's entries: the pivot entry 1/2 sqrt(z), z = 1 +- R00 +- R11 +- R22, carries
    itself (the root's own rounding) and |d/dz| (1 + Rm00 + Rm11 + Rm22); every other entry (a +- b) / (2 sqrt(z)) carries (mag a + mag b) / (2 sqrt(z)) and its own share of z"""
    zmag = 1.0 + Rm[0, 0] + Rm[1, 1] + Rm[2, 2]
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        piv, z = 3, R[0, 0] + R[1, 1] + R[2, 2] + 1.0
        pairs = {0: ((2, 1), (1, 2)), 1: ((0, 2), (2, 0)), 2: ((1, 0), (0, 1))}
    else:
        i = 1 if R[1, 1] > R[0, 0] else 0
        i = 2 if R[2, 2] > R[i, i] else i
        j, k = (i + 1) % 3, (i + 2) % 3
        piv, z = i, R[i, i] - R[j, j] - R[k, k] + 1.0
        pairs = {3: ((k, j), (j, k)), j: ((j, i), (i, j)), k: ((k, i), (i, k))}
    s = np.sqrt(z)
    m = np.zeros(4)
    m[piv] = abs(qt[piv]) + 0.25 / s * zmag
    for e, (a, b) in pairs.items():
        m[e] = (Rm[a] + Rm[b]) * 0.5 / s + abs(qt[e]) * 0.5 / z * zmag
    return m


def landing_flags(grid, events, modes):
    """[MAX_EVENTS, 4] int32 from the schedule alone: 1 where foot c lands at event e strictly inside (grid[0], grid[-1])"""
    flag = np.zeros((MAX_EVENTS, 4), dtype=np.int32)
    for e, t in enumerate(events):
        if grid[0] < t < grid[-1]:
            before, after = LR.contact_flags(modes[e]), LR.contact_flags(modes[e + 1])
            flag[e] = [int((not before[c]) and after[c]) for c in range(4)]
    return flag


def trajectory_taskspace(gravity, grid, X, U=None, events=None, modes=None):
    """Every output of the call for one instance (U None: positions only; events None: no footholds), and under "mag" the magnitude of every entry.
    events [nev], modes [nev + 1]: the mode schedule."""
    grid, X = np.asarray(grid, float), np.asarray(X, float)
    N = len(grid) - 1
    pos = _positions(X)
    quat = np.array([LR.quaternion_of(pos["Ree"][k].astype(complex)).real for k in range(N + 1)])
    o = dict(feet_pos=pos["feet"], ee_pos=pos["ee"], ee_quat=quat, com=pos["com"])
    m = dict(feet_pos=pos["feet_mag"], ee_pos=pos["ee_mag"], com=pos["com_mag"], ee_quat=np.array([quaternion_mag(pos["Ree"][k], pos["Ree_mag"][k], quat[k]) for k in range(N + 1)]))
    if U is not None:
        U = np.asarray(U, float)
        f, kin = LR.flow(X[:N].astype(complex), U.astype(complex), gravity)
        A, J = kin["A"].real, kin["Jfeet"].real                                # [N, 6, 24], [N, 4, 24, 3]
        v = f.real[:, 6:30]                                                    # generalised velocity [dp, Euler ZYX rates, joint rates]
        vj = np.abs(U[:, 12:30])
        vb = np.einsum("nij,nj->ni", np.abs(np.linalg.inv(A[:, :, :6])), LR.MASS * np.abs(X[:N, :6]) + np.einsum("nij,nj->ni", np.abs(A[:, :, 6:]), vj))
        vmag = np.concatenate([vb, vj], axis=1)
        o["feet_vel"] = kin["footvel"].real
        m["feet_vel"] = np.einsum("nd,ncdk->nck", vmag, np.abs(J))
        # world angular velocity of the base: the Euler rates about z, the rotated y and the twice-rotated x (lq_reference.twists)
        Rz, Ry = UM.rot((0, 0, 1), X[:N, 9]).real, UM.rot((0, 1, 0), X[:N, 10]).real
        axes = np.stack([np.broadcast_to(np.array([0.0, 0.0, 1.0]), (N, 3)), Rz @ np.array([0.0, 1.0, 0.0]), (Rz @ Ry) @ np.array([1.0, 0.0, 0.0])], axis=1)   # [N, 3 rates, 3]
        o["base_twist"] = np.concatenate([v[:, 0:3], np.einsum("nr,nrk->nk", v[:, 3:6], axes)], axis=1)
        m["base_twist"] = np.concatenate([vmag[:, 0:3], np.einsum("nr,nrk->nk", vmag[:, 3:6], np.abs(axes))], axis=1)
        fz = U[:, [2, 5, 8, 11]]
        s = ((fz[:, 0] + fz[:, 1]) + fz[:, 2]) + fz[:, 3]
        cop, cmag = np.zeros((N, 3)), np.zeros((N, 3))
        on = s > 0
        feet, fmag = pos["feet"][:N], pos["feet_mag"][:N]
        cop[on] = np.einsum("nc,nck->nk", fz[on], feet[on]) / s[on, None]
        cmag[on] = (np.einsum("nc,nck->nk", np.abs(fz[on]), fmag[on]) + np.abs(cop[on]) * np.abs(fz[on]).sum(axis=1, keepdims=True)) / np.abs(s[on, None])
        o["cop"], m["cop"], o["normal_force_sum"] = cop, cmag, s
    if events is not None:
        events = np.asarray(events, float)
        flag = landing_flags(grid, events, modes)
        fh, fm = np.zeros((MAX_EVENTS, 4, 3)), np.zeros((MAX_EVENTS, 4, 3))
        for e in np.flatnonzero(flag.any(axis=1)):
            i, al = LR.time_segment(grid, events[e])
            x = al * X[i] + (1 - al) * X[i + 1]
            xm = al * np.abs(X[i]) + (1 - al) * np.abs(X[i + 1])
            p = _positions(x[None, :])
            full = p["feet"][0]
            # |p| of the interpolated base position, |R0| |c|, and the interpolated angles (base Euler angles, joints) carried through the foot Jacobian
            fullm = xm[6:9] + (p["feet_mag"][0] - np.abs(x[6:9])) + np.einsum("cdk,d->ck", np.abs(p["J"][0][:, 3:]), xm[9:30])
            fh[e], fm[e] = np.where(flag[e, :, None] == 1, full, 0.0), np.where(flag[e, :, None] == 1, fullm, 0.0)
        o["foothold_pos"], o["foothold_flag"], m["foothold_pos"] = fh, flag, fm
    o["mag"] = m
    return o


def ratios(got, ref):
    """worst |got - ref| / (eps * magnitude) per output class present in both (got: the call's arrays of one instance; ref: trajectory_taskspace).  An entry without
    terms (magnitude 0: cop with s <= 0, a foothold entry without a landing) must be exact."""
    out = {}
    for cls in CLASSES:
        if cls not in got or cls not in ref:
            continue
        d, s = np.abs(got[cls] - ref[cls]), ref["mag"][cls]
        assert (d[s == 0] == 0).all(), (cls, "a value without terms must be exact")
        out[cls] = float((d[s > 0] / (EPS * s[s > 0])).max()) if (s > 0).any() else 0.0
    return out
