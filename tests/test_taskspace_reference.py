"""CPU tier: the numpy reference of the task-space trajectories (taskspace_reference.py) against itself and against what already exists -- the complex-step derivative
of the foot positions, the link poses of urdf_model.fk, the rotation the quaternion came from, the convex hull of the stance feet."""
import numpy as np
import pytest

import lq_reference as LR
import taskspace_reference as TR
import urdf_model as UM

GRAVITY = 9.81
H = 1e-30


@pytest.fixture(scope="module")
def case():
    """a 6-interval trajectory around a standing pose, 0.1 off it, momenta and joint rates of order one, normal forces all positive; a trot schedule with two landings"""
    rng = np.random.default_rng(3)
    N = 6
    x_nom = np.zeros(30)
    x_nom[8] = 0.4
    x_nom[12:24] = np.tile([0.0, 0.7, -1.4], 4)
    x_nom[24:30] = [0.0, 1.0, -1.2, 0.2, 0.0, 0.0]
    X = x_nom + 0.1 * rng.standard_normal((N + 1, 30))
    U = np.concatenate([rng.standard_normal((N, 12)) * np.tile([5.0, 5.0, 10.0], 4) + np.tile([0.0, 0.0, 60.0], 4), 0.5 * rng.standard_normal((N, 18))], axis=1)
    grid = np.array([0.0, 0.015, 0.03, 0.04, 0.055, 0.07, 0.09])
    events, modes = np.array([0.02, 0.05, 0.09]), np.array([9, 15, 6, 15])      # LF_RH -> STANCE (RF, LH land) -> RF_LH -> STANCE (at t_N: excluded)
    return grid, X, U, events, modes, TR.trajectory_taskspace(GRAVITY, grid, X, U, events, modes)


def test_foot_velocity_is_the_complex_step_of_the_foot_position(case):
    """feet_vel = d feet_pos / dt along the generalised velocity [base_twist's dp, Euler rates, joint rates] the flow map returns"""
    grid, X, U, _, _, o = case
    N = len(grid) - 1
    f, _ = LR.flow(X[:N].astype(complex), U.astype(complex), GRAVITY)
    v = f.real[:, 6:30]
    feet = LR.kinematics(X[:N, 6:30] + 1j * H * v)["feet"]
    assert np.abs(feet.imag / H - o["feet_vel"]).max() <= 1e-13 * max(1.0, np.abs(o["feet_vel"]).max())
    assert np.abs(o["base_twist"][:, :3] - v[:, :3]).max() == 0.0
    # omega: the angular velocity that turns the base rotation, R' = [omega]x R, along the same velocity
    Rb = UM.fk(X[:N, 6:30] + 1j * H * v)["base"][0]
    W = np.einsum("nij,nkj->nik", Rb.imag / H, Rb.real)
    omega = np.stack([W[:, 2, 1], W[:, 0, 2], W[:, 1, 0]], axis=1)
    assert np.abs(omega - o["base_twist"][:, 3:]).max() <= 1e-13 * max(1.0, np.abs(omega).max())
    assert (o["mag"]["feet_vel"] >= np.abs(o["feet_vel"]) * (1 - 1e-12)).all() and (o["mag"]["base_twist"] >= np.abs(o["base_twist"]) * (1 - 1e-12)).all()


def test_com_is_the_mass_weighted_mean_of_the_link_coms(case):
    grid, X, _, _, _, o = case
    pose = UM.fk(X[:, 6:30])
    com = sum(L["m"] * (pose[n][1] + pose[n][0] @ L["c"]) for n, L in UM.LINKS.items() if L["m"] != 0.0).real / sum(L["m"] for L in UM.LINKS.values())
    assert np.abs(com - o["com"]).max() <= 1e-14
    feet = np.stack([pose[f"{leg}_FOOT"][1].real for leg in UM.FEET], axis=1)
    assert np.array_equal(feet, o["feet_pos"]) and np.array_equal(pose[UM.EE_LINK][1].real, o["ee_pos"])
    for k in ("feet_pos", "ee_pos", "com"):
        assert (o["mag"][k] >= np.abs(o[k]) * (1 - 1e-12)).all(), k


def test_quaternions_are_unit_and_reproduce_the_rotation(case):
    grid, X, _, _, _, o = case
    Ree = UM.fk(X[:, 6:30])[UM.EE_LINK][0].real
    q = o["ee_quat"]
    assert np.abs(np.linalg.norm(q, axis=1) - 1.0).max() <= 4 * TR.EPS
    x, y, z, w = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)
    assert np.abs(R - Ree).max() <= 1e-14
    assert (o["mag"]["ee_quat"] >= np.abs(q) * (1 - 1e-12)).all()
    # Eigen's other branches: a half turn about each axis (trace = -1) puts the pivot on that axis
    for i in range(3):
        R = -np.eye(3)
        R[i, i] = 1.0
        qt = LR.quaternion_of(R.astype(complex)).real
        assert np.array_equal(np.abs(qt), np.eye(4)[i]) and np.isfinite(TR.quaternion_mag(R, np.abs(R), qt)).all()


def test_cop_lies_in_the_convex_hull_of_the_feet_and_vanishes_without_load(case):
    grid, X, U, events, modes, o = case
    fz = U[:, [2, 5, 8, 11]]
    assert (fz > 0).all() and (o["normal_force_sum"] > 0).all()
    w = fz / fz.sum(axis=1, keepdims=True)                                      # the barycentric weights: non-negative, summing to one
    assert np.abs(np.einsum("nc,nck->nk", w, o["feet_pos"][:-1]) - o["cop"]).max() <= 1e-14
    lo, hi = o["feet_pos"][:-1].min(axis=1), o["feet_pos"][:-1].max(axis=1)
    assert (o["cop"] >= lo - 1e-14).all() and (o["cop"] <= hi + 1e-14).all()
    assert (o["mag"]["cop"] >= np.abs(np.einsum("nc,nck->nk", np.abs(fz), np.abs(o["feet_pos"][:-1])) / o["normal_force_sum"][:, None]) * (1 - 1e-12)).all()
    # no load, or a pull: exactly zero, value and magnitude
    U0 = U.copy()
    U0[0, [2, 5, 8, 11]] = 0.0
    U0[1, [2, 5, 8, 11]] = [1.0, -3.0, 1.0, 0.5]
    z = TR.trajectory_taskspace(GRAVITY, grid, X, U0)
    assert not z["cop"][:2].any() and not z["mag"]["cop"][:2].any() and np.array_equal(z["cop"][2:], o["cop"][2:])


def test_footholds_follow_the_schedule_and_the_interpolated_state(case):
    grid, X, U, events, modes, o = case
    flag = o["foothold_flag"]
    assert flag.shape == (TR.MAX_EVENTS, 4) and flag[0].tolist() == [0, 1, 1, 0] and flag[1].tolist() == [0, 0, 0, 0] and not flag[2:].any()   # the event at t_N is excluded
    i, al = LR.time_segment(grid, events[0])
    assert i == 1 and 0.0 < al < 1.0
    x = al * X[1] + (1 - al) * X[2]
    feet = LR.kinematics(x[None, 6:30])["feet"][0].real
    assert np.array_equal(o["foothold_pos"][0][[1, 2]], feet[[1, 2]]) and not o["foothold_pos"][0][[0, 3]].any() and not o["foothold_pos"][1:].any()
    assert not o["mag"]["foothold_pos"][flag == 0].any() and (o["mag"]["foothold_pos"][flag == 1] >= np.abs(o["foothold_pos"][flag == 1])).all()
    # an event ON a node: the weight sits at its edge and the foothold is that node's foot position, bit for bit
    on_node = TR.trajectory_taskspace(GRAVITY, grid, X, None, np.array([grid[3]]), np.array([9, 15]))
    assert np.array_equal(on_node["foothold_pos"][0][[1, 2]], o["feet_pos"][3][[1, 2]])
    assert "feet_vel" not in on_node and "cop" not in on_node
