"""CPU tier: plant_reference.py on its own -- the constraint, the momentum equation, flight, a standing robot at rest, the output record -- before any kernel is compared
with it.  Bounds: C eps sum|terms| of the identity checked, C = 64 (a 62-term sum evaluated once in fp64 after a refined solve; no measured figure enters)."""
import numpy as np
import pytest

import plant_cases as PC
import plant_reference as PR
import support as S
from qm_door_amd import abi, api

EPS = PR.EPS


@pytest.fixture(scope="module")
def ctx():
    itf = api.QMInterface(lib=abi.load_library(S.build_emu()))
    return itf, S.Oracle(itf.problem)


@pytest.mark.parametrize("mode", [15, 9, 6, 13, 0])
def test_constraint_and_momentum_equation(ctx, mode):
    itf, orc = ctx
    c = PC.make_case(itf, orc, 3, mode, seed=70 + mode)
    for i in range(3):
        h = 0.002
        q, v = PR.coordinates(c["rbd"][i])
        M, nle, Jf = PR.model_terms(orc, c["rbd"][i])
        st = PR.substep(M, nle, Jf, q, v, c["tau_ff"][i], mode, h, 0.5)
        Jc = st["Jc"]
        assert Jc.shape[0] == 3 * sum(S.contact_flags(mode)) and st["sol"]["correction"] <= 1e-18
        if Jc.shape[0]:
            assert (np.abs(Jc @ st["v"]) <= 64 * EPS * (np.abs(Jc) @ np.abs(st["v"]))).all()
        res = M @ (st["v"] - v) / h + nle - np.r_[np.zeros(6), c["tau_ff"][i]] - Jc.T @ st["F"]
        terms = np.abs(M) @ (np.abs(st["v"]) + np.abs(v)) / h + np.abs(nle) + np.r_[np.zeros(6), np.abs(c["tau_ff"][i])] + np.abs(Jc).T @ np.abs(st["F"])
        assert (np.abs(res) <= 64 * EPS * terms).all(), np.abs(res / terms).max() / EPS


def test_flight_is_free_motion(ctx):
    itf, orc = ctx
    c = PC.make_case(itf, orc, 2, 0, seed=75)
    for i in range(2):
        q, v = PR.coordinates(c["rbd"][i])
        M, nle, Jf = PR.model_terms(orc, c["rbd"][i])
        r = PR.step(orc, itf.problem, c["rbd"][i], c["tau_ff"][i], 0, 0.002, bounds=False)
        free = v + 0.002 * np.linalg.solve(M, np.r_[np.zeros(6), c["tau_ff"][i]] - nle)
        assert r["F"].size == 0 and not r["contact_force"].any() and r["status"] == 0
        assert np.abs(r["v"] - free).max() <= 1e-12 * np.abs(free).max()
        assert np.array_equal(r["q"], q + 0.002 * r["v"])


def test_standing_robot_at_rest_stays_at_rest(ctx):
    itf, orc = ctx
    c = PC.make_case(itf, orc, 2, 15, seed=76, moving=False)
    for i in range(2):
        M, nle, Jf = PR.model_terms(orc, c["rbd"][i])
        first = PR.step(orc, itf.problem, c["rbd"][i], c["tau_ff"][i], 15, 0.002, bounds=False)       # the reference's own force split F0
        tau = (nle - Jf.T @ first["contact_force"] - M @ (first["v"] / 0.002))[6:]
        tau = (nle - Jf.T @ np.linalg.lstsq(Jf[:, :6].T, nle[:6], rcond=None)[0])[6:] if not np.isfinite(tau).all() else tau
        F0 = np.linalg.lstsq(Jf[:, :6].T, nle[:6], rcond=None)[0]
        r = PR.step(orc, itf.problem, c["rbd"][i], (nle - Jf.T @ F0)[6:], 15, 0.002, bounds=False)
        assert r["status"] == 0 and np.abs(r["v"]).max() <= 1e-12 and np.abs(r["rbd_next"][:24] - c["rbd"][i][:24]).max() <= 1e-14
        assert np.abs(r["F"] - F0).max() <= 1e-9 * np.abs(F0).max()
        assert abs(r["contact_force"][2::3].sum() - itf.robot_mass * itf.problem.settings.gravity) <= 1e-9 * itf.robot_mass * 9.81


def test_record_round_trip_and_status_bits(ctx):
    itf, orc = ctx
    c = PC.make_case(itf, orc, 1, 15, seed=77)
    q, v = PR.coordinates(c["rbd"][0])
    back = PR.state_record(q, v)
    assert np.abs(back[:48] - c["rbd"][0][:48]).max() <= 8 * EPS * np.abs(c["rbd"][0][:48]).max()
    assert np.abs(back[48:] - c["rbd"][0][48:]).max() <= 1e-12                     # the slots support.rbd_from_state took from the oracle's kinematics
    pull = PR.step(orc, itf.problem, c["rbd"][0], c["tau_ff"][0] + np.r_[0, 60.0, 60.0, np.zeros(15)], 15, 0.002, bounds=False)
    assert pull["status"] & (PR.PULL | PR.FRICTION) and not pull["status"] & PR.FAILED
    assert PR.contact_rows(9) == [0, 1, 2, 9, 10, 11] and PR.contact_rows(0) == []
