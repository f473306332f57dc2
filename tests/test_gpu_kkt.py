"""-m gpu: the product's SQP step against an independent high-precision solve of the QP it says it formed (kkt_reference.py), over every node of every instance.

For each scenario of kkt_scenarios.gpu_scenarios() (all four factorisation unrolls of lq_node_kernel and a batch mixing them, defect-laden warm starts and the
cold initializer, an event-aligned grid with a step of dt / 6, the relaxed barriers in their quadratic branches with three target knots, force tracking,
N = 1, 2, 200, 300, line search off and on, and a 300-instance batch that takes the 128-thread line-search launch): one SQP iteration with the LQ dump on;
nc and the blocks of every node against the oracle (1e-10); the reference solved from the product's OWN blocks; X_out - X and U_out - U against alpha times
its step under the tolerance rule of kkt_scenarios.py (10 x the larger of the oracle's and a plain fp64 LU's error against the reference, measured here);
and the same solve with the dump off bit-identical.  Every scenario prints its measured figures; with KKT_STEP_RECORD set to a file path they are also
collected there as JSON (the record of profiles/r08_kkt_step.json)."""
import os

import numpy as np
import pytest

import kkt_scenarios as KS
import support as S

pytestmark = pytest.mark.gpu

RECORD = os.environ.get("KKT_STEP_RECORD") or None


@pytest.fixture(scope="module")
def force_tracking_setup():
    itf = KS.force_tracking_interface()
    return itf, S.Oracle(itf.problem)


def _solve(G, sol, sc):
    import torch
    mb = G.MpcBatch(sc.x0, sc.tt, sc.ts, sc.nev, sc.ev, sc.md, sc.N, warm=(sc.X, sc.U) if sc.warm else None, line_search=sc.line_search,
                    time_grid=None if sc.uniform else sc.grid)
    if sc.contact is not None:
        mb.contact = G.dev(sc.contact, torch.float64)                  # kept alive with the batch
        mb.args.ee_contact_ref = mb.contact.data_ptr()
    sol.mpc(mb.args)
    return mb.results()


@pytest.mark.parametrize("name", list(KS.gpu_scenarios()))
def test_product_step_equals_kkt_reference(interface, oracle, force_tracking_setup, name):
    import gpu_harness as G
    itf, orc = force_tracking_setup if name == "force_tracking" else (interface, oracle)
    sc = KS.build(KS.gpu_scenarios(), name, itf, orc)
    sol = G.make_solver(itf, sc.B, sc.N)
    off = _solve(G, sol, sc)
    sol.enable_debug(True)
    on = _solve(G, sol, sc)
    KS.check_product(sc, orc, on, sol.debug_lq, record_path=RECORD)
    for key in ("T", "X", "U", "mode", "stats"):
        assert np.array_equal(on[key], off[key]), (name, key)          # the checked path is the product path
    sol.close()
