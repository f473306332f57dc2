// metrics_lds.h -- the dynamic LDS of one metrics_kernel workgroup (one MPC instance, METRICS_THREADS nodes per pass): every region once, in address order.  The unit
// is `real`.  metrics_kernel.h takes every offset and every row stride from here.  No overlays: every region keeps its meaning for the whole kernel.
#pragma once
#include "layout.h"
#include "lds_region.h"
#include "problem_r.h"
#include "real.h"

namespace qmk {

constexpr int METRICS_THREADS = 128;   // one node per lane and pass; a horizon of N + 1 <= 128 nodes is one pass

// Row strides (reals).  A lane reads and writes ITS node's row, so consecutive lanes are one stride apart: 30, 16 and 8 reals would put them 4, 32 and 16 deep on the
// same banks (64 banks of 4 bytes); odd strides spread the 64-bit accesses of a wavefront over all of them.
constexpr int ML_XROW = 31, ML_EROW = 17, ML_TROW = 9;
constexpr int METRICS_TERMS = 8;       // QMGPU_NCOST_TERMS

using MetricsRegion = LdsRegion<real, real>;
constexpr MetricsRegion ML_Q{0, NX * NX};                                              // Q  [30][30] of the tracking cost: every lane reads all of it per node
constexpr auto ML_R = ldsAfter<real>(ML_Q, NU * NU);                                   // R' [30][30]
constexpr auto ML_MODEL = ldsAfter<int>(ML_R, int(sizeof(ModelR) / sizeof(int)));      // the model constants: the sweeps read them with wave-uniform indices
constexpr auto ML_X = ldsAfter<real>(ML_MODEL, (METRICS_THREADS + 1) * ML_XROW);       // states of the pass's nodes and of the node behind the last one (x_next of that lane)
constexpr auto ML_U = ldsAfter<real>(ML_X, METRICS_THREADS * ML_XROW);                 // inputs of the pass's nodes; zeros for the terminal node
constexpr auto ML_D = ldsAfter<real>(ML_U, METRICS_THREADS * ML_XROW);                 // out: defect rows, stored to HBM as one run behind the barrier
constexpr auto ML_E = ldsAfter<real>(ML_D, METRICS_THREADS * ML_EROW);                 // out: equality rows, rows >= nc zero
constexpr auto ML_T = ldsAfter<real>(ML_E, METRICS_THREADS * ML_TROW);                 // out: cost terms
constexpr int METRICS_RED_ROWS = 4;
constexpr auto ML_RED = ldsAfter<real>(ML_T, METRICS_RED_ROWS * METRICS_THREADS);      // per-thread partial sums: cost | dt |defect|^2 | dt |eq|^2 | (x0 - X_0)_t^2 (row r of thread t: [r * THREADS + t]), reduced by a pairwise tree
constexpr int METRICS_LDS_REALS = ML_RED.end();
constexpr int METRICS_LDS_BYTES = METRICS_LDS_REALS * int(sizeof(real));
static_assert(sizeof(ModelR) % sizeof(int) == 0 && alignof(ModelR) <= sizeof(real), "the model is copied word by word to a real-aligned offset");
static_assert((METRICS_THREADS & (METRICS_THREADS - 1)) == 0 && NX <= METRICS_THREADS, "the tree halves a power of two; one lane per entry of x0");
static_assert(METRICS_LDS_BYTES <= QM_CU_LDS_BYTES, "one instance per compute unit");
static_assert(NX <= ML_XROW && NU <= ML_XROW && NCMAX <= ML_EROW && METRICS_TERMS <= ML_TROW, "a row holds its vector");

}  // namespace qmk
