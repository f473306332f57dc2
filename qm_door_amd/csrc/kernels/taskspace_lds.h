// taskspace_lds.h -- the dynamic LDS of one taskspace_kernel workgroup (one MPC instance, TASKSPACE_THREADS nodes per pass): every region once, in address order.  The
// unit is `real`.  taskspace_kernel.h takes every offset and every row stride from here.  No overlays: every region keeps its meaning for the whole kernel; the foothold
// phase reuses the ROWS of TL_X / TL_U (row e: the state interpolated at event e, and zeros) behind a barrier, not other regions.
#pragma once
#include "layout.h"
#include "lds_region.h"
#include "problem_r.h"
#include "real.h"

namespace qmk {

constexpr int TASKSPACE_THREADS = 128;   // one node per lane and pass; a horizon of N + 1 <= 128 nodes is one pass.  Two wavefronts: they share the events of the foothold phase

// Row strides (reals).  A lane reads and writes ITS node's row, so consecutive lanes are one stride apart: 30, 12, 4 and 6 reals would put them 4, 8, 8 and 16 deep on
// the same banks (64 banks of 4 bytes, 32 lanes per group of a 64-bit access); odd strides spread a group over all of them.
constexpr int TL_XROW = 31, TL_FROW = 13, TL_VROW = 3, TL_QROW = 5, TL_TWROW = 7;
constexpr int TASKSPACE_FEET_W = 12, TASKSPACE_VEC_W = 3, TASKSPACE_QUAT_W = 4, TASKSPACE_TWIST_W = 6;   // widths of the output rows: [4][3], [3], x y z w, [dp ; omega]

constexpr LdsRegion<int, real> TL_MODEL{0, int(sizeof(ModelR) / sizeof(int))};           // the model constants: the sweeps read them with wave-uniform indices
constexpr auto TL_X = ldsAfter<real>(TL_MODEL, TASKSPACE_THREADS * TL_XROW);            // states of the pass's nodes; foothold phase: row e = the state at event e
constexpr auto TL_U = ldsAfter<real>(TL_X, TASKSPACE_THREADS * TL_XROW);                // inputs of the pass's nodes, zeros for the terminal node and without U; foothold phase: zeros
constexpr auto TL_FP = ldsAfter<real>(TL_U, TASKSPACE_THREADS * TL_FROW);               // out: feet_pos rows, stored to HBM as one run behind the barrier
constexpr auto TL_EE = ldsAfter<real>(TL_FP, TASKSPACE_THREADS * TL_VROW);              // out: ee_pos
constexpr auto TL_Q = ldsAfter<real>(TL_EE, TASKSPACE_THREADS * TL_QROW);               // out: ee_quat
constexpr auto TL_COM = ldsAfter<real>(TL_Q, TASKSPACE_THREADS * TL_VROW);              // out: com
constexpr auto TL_FV = ldsAfter<real>(TL_COM, TASKSPACE_THREADS * TL_FROW);             // out: feet_vel (intermediate nodes)
constexpr auto TL_TW = ldsAfter<real>(TL_FV, TASKSPACE_THREADS * TL_TWROW);             // out: base_twist
constexpr auto TL_COP = ldsAfter<real>(TL_TW, TASKSPACE_THREADS * TL_VROW);             // out: cop
constexpr auto TL_FH = ldsAfter<real>(TL_COP, QMGPU_MAX_EVENTS * TL_FROW);              // out: foothold_pos rows, one per event, entries of feet that do not land zero
constexpr int TASKSPACE_LDS_REALS = TL_FH.end();
constexpr int TASKSPACE_LDS_BYTES = TASKSPACE_LDS_REALS * int(sizeof(real));
static_assert(sizeof(ModelR) % sizeof(int) == 0 && alignof(ModelR) <= sizeof(real), "the model is copied word by word to a real-aligned offset");
static_assert(TASKSPACE_THREADS % 64 == 0 && QMGPU_MAX_EVENTS <= TASKSPACE_THREADS, "whole wavefronts; one lane and one row of TL_X / TL_U per event");
static_assert(2 * NX <= 64, "lanes 0..29 of a wavefront interpolate an event's state, lanes 30..59 clear its input row");
static_assert(TASKSPACE_LDS_BYTES <= QM_CU_LDS_BYTES, "one instance per compute unit");
static_assert(NX <= TL_XROW && NU <= TL_XROW && TASKSPACE_FEET_W <= TL_FROW && TASKSPACE_VEC_W <= TL_VROW && TASKSPACE_QUAT_W <= TL_QROW && TASKSPACE_TWIST_W <= TL_TWROW, "a row holds its vector");

}  // namespace qmk
