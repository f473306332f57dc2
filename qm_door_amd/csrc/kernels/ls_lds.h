// ls_lds.h -- the LDS of one linesearch_kernel workgroup (one MPC instance).  The fixed part is six separate __shared__ arrays whose types are declared here; its size
// is the sum of their sizeofs, each padded to 16 bytes, and the kernel asserts the same sum beside its declarations.  Behind it lies the dynamic part, the trial
// trajectories of the launches whose horizon fits.  linesearch_kernel.h takes the rows of `red`, the control words and the place of a trial slice from here, the host
// (mpc_pipeline.h) the budget.
// Why six objects and not one: as one struct, and as the head of a single dynamic carve, the registers and spills of the kernel AND of the called nodePerformance
// moved (profiles/ad_ls_lds.md), and nodePerformance is the function whose compilation DESIGN.md 4.4 is careful about.
#pragma once
#include <cstddef>

#include "layout.h"
#include "problem_r.h"
#include "real.h"

namespace qmk {

constexpr int LS_MAX_THREADS = 256;   // launch bound of the kernel, row length of `red`, the larger of the two launch shapes (lsThreads)

// control words: thread 0 writes them between two barriers, every thread reads them behind the second
enum LsCtl {
  LS_MERIT0, LS_VIOL0,        // merit and constraint violation of the incoming iterate (sums of lq_node_kernel's node metrics)
  LS_MERIT1, LS_VIOL1,        // of the last trial judged in this pass
  LS_ACCEPTED, LS_STEP_TYPE,  // that trial was accepted (0 / 1); the branch of FilterLinesearch::acceptStep that judged it
  LS_ALPHA,                   // its step length
  LS_STRUCTURED,              // the tracking weights have the structured pattern (nodePerformance: weightStructure)
  LS_CTL_WORDS
};

// ---- the fixed part: the types of the kernel's six __shared__ arrays, in the order it declares them
using LsRed = real[3][LS_MAX_THREADS];   // per-thread partial sums: cost | defect | equality of a trial (row r of thread t: red[r][t])
using LsCtlWords = real[LS_CTL_WORDS];
using LsVotes = int[LS_MAX_THREADS];     // per thread: one of my weight entries lies outside the structured pattern
//    ModelR mdS                         // the model constants: the sweeps read them with wave-uniform indices, from LDS instead of through the scalar cache
using LsWeights = real[NX * NX];         // wQ, wR (NU = NX): state / input weights of the tracking cost, every lane reads all 1800 of them per node (ds_read_b128: 16-byte aligned)
static_assert(NU == NX, "wQ and wR share a type");
// What the launch has to leave free of the CU's LDS.  The compiler places the six objects in an order of its own, none aligned to more than 16 bytes: every sizeof
// rounded up to 16 bounds the total whatever the order.  This list and the kernel's assertion are both kept by hand: a new __shared__ array has to be added to both,
// and the figure to check them against is .group_segment_fixed_size of linesearch_kernel in the device assembly (build.device_asm).  The bound is tight: .group_segment_fixed_size of
// linesearch_kernel is 24,496 B in the fp64 code object and 12,848 B in the fp32 one (8 B of padding in front of the weights; the plain sum of sizeofs is 12,840).
// (Until this header the figure was a sum of element counts kept by hand, with 256 B on top for such padding.)
constexpr int lsLdsBytes(size_t size) { return int((size + 15) / 16 * 16); }
constexpr int LS_STATIC_LDS_BYTES = lsLdsBytes(sizeof(LsRed)) + lsLdsBytes(sizeof(LsCtlWords)) + lsLdsBytes(sizeof(LsVotes)) + lsLdsBytes(sizeof(ModelR)) + 2 * lsLdsBytes(sizeof(LsWeights));
static_assert(LS_STATIC_LDS_BYTES == (sizeof(real) == 8 ? 24496 : 12848), "the fixed part as the code objects record it");

// ---- the dynamic part: one slice per trial evaluated side by side, X [N+1][30] then U [N][30]
__host__ __device__ constexpr int lsTrialRows(int N) { return 2 * N + 1; }   // rows of NX = NU reals in one slice: N + 1 of X, then N of U
// dynamic LDS of a line-search launch that keeps the trial trajectories on chip: 0 if they do not fit beside the fixed part
inline int lsTrialLdsBytes(int N, int threads) {
  const int trials = (N + 1 <= threads / 2) ? 2 : 1;
  const long long need = (long long)trials * lsTrialRows(N) * NX * (long long)sizeof(real);
  return need + LS_STATIC_LDS_BYTES <= QM_CU_LDS_BYTES ? int(need) : 0;
}

}  // namespace qmk
