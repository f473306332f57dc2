// The SQP feedback policy (task.info sqp.useFeedbackPolicy): what upstream's SqpSolver returns as a LinearController instead of a feed-forward one
// (multiple_shooting::remapProjectedGain, then toPrimalSolution with gains) and what MRT_BASE::evaluatePolicy -> LinearController::computeInput makes of it.
//
//   feedback_gain_kernel      K_k   = Px_k + Pu_k K~_k          k = 0 .. N-1   (30 x 30, row-major)
//                             uff_k = u_k - K_k x_k             (x, u: the iterate the solve returned)
//                             K_N   = K_{N-1}, uff_N = uff_{N-1}                (upstream: "copy last one to get correct length")
//   policy_feedback_kernel    u(t) = uff(t) + K(t) x_measured, uff and K interpolated with the index and alpha of policy_eval_kernel
//
// Everything the gains need is in HBM after a solve: the projected Riccati gains K~ [MT][30] (layout.h: OFF_KFB) and Px, Pu in the head of every stage
// record (rows 12..29; rows 0..11 of Px are zero and rows 0..11 of Pu unit vectors on the free stance forces, neither stored).  Rows and columns beyond
// m~ = 30 - nc are zero in the record and in the gains image, so all MT = 18 are multiplied without masks.  With sqp.sqpIteration > 1 the kernels of the
// later iterations return at once for an instance that has converged: its records and gains are those of the last iteration it performed, the iteration
// its out_x / out_u come from -- no special case here.
//
// The gain kernel streams (19.2 KB per node, 20 k multiply-adds): one wavefront per (instance, node).  The 18 x 18 x 30 product runs on the matrix cores
// as 2 x 2 tiles of 16 x 16 with five steps of four (rows 28, 29, columns 30, 31 and steps 18, 19 are zero operands); the tile of K is assembled in LDS so
// that it leaves as one contiguous run of 900 doubles and so that lane i can form row i of K x.
#pragma once
#include "gpu_rt.h"
#include "layout.h"
#include "schedule_dev.h"

namespace qmk {

struct FeedbackArgs {
  int batch, N;
  const real* stages;      // [batch][N+1][STAGE_DOUBLES]
  const real* gains;       // [batch][N][GAIN_DOUBLES]
  const real* instStats;   // [batch][4]: [1] = status of the backward sweep (out_stats[7])
  const double* X;         // [batch][N+1][30]
  const double* U;         // [batch][N][30]
  double* K;               // [batch][N+1][30][30]
  double* uff;             // [batch][N+1][30]
  int* status;             // [batch] or null
};

constexpr int FB_LD = 31;   // row stride of the K tile in LDS: odd, so that the lanes that walk one row each stay on different banks

__global__ void __launch_bounds__(64) feedback_gain_kernel(FeedbackArgs a) {
  __shared__ real Kl[30 * FB_LD];
  const int lane = threadIdx.x, N = a.N;
  const int inst = blockIdx.x / (N + 1), node = blockIdx.x - inst * (N + 1);
  if (inst >= a.batch) return;
  const int k = node < N ? node : N - 1;   // node N repeats node N - 1: the same arithmetic on the same data, bit for bit
  const double* x = a.X + (size_t(inst) * (N + 1) + k) * 30;
  const double* u = a.U + (size_t(inst) * N + k) * 30;
  double* Ko = a.K + (size_t(inst) * (N + 1) + node) * 900;
  double* uo = a.uff + (size_t(inst) * (N + 1) + node) * 30;
  // a failed factorisation (wavefront-uniform) leaves gains that may hold inf / NaN: the instance gets the feed-forward policy K = 0, uff = u
  const bool failed = !(a.instStats[size_t(inst) * 4 + 1] == 0.0_r);
  if (a.status && node == 0 && lane == 0) a.status[inst] = failed ? 1 : 0;
  if (failed) {
    for (int e = lane; e < 900; e += 64) QM_STREAM_STORE(Ko + e, 0.0);
    if (lane < 30) uo[lane] = u[lane];
    return;
  }
  const real* rec = a.stages + (size_t(inst) * (N + 1) + k) * STAGE_DOUBLES;
  const real* gn = a.gains + (size_t(inst) * N + k) * GAIN_DOUBLES;
  const int l16 = lane & 15, lq = lane >> 4;
  // ---- every load in front of the first use: the operands of the 20 matrix-core steps, Px into the accumulators, the force rows, x and u
  real av[2][5], bv[2][5];
  QmAcc acc[2][2];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int i = 12 + 16 * rt + qmARow(l16);   // row of Pu this lane supplies
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      const int r = 4 * s + lq;
      const bool ok = i < 30 && r < MT;
      const real v = rec[ok ? offPuRow(i) + r : offPuRow(12)];
      av[rt][s] = ok ? v : 0.0_r;
    }
  }
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int c = 16 * ct + l16;
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      const int r = 4 * s + lq;
      const bool ok = c < 30 && r < MT;
      const real v = gn[ok ? OFF_KFB + r * 30 + c : OFF_KFB];
      bv[ct][s] = ok ? v : 0.0_r;
    }
  }
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = 12 + 16 * rt + lq + 4 * q, c = 16 * ct + l16;
        const bool ok = i < 30 && c < 30;
        const real v = rec[ok ? offPxRow(i) + c : offPxRow(12)];
        acc[rt][ct][q] = ok ? v : 0.0_r;
      }
  // rows 0..11: row puColumnOfForce(mode, i) of K~, or zero for a swing foot
  const int mode = int(rec[OFF_MODE]);
  real force[6];
#pragma unroll
  for (int p = 0; p < 6; ++p) {
    const int e = min(lane + 64 * p, 359), i = e / 30, c = e - 30 * i;
    const int pc = puColumnOfForce(mode, i);
    const real v = gn[OFF_KFB + max(pc, 0) * 30 + c];
    force[p] = pc >= 0 ? v : 0.0_r;
  }
  const int li = lane < 30 ? lane : 0;
  real xv[30];
#pragma unroll
  for (int c = 0; c < 30; ++c) xv[c] = real(x[c]);   // wavefront-uniform addresses
  const real ui = real(u[li]);
  // ---- K rows 12..29 = Px + Pu K~
#pragma unroll
  for (int s = 0; s < 5; ++s)
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) qmMfma(acc[rt][ct], av[rt][s], bv[ct][s]);
  // ---- the tile of K in LDS
#pragma unroll
  for (int p = 0; p < 6; ++p) {
    const int e = lane + 64 * p, i = e / 30, c = e - 30 * i;
    if (e < 360) Kl[i * FB_LD + c] = force[p];
  }
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = 12 + 16 * rt + lq + 4 * q, c = 16 * ct + l16;
        if (i < 30 && c < 30) Kl[i * FB_LD + c] = acc[rt][ct][q];
      }
  QM_WAVE_SYNC();
  // ---- out: K as one contiguous run, uff_i = u_i - K_i . x by lane i
#pragma unroll
  for (int p = 0; p < 15; ++p) {
    const int e = lane + 64 * p, i = e / 30, c = e - 30 * i;
    if (e < 900) QM_STREAM_STORE(Ko + e, double(Kl[i * FB_LD + c]));
  }
  real s = ui;
#pragma unroll
  for (int c = 0; c < 30; ++c) s = fma(-Kl[li * FB_LD + c], xv[c], s);
  if (lane < 30) uo[lane] = double(s);
}

// LinearController::computeInput behind MRT_BASE::evaluatePolicy (call site QMController.cpp:134-142): u = uff(t) + K(t) x_measured, uff and K interpolated
// linearly with the index and alpha policy_eval_kernel uses for U (end values held; K and uff have N + 1 entries, the last a copy, so no clamp is needed).
// x_out and mode_out are policy_eval_kernel's, expression for expression.  One wavefront per instance: lanes 0..29 interpolate the state and then form row
// `lane` of the input, lane 63 the mode.  The interpolated gains are rounded as products and a sum of their own (no fused multiply-add), i.e. as the plain
// statement of the formula rounds them: where the two ends of an interval cancel, a fused form would differ from it by more than the size of the result.
__global__ void __launch_bounds__(64) policy_feedback_kernel(int batch, int N, const real* tgrid, const real* X, const real* uff, const real* K, const int* modes,
                                                             const real* tEval, const real* xMeasured, real* xOut, real* uOut, int* modeOut) {
  const int inst = blockIdx.x, lane = threadIdx.x;
  if (inst >= batch) return;
  const real* tg = tgrid + size_t(inst) * (N + 1);
  const real t = tEval[inst];
  int idx; real alpha;
  timeSegmentWave(tg, N + 1, t, lane, idx, alpha);
  const int kMode = gridCountBelow(tg + 1, N, t, lane);
  if (lane < 30) {
    const real* xl = X + (size_t(inst) * (N + 1) + idx) * 30;
    xOut[size_t(inst) * 30 + lane] = alpha * xl[lane] + (1.0_r - alpha) * xl[30 + lane];
    const real beta = 1.0_r - alpha;
    const real* fl = uff + (size_t(inst) * (N + 1) + idx) * 30;
    const real* Kl = K + ((size_t(inst) * (N + 1) + idx) * 30 + lane) * 30;   // row `lane` of K_idx; K_{idx + 1} follows 900 entries later
    const real* xm = xMeasured + size_t(inst) * 30;
    real s = qmMulNoFma(alpha, fl[lane]) + qmMulNoFma(beta, fl[30 + lane]);
#pragma unroll
    for (int c = 0; c < 30; ++c) {
      const real kt = qmMulNoFma(alpha, Kl[c]) + qmMulNoFma(beta, Kl[900 + c]);
      s = fma(kt, xm[c], s);
    }
    uOut[size_t(inst) * 30 + lane] = s;
  } else if (lane == 63) {
    modeOut[inst] = modes[size_t(inst) * (N + 1) + kMode];
  }
}

}  // namespace qmk
