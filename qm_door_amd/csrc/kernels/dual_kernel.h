// The SQP dual solution: the multipliers of the equality-constrained QP of the last SQP iteration (the KKT system stated in tests/kkt_reference.py) at its full step
// (dx, du), with the symmetric parts of Q, R:
//     lambda_N = Q_N dx_N + q_N
//     lambda_k = Q_k dx_k + q_k + A_k' lambda_{k+1} + C_k' nu_k          k = N-1 .. 0        (the costate: the multiplier of the dynamics row that ends in node k)
//     0        = R_k du_k + r_k + B_k' lambda_{k+1} + D_k' nu_k          k = 0 .. N-1        (nu_k: the multipliers of C_k dx + D_k du + e_k = 0)
//
//   costate_kernel            lambda_k, k = N .. 0, from what every solve leaves in HBM: the projected stage records, the projected gains [K~ | k~] and the step dX.
//                             The dynamics multipliers of the projected QP (du = Pe + Px dx + Pu du~, equality-free) and of the original one coincide, and on the
//                             projected QP   lambda_k = Q~ dx + P~' du~ + q~ + A~' lambda_{k+1},   0 = rho_k := R~ du~ + P~ dx + r~ + B~' lambda_{k+1},   du~ = K~ dx + k~.
//   dual_multiplier_kernel    nu_k from the un-projected blocks of the LQ dump (qmgpu_enable_debug), the step dU and lambda_{k+1}:  D_k' nu_k = -g_k in the
//                             least-squares sense, g_k = R_k du_k + r_k + B_k' lambda_{k+1}.  D_k has full row rank, so nu_k is unique.
//
// The recursion kept is the CLOSED-LOOP form
//     lambda_k = Q~ dx + P~' du~ + q~ + A~' lambda_{k+1} + K~' rho_k
// which adds K~' times a quantity that is zero in exact arithmetic.  A rounding error d of lambda_{k+1} then reaches lambda_k as (A~ + B~ K~)' d = A_cl' d instead of
// the open-loop A~' d (spectral radius above one), whose growth over N = 200 nodes value_kernel.h records for the short form of the value recursion.  rho_k itself is a
// by-product worth having: it is the stationarity residual of the stored step, of rounding size for a sound solve.
//
// costate_kernel: one workgroup of four wavefronts per instance, sequential from node N down to 0.  The sums are 30 / MT terms long: one lane per row, operands from LDS.
//   S1   wavefront 0: du~ = K~ dx + k~ (rows >= m~ zero)                     wavefront 1: t = q~ + Q~ dx + A~' lambda_{k+1}
//   S2   wavefront 0: rho = r~ + R~ du~ + P~ dx + B~' lambda_{k+1}            wavefront 1: t += P~' du~
//   S3   wavefront 1: lambda_k = t + K~' rho -> LDS, HBM                     all: the record, the gains and dx of node k - 1 land in LDS
// The record and the gains of node k - 1 are in flight in registers of all four wavefronts while node k is computed (StagePrefetch), their joint rows landing as
// A~ = e_i + dt Px, B~ = dt Pu (commitDynamics).  Rows >= m~ of P~ / r~ / R~ are not written by lq_node_kernel: they are masked with m~ = 30 - constraintCount(mode)
// (contact_rows.h; the mode rides in the record).  Only the upper triangle of Q~ and the lower triangle of R~ are stored.
//
// dual_multiplier_kernel: one wavefront per (instance, node k < N).  Lane i < 30 forms g_i; lane j < nc then owns column j of D' (row j of the dump's D, 30 numbers in
// registers) and lane NCMAX the right-hand side -g: the Householder QR of lq_node_kernel's projection -- every lane builds the reflector of step c from column c, fetched
// with v_readlane, and applies it to its own column; no LDS, no reduction across lanes -- leaves R1[r][c] in lane c, register r, and Q'(-g) in lane NCMAX.  Back
// substitution by columns gives nu.  Rows >= nc of nu are written as zero.
#pragma once
#include "gpu_rt.h"
#include "layout.h"
#include "contact_rows.h"
#include "riccati_kernel.h"   // StagePrefetch, jointRowMask
#include "dual_lds.h"

namespace qmk {

struct DualArgs {
  int batch, N;
  const real* stages;      // [batch][N+1][STAGE_DOUBLES]
  const real* gains;       // [batch][N][GAIN_DOUBLES]
  const real* dtgrid;      // [batch][N+1]
  const real* instStats;   // [batch][4]: [1] = status of the backward sweep (out_stats[7])
  const real* dX;          // [batch][N+1][30] the full step
  const real* dU;          // [batch][N][30]
  const real* debug;       // [batch][N+1][DBG_DOUBLES] the LQ dump of the solve, or null (costates only)
  const int* stageNc;      // [batch][N+1]
  double* costate;         // [batch][N+1][30]
  double* nu;              // [batch][N][NCMAX] or null
  int* nc;                 // [batch][N] or null
  int* status;             // [batch] or null
};

constexpr int DUAL_WAVES = 4, DUAL_THREADS = DUAL_WAVES * 64;
constexpr int DUAL_PF_STG = (DUAL_STG / 2 + DUAL_THREADS - 1) / DUAL_THREADS;      // 7 units of 16 bytes per thread
constexpr int DUAL_PF_GN = (GAIN_DOUBLES / 2 + DUAL_THREADS - 1) / DUAL_THREADS;   // 2

__global__ void __launch_bounds__(DUAL_THREADS) costate_kernel(DualArgs a) {
  QM_DYNAMIC_LDS(lds);
  QM_POISON_LDS(lds, DUAL_LDS_REALS);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int inst = blockIdx.x, N = a.N;
  if (inst >= a.batch) return;
  double* lamOut = a.costate + size_t(inst) * (N + 1) * 30;
  // a failed factorisation (workgroup uniform) leaves gains and a step that may hold inf / NaN: the instance gets zeros
  const bool failed = !(a.instStats[size_t(inst) * 4 + 1] == 0.0_r);
  if (a.status && tid == 0) a.status[inst] = failed ? 1 : 0;
  if (failed) {
    for (int e = tid; e < (N + 1) * 30; e += DUAL_THREADS) lamOut[e] = 0.0;
    return;
  }
  real* STG = lds + DL_STG.off; real* LAM = lds + DL_LAM.off; real* DX = lds + DL_DX.off; real* DU = lds + DL_DU.off; real* RHO = lds + DL_RHO.off;
  const real* stagesI = a.stages + size_t(inst) * (N + 1) * STAGE_DOUBLES;
  const real* gainsI = a.gains + size_t(inst) * N * GAIN_DOUBLES;
  const real* dXI = a.dX + size_t(inst) * (N + 1) * 30;
  const unsigned long long jm = jointRowMask<DUAL_PF_STG, DUAL_THREADS>(tid);   // which of my units of the staged copy are joint-row entries
  StagePrefetch<DUAL_PF_STG, DUAL_THREADS> pf;
  StagePrefetch<DUAL_PF_GN, DUAL_THREADS> pg;
  const int li = lane < 30 ? lane : 0, lj = lane < MT ? lane : 0;   // my state row / projected-input row (clamped: lanes beyond compute on row 0 and store nothing)
  const int xi = tid - 2 * 64;                                      // wavefront 2 fetches dx of the next node

  // ---- terminal node: lambda_N = sym(Q_N) dx_N + q_N, straight from HBM; the record and the gains of node N - 1 are requested first and land behind it
  {
    pf.issue(stagesI + size_t(N - 1) * STAGE_DOUBLES, DUAL_STG, tid);
    pg.issue(gainsI + size_t(N - 1) * GAIN_DOUBLES, GAIN_DOUBLES, tid);
    const real dtLast = a.dtgrid[size_t(inst) * (N + 1) + N - 1];
    const real dxk = dXI[size_t(N - 1) * 30 + (xi >= 0 && xi < 30 ? xi : 0)];
    if (wave == 1) {
      const real* rec = stagesI + size_t(N) * STAGE_DOUBLES;
      const real* dxN = dXI + size_t(N) * 30;
      real t = rec[OFF_qt + li];
#pragma unroll 6
      for (int c = 0; c < 30; ++c) t = fma(0.5_r * (rec[OFF_QT + li * 30 + c] + rec[OFF_QT + c * 30 + li]), dxN[c], t);
      if (lane < DUAL_VEC) LAM[lane] = lane < 30 ? t : 0.0_r;
      if (lane < 30) lamOut[size_t(N) * 30 + lane] = double(t);
    }
    if (xi >= 0 && xi < DUAL_VEC) DX[xi] = xi < 30 ? dxk : 0.0_r;
    pf.commitDynamics(STG, DUAL_STG, tid, jm, dtLast);
    pg.commit(lds + DL_GN.off + ((N - 1) & 1) * GAIN_DOUBLES, GAIN_DOUBLES, tid);
  }
  __syncthreads();

#pragma unroll 1
  for (int k = N - 1; k >= 0; --k) {
    // STG, GN[k & 1], DX: node k;  LAM: lambda_{k+1}.  Node k - 1 is requested before anything else
    if (k > 0) {
      pf.issue(stagesI + size_t(k - 1) * STAGE_DOUBLES, DUAL_STG, tid);
      pg.issue(gainsI + size_t(k - 1) * GAIN_DOUBLES, GAIN_DOUBLES, tid);
    }
    const real dxPrev = dXI[size_t(k > 0 ? k - 1 : 0) * 30 + (xi >= 0 && xi < 30 ? xi : 0)];
    const real* GN = lds + DL_GN.off + (k & 1) * GAIN_DOUBLES;
    const int nt = 30 - constraintCount(int(STG[OFF_MODE]));   // m~ of the node (workgroup uniform)
    const real dtPrev = STG[OFF_DTPREV];                       // the step of node k - 1, whose record lands in S3
    real t = 0.0_r;
    // ---- S1
    if (wave == 0) {
      real du = GN[OFF_kff + lj];
#pragma unroll
      for (int c = 0; c < 30; ++c) du = fma(GN[OFF_KFB + lj * 30 + c], DX[c], du);
      if (lane < DUAL_VEC) DU[lane] = lane < nt ? du : 0.0_r;   // rows >= m~ of the gains are zero padding; masked all the same
    } else if (wave == 1) {
      t = STG[OFF_qt + li];
#pragma unroll
      for (int c = 0; c < 30; ++c) t = fma(STG[OFF_QT + (c < li ? c * 30 + li : li * 30 + c)], DX[c], t);   // only the upper triangle of the symmetric Q~ is stored
#pragma unroll
      for (int r = 0; r < 30; ++r) t = fma(STG[OFF_AT + r * 30 + li], LAM[r], t);                            // A~'[i][r] = A~[r][i]
    }
    QM_LDS_BARRIER();
    // ---- S2
    if (wave == 0) {
      real rho = STG[OFF_rt + lj];
#pragma unroll
      for (int c = 0; c < MT; ++c) {
        const real rv = STG[OFF_RT + (lj >= c ? lj * MT + c : c * MT + lj)];   // R~ is stored as its lower triangle; rows / columns >= m~ are not written
        rho = fma(c < nt ? rv : 0.0_r, DU[c], rho);
      }
#pragma unroll
      for (int c = 0; c < 30; ++c) rho = fma(STG[OFF_PT + lj * 30 + c], DX[c], rho);
#pragma unroll
      for (int r = 0; r < 30; ++r) rho = fma(STG[OFF_BT + r * MT + lj], LAM[r], rho);   // B~'[j][r] = B~[r][j]
      if (lane < DUAL_VEC) RHO[lane] = lane < nt ? rho : 0.0_r;                           // rows >= m~ of P~ / r~ / R~ are not written: whatever they gave is dropped here
    } else if (wave == 1) {
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        const real pv = STG[OFF_PT + j * 30 + li];                                        // P~'[i][j] = P~[j][i]
        t = fma(j < nt ? pv : 0.0_r, DU[j], t);
      }
    }
    QM_LDS_BARRIER();
    // ---- S3: nobody reads STG, DX or the other half of GN any more; LAM was last read in S2
    if (wave == 1) {
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        const real kv = GN[OFF_KFB + j * 30 + li];                                        // K~'[i][j] = K~[j][i]
        t = fma(j < nt ? kv : 0.0_r, RHO[j], t);
      }
      if (lane < 30) { LAM[lane] = t; lamOut[size_t(k) * 30 + lane] = double(t); }
    }
    if (k > 0) {
      if (xi >= 0 && xi < 30) DX[xi] = dxPrev;
      pf.commitDynamics(STG, DUAL_STG, tid, jm, dtPrev);
      pg.commit(lds + DL_GN.off + ((k - 1) & 1) * GAIN_DOUBLES, GAIN_DOUBLES, tid);
    }
    QM_LDS_BARRIER();
  }
}

// One reflector step of the QR of D' (columns in lanes 0 .. nc - 1, the right-hand side in lane NCMAX): as the projection's QR in lq_node_kernel, 30 rows.
template <int C> __device__ __forceinline__ void dualReflect(real (&col)[30], int lane) {
  real v[30];
  real n2a = 0.0_r, n2b = 0.0_r;
#pragma unroll
  for (int i = C; i < 30; ++i) { v[i] = qmReadLane(col[i], C); if ((i - C) & 1) n2b += v[i] * v[i]; else n2a += v[i] * v[i]; }
  // reflector v = column - alpha e_C, alpha = -sign(d_C) |column|; beta = 2 / v'v = 1 / (|column| |v_C|)
  const real dc = v[C], n2 = n2a + n2b;
  const real nrm = sqrt(n2);
  const real alpha = dc > 0.0_r ? -nrm : nrm;
  v[C] = dc - alpha;
  const real den = nrm * fabs(v[C]);
  const real beta = den > 0.0_r ? 1.0_r / den : 0.0_r;
  real sa = 0.0_r, sb = 0.0_r;
#pragma unroll
  for (int i = C; i < 30; ++i) { if ((i - C) & 1) sb += v[i] * col[i]; else sa += v[i] * col[i]; }
  const real sf = (sa + sb) * beta;
#pragma unroll
  for (int i = C; i < 30; ++i) col[i] -= sf * v[i];
  col[C] = lane == C ? alpha : col[C];   // R1[C][C] exactly; the entries below it in lane C (rounding residue instead of zeros) are never read
}

__global__ void __launch_bounds__(64) dual_multiplier_kernel(DualArgs a) {
  const int lane = threadIdx.x, N = a.N;
  const int inst = blockIdx.x / N, k = blockIdx.x - inst * N;
  if (inst >= a.batch) return;
  const size_t node = size_t(inst) * (N + 1) + k, at = size_t(inst) * N + k;
  const int ncRaw = a.stageNc[node], nc = ncRaw < 0 ? 0 : (ncRaw > NCMAX ? NCMAX : ncRaw);   // (12 .. 16 from lq_node_kernel; the clamp keeps every index in range whatever it finds)
  if (a.nc && lane == 0) a.nc[at] = nc;
  if (!a.nu) return;
  const bool failed = !(a.instStats[size_t(inst) * 4 + 1] == 0.0_r);   // (wavefront uniform)
  if (failed) {
    if (lane < NCMAX) a.nu[at * NCMAX + lane] = 0.0;
    return;
  }
  const real* dbg = a.debug + node * DBG_DOUBLES;
  const real* du = a.dU + at * 30;
  const double* lamNext = a.costate + (node + 1) * 30;
  const int li = lane < 30 ? lane : 0;
  // g_i = r_i + sum_c sym(R)[i][c] du_c + sum_r B[r][i] lambda_{k+1}[r]
  real g = dbg[DBG_r + li];
#pragma unroll 6
  for (int c = 0; c < 30; ++c) g = fma(0.5_r * (dbg[DBG_R + li * 30 + c] + dbg[DBG_R + c * 30 + li]), du[c], g);
#pragma unroll 6
  for (int r = 0; r < 30; ++r) g = fma(dbg[DBG_B + r * 30 + li], real(lamNext[r]), g);
  // my column: row `lane` of D (rows >= nc of the dump are not written), -g in lane NCMAX, zero elsewhere
  real col[30];
  const int lr = lane < nc ? lane : 0;
#pragma unroll
  for (int i = 0; i < 30; ++i) {
    const real dv = dbg[DBG_D + lr * 30 + i];
    const real gi = qmReadLane(g, i);
    col[i] = lane < nc ? dv : (lane == NCMAX ? -gi : 0.0_r);
  }
  // the steps written out: every register index and every v_readlane source is a constant
#define QM_DUAL_STEP(C) if (C < nc) dualReflect<C>(col, lane);
  QM_DUAL_STEP(0) QM_DUAL_STEP(1) QM_DUAL_STEP(2) QM_DUAL_STEP(3) QM_DUAL_STEP(4) QM_DUAL_STEP(5) QM_DUAL_STEP(6) QM_DUAL_STEP(7)
  QM_DUAL_STEP(8) QM_DUAL_STEP(9) QM_DUAL_STEP(10) QM_DUAL_STEP(11) QM_DUAL_STEP(12) QM_DUAL_STEP(13) QM_DUAL_STEP(14) QM_DUAL_STEP(15)
#undef QM_DUAL_STEP
  static_assert(NCMAX == 16, "sixteen reflector steps");
  // R1 nu = y, y = rows 0 .. nc - 1 of lane NCMAX; R1[r][c] (r <= c) lives in lane c, register r: by columns from the last one, every lane computes nu_c,
  // lane NCMAX takes column c out of its y
  real mine = 0.0_r;
#pragma unroll
  for (int c = NCMAX - 1; c >= 0; --c) {
    if (c < nc) {
      const real yc = qmReadLane(col[c], NCMAX), rcc = qmReadLane(col[c], c);
      const real x = rcc != 0.0_r ? yc / rcc : 0.0_r;
      mine = lane == c ? x : mine;
#pragma unroll
      for (int r = 0; r < c; ++r) { const real rrc = qmReadLane(col[r], c); col[r] = lane == NCMAX ? fma(-rrc, x, col[r]) : col[r]; }
    }
  }
  if (lane < NCMAX) a.nu[at * NCMAX + lane] = double(mine);
}

}  // namespace qmk
