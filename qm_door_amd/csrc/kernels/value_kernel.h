// The SQP value function: what upstream's SqpSolver keeps when sqp.createValueFunction is set (SqpSolver::extractValueFunction: hpipm's getRiccatiCostToGo,
// re-centred on the linearisation state) and what SqpSolver::getValueFunction(time, state) makes of it.
//
//   value_function_kernel     V_k(dx) = 1/2 dx' Sm_k dx + sv_lin_k' dx (+ const), the optimal cost of the equality-constrained QP over nodes k .. N of the last SQP
//                             iteration with dx_k = dx, k = N .. 0;  Sv_k = sv_lin_k - Sm_k x_lin_k, so that dfdx(x) = Sv_k + Sm_k x
//   value_eval_kernel         dfdxx = Sm(t), dfdx = Sv(t) + Sm(t) x, interpolated with the index and alpha of policy_eval_kernel
//
// riccati_kernel forms S_k on its way and drops it (it sits at its LDS and register limits).  Everything the recursion needs is in HBM
// after a solve: the projected stage records, the projected gains [K~ | k~] and the iterate.  With the gains known nothing is factorised.  The recursion is the
// Joseph form -- the cost of the stored policy du~ = K~ dx + k~ --, with A_cl = A~ + B~ K~, b_cl = b~ + B~ k~:
//   P1  [A_cl | b_cl] = [A~ | b~] + B~ [K~ | k~]  (in place)         30 x 31;      W = [P~ | r~] + R~ [K~ | k~]      m~ x 31
//   P2  Y = S+ [A_cl | b_cl]  (+ s+ in column 30)                   32 x 32, S+ with s+ as row 30 and a unit entry at (30, 30) of the right factor, as the sweep's P1
//   P3  [S | s] = [Q~ | q~] + A_cl^T Y + P~^T [K~ | k~] + K~^T W     30 x 31
//   P4  S <- (S + S^T) / 2, s -> row 30 of S                        the whole update is symmetrised (the sweep symmetrises P6a and subtracts a bit-symmetric W^T W)
// The short form S = Q~ + A~^T S+ A~ + G^T K~, s = q~ + A~^T (S+ b~ + s+) + G^T k~ with G = P~ + B~^T S+ A~ was built first.  It takes the gains as given, so a
// rounding error of s+ is carried on by the OPEN-loop A~^T (spectral radius above one) instead of A_cl^T: sv_lin of node 0 was off by 2.7e-10 at N = 200 where the
// reference allows 9e-13 (Sm, which keeps one closed-loop factor, was not).  The Joseph form is exact for any gains, second-order insensitive to their error, and
// carries every error on through A_cl on both sides.
// One workgroup of four wavefronts per instance, sequential from node N down to 0 -- the dependent chain of the backward sweep without its factorisation.  Each
// product is four 16 x 16 tiles, one per wavefront, on the fp64 matrix cores.  The record and the gains of node k - 1 are in flight in registers while node k is
// computed (StagePrefetch) and land in LDS in P4, their joint rows as A~ = e_i + dt Px, B~ = dt Pu (commitDynamics).  Rows >= m~ of P~ / r~ / R~ are not written by
// lq_node_kernel: they are masked with m~ = 30 - constraintCount(mode) (contact_rows.h; the mode rides in the record).  Columns >= m~ of B~ and rows >= m~ of the gains
// are zero padding.  Rows 0..11 of Px / Pu (force inputs) do not enter: the state rows 0..11 of A~ / B~ are stored dense.  Only the upper triangle of Q~ and the lower
// triangle of R~ are stored.
#pragma once
#include "gpu_rt.h"
#include "layout.h"
#include "contact_rows.h"
#include "riccati_kernel.h"   // StagePrefetch, jointRowMask
#include "schedule_dev.h"
#include "value_lds.h"

namespace qmk {

struct ValueArgs {
  int batch, N;
  const real* stages;      // [batch][N+1][STAGE_DOUBLES]
  const real* gains;       // [batch][N][GAIN_DOUBLES]
  const real* dtgrid;      // [batch][N+1]
  const real* instStats;   // [batch][4]: [1] = status of the backward sweep (out_stats[7])
  const real* X;           // [batch][N+1][30] the iterate the records were linearised at
  double* Sm;              // [batch][N+1][30][30]
  double* Sv;              // [batch][N+1][30]
  double* svLin;           // [batch][N+1][30] or null
  double* xLin;            // [batch][N+1][30] or null
  int* status;             // [batch] or null
};

constexpr int VALUE_WAVES = 4, VALUE_THREADS = VALUE_WAVES * 64;
constexpr int VALUE_PF_STG = (VALUE_STG / 2 + VALUE_THREADS - 1) / VALUE_THREADS;     // 7 units of 16 bytes per thread
constexpr int VALUE_PF_GN = (GAIN_DOUBLES / 2 + VALUE_THREADS - 1) / VALUE_THREADS;   // 2

// node `node` out: Sm as one contiguous run of 900 doubles by the whole workgroup; Sv, sv_lin, x_lin by lanes 0..29 of the last wavefront
__device__ __forceinline__ void valueEmitNode(const ValueArgs& a, const real* lds, int inst, int node, int tid) {
  const real* S = lds + VL_S.off; const real* XL = lds + VL_X.off;
  const size_t at = size_t(inst) * (a.N + 1) + node;
  double* So = a.Sm + at * 900;
#pragma unroll
  for (int p = 0; p < (900 + VALUE_THREADS - 1) / VALUE_THREADS; ++p) {
    const int e = tid + p * VALUE_THREADS, i = e / 30, j = e - 30 * i;
    if (e < 900) QM_STREAM_STORE(So + e, double(S[i * LDS_S + j]));
  }
  const int li = tid - (VALUE_THREADS - 64);
  if (li >= 0 && li < 30) {
    const real sl = S[30 * LDS_S + li];
    real acc = sl;
#pragma unroll
    for (int c = 0; c < 30; ++c) acc = fma(-S[li * LDS_S + c], XL[c], acc);
    a.Sv[at * 30 + li] = double(acc);
    if (a.svLin) a.svLin[at * 30 + li] = double(sl);
    if (a.xLin) a.xLin[at * 30 + li] = double(XL[li]);
  }
}

__global__ void __launch_bounds__(VALUE_THREADS) value_function_kernel(ValueArgs a) {
  QM_DYNAMIC_LDS(lds);
  QM_POISON_LDS(lds, VALUE_LDS_REALS);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, h = lane >> 4, la = qmARow(l16);   // MFMA operand coordinates of this lane (gpu_rt.h)
  const int inst = blockIdx.x, N = a.N;
  if (inst >= a.batch) return;
  const real* XI = a.X + size_t(inst) * (N + 1) * 30;
  // a failed factorisation (workgroup uniform) leaves gains that may hold inf / NaN: the instance gets zeros, and its linearisation states
  const bool failed = !(a.instStats[size_t(inst) * 4 + 1] == 0.0_r);
  if (a.status && tid == 0) a.status[inst] = failed ? 1 : 0;
  if (failed) {
    double* So = a.Sm + size_t(inst) * (N + 1) * 900;
    for (int e = tid; e < (N + 1) * 900; e += VALUE_THREADS) QM_STREAM_STORE(So + e, 0.0);
    for (int e = tid; e < (N + 1) * 30; e += VALUE_THREADS) {
      const size_t at = size_t(inst) * (N + 1) * 30 + e;
      a.Sv[at] = 0.0;
      if (a.svLin) a.svLin[at] = 0.0;
      if (a.xLin) a.xLin[at] = double(XI[e]);
    }
    return;
  }
  real* STG = lds + VL_STG.off; real* GN = lds + VL_GN.off; real* S = lds + VL_S.off; real* Y = lds + VL_Y.off;
  real* G = lds + VL_G.off; real* Cs = lds + VL_C.off; real* XL = lds + VL_X.off;
  const real* stagesI = a.stages + size_t(inst) * (N + 1) * STAGE_DOUBLES;
  const real* gainsI = a.gains + size_t(inst) * N * GAIN_DOUBLES;
  const unsigned long long jm = jointRowMask<VALUE_PF_STG, VALUE_THREADS>(tid);   // which of my units of the staged copy are joint-row entries
  StagePrefetch<VALUE_PF_STG, VALUE_THREADS> pf;
  StagePrefetch<VALUE_PF_GN, VALUE_THREADS> pg;

  // ---- terminal node: S_N = sym(Q_N), s_N = q_N as row 30, zero padding; the record and the gains of node N - 1 are requested first and land behind it
  {
    pf.issue(stagesI + size_t(N - 1) * STAGE_DOUBLES, VALUE_STG, tid);
    pg.issue(gainsI + size_t(N - 1) * GAIN_DOUBLES, GAIN_DOUBLES, tid);
    const real dtLast = a.dtgrid[size_t(inst) * (N + 1) + N - 1];
    const real* rec = stagesI + size_t(N) * STAGE_DOUBLES;
    constexpr int NS = (32 * LDS_S + VALUE_THREADS - 1) / VALUE_THREADS;
    real sv[NS], sw[NS];   // all of a thread's loads before its first LDS store
#pragma unroll
    for (int q = 0; q < NS; ++q) {
      const int e = tid + q * VALUE_THREADS, i = e / LDS_S, j = e % LDS_S;
      const bool inQ = e < 32 * LDS_S && i < 30 && j < 30, inq = e < 32 * LDS_S && i == 30 && j < 30;
      sv[q] = (inQ || inq) ? rec[inq ? OFF_qt + j : OFF_QT + i * 30 + j] : 0.0_r;
      sw[q] = inQ ? rec[OFF_QT + j * 30 + i] : sv[q];
    }
    const real xl = XI[size_t(N) * 30 + (tid < 30 ? tid : 0)];
#pragma unroll
    for (int q = 0; q < NS; ++q) { QM_KEEP(sv[q]); QM_KEEP(sw[q]); }
#pragma unroll
    for (int q = 0; q < NS; ++q) { const int e = tid + q * VALUE_THREADS; if (e < 32 * LDS_S) S[e] = 0.5_r * (sv[q] + sw[q]); }
    if (tid < 32) XL[tid] = tid < 30 ? xl : 0.0_r;
    pf.commitDynamics(STG, VALUE_STG, tid, jm, dtLast);
    pg.commit(GN, GAIN_DOUBLES, tid);
  }
  __syncthreads();

  const int tm = wave >> 1, tn = wave & 1;     // my 16 x 16 tile of every product
  const int jc = tn * 16 + l16;                // my column of Y, [G | g] and C
  const int xi = tid - (VALUE_THREADS - 64);   // (the lanes that write Sv: valueEmitNode)
#pragma unroll 1
  for (int k = N - 1; k >= 0; --k) {
    // S, XL: node k + 1;  STG, GN: node k.  Node k - 1 is requested before anything else; node k + 1 goes out while P1 reads S
    if (k > 0) {
      pf.issue(stagesI + size_t(k - 1) * STAGE_DOUBLES, VALUE_STG, tid);
      pg.issue(gainsI + size_t(k - 1) * GAIN_DOUBLES, GAIN_DOUBLES, tid);
    }
    const real xNext = XI[size_t(k) * 30 + (xi >= 0 && xi < 30 ? xi : 0)];
    valueEmitNode(a, lds, inst, k + 1, tid);
    const int nt = 30 - constraintCount(int(STG[OFF_MODE]));   // m~ of the node (workgroup uniform)
    // ---- P1: [A_cl | b_cl] = [A~ | b~] + B~ [K~ | k~] in place (every entry is read and written by one lane); W = [P~ | r~] + R~ [K~ | k~], rows >= m~ zero
    {
      const int ia = tm * 16 + la, iac = ia < 30 ? ia : 29, iw = ia < MT ? ia : 0;
      real av[VALUE_G_ROWS / 4], rv[VALUE_G_ROWS / 4], kv[VALUE_G_ROWS / 4];
#pragma unroll
      for (int ks = 0; ks < VALUE_G_ROWS / 4; ++ks) {
        const int kk = 4 * ks + h, kc = kk < MT ? kk : 0;
        const real vb = STG[OFF_BT + iac * MT + kc];                                   // columns >= m~ of B~ are zero padding; masked all the same
        av[ks] = (ia < 30 && kk < nt) ? vb : 0.0_r;
        const real vr = STG[OFF_RT + (iw >= kc ? iw * MT + kc : kc * MT + iw)];         // R~ is stored as its lower triangle (lq_node_kernel); rows / columns >= m~ are not written
        rv[ks] = (ia < nt && kk < nt) ? vr : 0.0_r;
        const real vk = GN[jc < 30 ? OFF_KFB + kc * 30 + jc : OFF_kff + kc];            // rows >= m~ of the gains are zero
        kv[ks] = (kk < MT && jc <= 30) ? vk : 0.0_r;
      }
      QmAcc c, w;
      int dst[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = tm * 16 + h + 4 * r, ic = i < 30 ? i : 29, iv = i < MT ? i : 0;
        dst[r] = jc < 30 ? OFF_AT + ic * 30 + jc : OFF_bt + ic;
        const real vm = STG[dst[r]];
        c[r] = (i < 30 && jc <= 30) ? vm : 0.0_r;
        const real vp = STG[jc < 30 ? OFF_PT + iv * 30 + jc : OFF_rt + iv];            // rows >= m~ of P~ / r~ are not written
        w[r] = (i < nt && jc <= 30) ? vp : 0.0_r;
      }
#pragma unroll
      for (int ks = 0; ks < VALUE_G_ROWS / 4; ++ks) { qmMfma(c, av[ks], kv[ks]); qmMfma(w, rv[ks], kv[ks]); }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = tm * 16 + h + 4 * r;
        if (i < 30 && jc <= 30) STG[dst[r]] = c[r];
        if (i < VALUE_G_ROWS) G[i * LDS_VG + jc] = w[r];
      }
    }
    QM_LDS_BARRIER();
    // ---- P2: Y = S+ M, M = [A_cl | b_cl] with the unit entry at (30, 30) that picks s+ out of row 30 of S
    {
      const bool jA = jc < 30, jb = jc == 30;
      real av[8], bv[8];
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const int kk = 4 * ks + h, kc = kk < 30 ? kk : 29;
        av[ks] = S[kk * LDS_S + tm * 16 + la];                 // S is symmetric: S[i][k] read as S[k][i]; row 30 is s+
        const real v = STG[jA ? OFF_AT + kc * 30 + jc : (jb ? OFF_bt + kc : 0)];
        bv[ks] = (kk < 30 && (jA || jb)) ? v : ((kk == 30 && jb) ? 1.0_r : 0.0_r);
      }
      QmAcc c;
#pragma unroll
      for (int r = 0; r < 4; ++r) c[r] = 0.0_r;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) qmMfma(c, av[ks], bv[ks]);
#pragma unroll
      for (int r = 0; r < 4; ++r) Y[(tm * 16 + h + 4 * r) * LDS_VY + jc] = c[r];
    }
    QM_LDS_BARRIER();
    // ---- P3: C = [Q~ | q~] + A_cl^T Y + P~^T [K~ | k~] + K~^T W
    const real dtPrev = STG[OFF_DTPREV];   // the step of node k - 1, whose record lands in P4
    {
      const int ia = tm * 16 + la, iac = ia < 30 ? ia : 29;
      real av[8], bv[8], pv[VALUE_G_ROWS / 4], kv[VALUE_G_ROWS / 4], kt[VALUE_G_ROWS / 4], wv[VALUE_G_ROWS / 4];
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const int kk = 4 * ks + h, kc = kk < 30 ? kk : 29;    // rows 30, 31 of Y are zero
        const real v = STG[OFF_AT + kc * 30 + iac];          // A_cl^T[i][k] = A_cl[k][i]
        av[ks] = (ia < 30 && kk < 30) ? v : 0.0_r;
        bv[ks] = Y[kk * LDS_VY + jc];
      }
#pragma unroll
      for (int ks = 0; ks < VALUE_G_ROWS / 4; ++ks) {
        const int kk = 4 * ks + h, kc = kk < MT ? kk : 0;
        const real vp = STG[OFF_PT + kc * 30 + iac];         // P~^T[i][r] = P~[r][i]
        pv[ks] = (ia < 30 && kk < nt) ? vp : 0.0_r;
        const real vk = GN[jc < 30 ? OFF_KFB + kc * 30 + jc : OFF_kff + kc];
        kv[ks] = (kk < MT && jc <= 30) ? vk : 0.0_r;
        const real vt = GN[OFF_KFB + kc * 30 + iac];         // K~^T[i][r] = K~[r][i]
        kt[ks] = (ia < 30 && kk < MT) ? vt : 0.0_r;
        wv[ks] = G[kk * LDS_VG + jc];
      }
      QmAcc c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = tm * 16 + h + 4 * r, ic = i < 30 ? i : 0, jq = jc < 30 ? jc : 0;
        const real qv = STG[OFF_QT + (jq < ic ? jq * 30 + ic : ic * 30 + jq)];   // only the upper triangle of the symmetric Q~ is stored (lq_node_kernel)
        const real qq = STG[OFF_qt + ic];
        c[r] = i < 30 ? (jc < 30 ? qv : (jc == 30 ? qq : 0.0_r)) : 0.0_r;
      }
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) qmMfma(c, av[ks], bv[ks]);
#pragma unroll
      for (int ks = 0; ks < VALUE_G_ROWS / 4; ++ks) { qmMfma(c, pv[ks], kv[ks]); qmMfma(c, kt[ks], wv[ks]); }
#pragma unroll
      for (int r = 0; r < 4; ++r) Cs[(tm * 16 + h + 4 * r) * LDS_VC + jc] = c[r];
    }
    QM_LDS_BARRIER();
    // ---- P4: S = (C + C^T) / 2 (the same sum on both sides of the diagonal: symmetric bit for bit), s as row 30; node k - 1 lands in the staging buffers
#pragma unroll
    for (int p = 0; p < (900 + VALUE_THREADS - 1) / VALUE_THREADS; ++p) {
      const int e = tid + p * VALUE_THREADS, i = e / 30, j = e - 30 * i;
      if (e < 900) S[i * LDS_S + j] = 0.5_r * (Cs[i * LDS_VC + j] + Cs[j * LDS_VC + i]);
    }
    if (tid < 30) S[30 * LDS_S + tid] = Cs[tid * LDS_VC + 30];
    if (xi >= 0 && xi < 30) XL[xi] = xNext;
    if (k > 0) {
      pf.commitDynamics(STG, VALUE_STG, tid, jm, dtPrev);
      pg.commit(GN, GAIN_DOUBLES, tid);
    }
    QM_LDS_BARRIER();
  }
  valueEmitNode(a, lds, inst, 0, tid);
}

// SqpSolver::getValueFunction(time, state): dfdxx = Sm(t), dfdx = Sv(t) + Sm(t) x, Sm and Sv interpolated linearly with the index and alpha policy_eval_kernel uses
// (end values held; N + 1 entries, so index + 1 <= N needs no clamp).  One wavefront per instance: all lanes write dfdxx as one contiguous run, lanes 0..29 form the
// rows of dfdx.  The interpolated entries are rounded as products and a sum of their own (no fused multiply-add), as the plain statement of the formula rounds
// them (policy_feedback_kernel gives the reason) -- and so both sides of the diagonal of dfdxx round alike: it is symmetric bit for bit.
__global__ void __launch_bounds__(64) value_eval_kernel(int batch, int N, const real* tgrid, const real* Sm, const real* Sv, const real* tEval, const real* x, real* dfdx,
                                                        real* dfdxx) {
  const int inst = blockIdx.x, lane = threadIdx.x;
  if (inst >= batch) return;
  const real* tg = tgrid + size_t(inst) * (N + 1);
  const real t = tEval[inst];
  int idx; real alpha;
  timeSegmentWave(tg, N + 1, t, lane, idx, alpha);
  const real beta = 1.0_r - alpha;
  const real* Sl = Sm + (size_t(inst) * (N + 1) + idx) * 900;   // Sm_idx; Sm_{idx + 1} follows 900 entries later
  real* Ho = dfdxx + size_t(inst) * 900;
#pragma unroll
  for (int p = 0; p < 15; ++p) {
    const int e = lane + 64 * p, ec = e < 900 ? e : 0;
    const real v = qmMulNoFma(alpha, Sl[ec]) + qmMulNoFma(beta, Sl[900 + ec]);
    if (e < 900) QM_STREAM_STORE(Ho + e, v);
  }
  if (lane < 30) {
    const real* vl = Sv + (size_t(inst) * (N + 1) + idx) * 30;
    const real* row = Sl + lane * 30;
    const real* xm = x + size_t(inst) * 30;
    real s = qmMulNoFma(alpha, vl[lane]) + qmMulNoFma(beta, vl[30 + lane]);
#pragma unroll
    for (int c = 0; c < 30; ++c) {
      const real st = qmMulNoFma(alpha, row[c]) + qmMulNoFma(beta, row[900 + c]);
      s = fma(st, xm[c], s);
    }
    dfdx[size_t(inst) * 30 + lane] = s;
  }
}

}  // namespace qmk
