// metrics_kernel -- the OCP evaluated on a trajectory: per node the cost (and its seven terms), the RK2 defect and the values of the state-input equalities; per
// instance the PerformanceIndex they sum to.  Stateless: it reads the model, the settings and R' behind the handle and the caller's arrays, nothing a solve leaves.
//
// Replaces upstream SqpSolver::computePerformance: multiple_shooting::computeIntermediateMetrics / computeTerminalMetrics per node (Metrics::cost, ::dynamicsViolation,
// ::stateInputEqConstraint) and toPerformanceIndex(metrics, dt) over the horizon, evaluating the node terms assembled in qm_interface/src/QMInterface.cpp:99-131.
//
// The line search's shape: one workgroup per instance, ONE SHOOTING NODE PER LANE (value-only evaluation, T = real instantiation of the tree sweep the LQ kernel
// differentiates), lanes striding over the horizon in passes of METRICS_THREADS nodes.  Per pass
//   S1  the states and inputs of the pass's nodes land in LDS as flat, coalesced copies (a lane reading its own node's rows from HBM touches 90 places 240 bytes apart)
//   S2  every lane evaluates its node and leaves its defect, equality and cost-term rows in LDS; node_cost and nc, one word per lane, go straight out
//   S3  the three row arrays leave as flat copies: consecutive threads, consecutive addresses
// and at the end the per-thread partial sums are added by a fixed pairwise tree over the threads: with the thread count fixed, an order that depends on N only.
// The node evaluation restates linesearch_kernel.h's nodePerformance term by term (that function returns three scalars and is not touched); a node takes the mode that
// starts at its time (nodePhaseAt) and its step from the grid, exactly as mpc_init_kernel forms them, and the rows come in contact_rows.h's order.
#pragma once
#include "gpu_rt.h"
#include "layout.h"
#include "contact_rows.h"
#include "schedule_dev.h"
#include "sweep_dev.h"
#include "linesearch_kernel.h"   // DblIn
#include "metrics_lds.h"

namespace qmk {

struct MetricsArgs {
  const ProblemR* P;
  const real* Rw;          // R' [900] and the barrier constants behind it (layout.h: QM_RW_DERIVED)
  int batch, N, K;
  const real* tgrid;       // [batch][N+1]
  const real* X;           // [batch][N+1][30]
  const real* U;           // [batch][N][30]
  const real* x0;          // [batch][30] or null
  const real* targetTimes; const real* targetStates;
  const int* schedNum; const real* schedTimes; const int* schedModes;
  const real* eeContact;   // [batch][K][6] or null (force tracking)
  // outputs, each may be null
  real* nodeCost;          // [batch][N+1]
  real* costTerms;         // [batch][N+1][METRICS_TERMS]
  real* defect;            // [batch][N][30]
  real* eq;                // [batch][N][NCMAX]
  int* nc;                 // [batch][N]
  real* performance;       // [batch][METRICS_PERF]
};
constexpr int METRICS_PERF = 8;   // QMGPU_NPERF: merit, cost, dualFeasibilitiesSSE, dynamicsViolationSSE, equalityConstraintsSSE, inequalityConstraintsSSE, equalityLagrangian, inequalityLagrangian

// rows [first, first + rows) of a [.][width] HBM array <-> LDS rows of `stride` reals, flat: thread t takes elements t, t + THREADS, ...
__device__ __forceinline__ void metricsLoadRows(real* ldsRows, int stride, const real* src, int rows, int width, int tid) {
  for (int e = tid; e < rows * width; e += METRICS_THREADS) { const int r = e / width, c = e - r * width; ldsRows[r * stride + c] = src[e]; }
}
__device__ __forceinline__ void metricsStoreRows(real* dst, const real* ldsRows, int stride, int rows, int width, int tid) {
  for (int e = tid; e < rows * width; e += METRICS_THREADS) { const int r = e / width, c = e - r * width; dst[e] = ldsRows[r * stride + c]; }
}

// One node at (x, u, xnext): terms[0..7] (metrics_lds.h / qmgpu.h: the cost terms, NOT dt-scaled), the defect row rk2(x, u, dt) - xnext, the equality row (rows >= nc zero)
// and their squared norms.  Terminal node: terms[2] only; no defect, no equalities.  x, u, xnext, dRow, eRow: LDS.
// WP: pointer type of the two weight matrices (LDS, through QM_OPAQUE_LDS: one address register and immediate offsets for the 1800 reads).
// NOT inlined, as nodePerformance: inlined into the kernel the body took all 512 registers and 14,064 B of scratch per lane (929 spill stores); as a called function it
// takes 428 registers and 1,200 B, the callee-saved registers the call saves and restores with the interprocedural register allocation off (linesearch_kernel.h says
// what that costs there: 14 %).
template <class WP> __device__ __attribute__((noinline)) void metricsNode(const ModelR& md, const SettingsR& st, WP Qw, WP Rw, const real* bc, const Schedule& sched, const real* tTimes, const real* tStates,
                                   const real* contact, int K, real t, real dt, int phase, bool terminal, const real* x, const real* u, const real* xnext, real (&terms)[METRICS_TERMS],
                                   real* dRow, real* eRow, int& ncOut, real& dyn, real& eq) {
  const int mode = sched.modes[phase];
  real eePosRef[3], eeQuatRef[4];
  eeReference(tTimes, tStates, K, t, eePosRef, eeQuatRef);
  real Ke = 0.0_r, fRef[3] = {0.0_r, 0.0_r, 0.0_r}, pEnv[3] = {0.0_r, 0.0_r, 0.0_r};   // force tracking (own formulation), intermediate nodes only
  if (contact && !terminal) { Ke = st.ee_contact_stiffness; eeContactReference(tTimes, contact, K, t, fRef, pEnv); }
#pragma unroll
  for (int i = 0; i < METRICS_TERMS; ++i) terms[i] = 0.0_r;
  real k1[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) k1[i] = 0.0_r;
  dyn = 0.0_r; eq = 0.0_r; ncOut = 0;
  real phi[12];
#pragma unroll 1
  for (int stage = 0; stage < (terminal ? 1 : 2); ++stage) {
    const DblIn in{x, u, stage ? dt : 0.0_r, k1};
    Feet<real> feet;
    real f[12];
    BaseMotion<real> bm;
    centroidalSweep<real>(
        md, st.gravity, in, [&](int cc, Vec3<real> r, Vec3<real> v) { feet.set(cc, r, v); },
        [&](Vec3<real> r, const Mat3<real>& R) {
          const real sdt = stage ? dt : 0.0_r;
          const Vec3<real> fe(-Ke * (x[6] + sdt * k1[6] + r.x - pEnv[0]), -Ke * (x[7] + sdt * k1[7] + r.y - pEnv[1]), -Ke * (x[8] + sdt * k1[8] + r.z - pEnv[2]));
          if (stage == 0) {
            if (Ke != 0.0_r) terms[6] = 0.5_r * st.ee_force_mu * ((fe.x - fRef[0]) * (fe.x - fRef[0]) + (fe.y - fRef[1]) * (fe.y - fRef[1]) + (fe.z - fRef[2]) * (fe.z - fRef[2]));
            real qee[4];
            matrixToQuaternion(R, qee);
            const Vec3<real> od = quaternionDistance(qee, eeQuatRef);
            const real muP = terminal ? st.ee_final_mu_position : st.ee_mu_position, muO = terminal ? st.ee_final_mu_orientation : st.ee_mu_orientation;
            const real hx = x[6] + r.x - eePosRef[0], hy = x[7] + r.y - eePosRef[1], hz = x[8] + r.z - eePosRef[2];
            terms[2] = 0.5_r * muP * (hx * hx + hy * hy + hz * hz) + 0.5_r * muO * (od.x * od.x + od.y * od.y + od.z * od.z);
          }
          return fe;
        },
        f, bm);
    if (stage == 0) {
      if (!terminal) {
        // the equality rows, foot by foot in contact_rows.h's order: a stance foot's three zero-velocity rows; a swing foot's three zero-force rows, then its normal-velocity row
        int row = 0;
        for (int cc = 0; cc < FEET; ++cc) {
          const Vec3<real> r = feet.r(cc);
          const Vec3<real> vf = bm.dp + cross(bm.omega, r) + feet.v(cc);
          if (contactOf(mode, cc)) {
            const real hz = vf.z + st.position_error_gain * (x[8] + r.z);
            eRow[row] = vf.x; eRow[row + 1] = vf.y; eRow[row + 2] = hz;
            eq += vf.x * vf.x + vf.y * vf.y + hz * hz;
            row += STANCE_ROWS;
          } else {
            real zp, zv;
            swingReference(st, sched, cc, t, phase, zp, zv);
            const real h = vf.z - zv + st.position_error_gain * (x[8] + r.z - zp);
            eRow[row] = u[3 * cc]; eRow[row + 1] = u[3 * cc + 1]; eRow[row + 2] = u[3 * cc + 2]; eRow[row + 3] = h;
            eq += u[3 * cc] * u[3 * cc] + u[3 * cc + 1] * u[3 * cc + 1] + u[3 * cc + 2] * u[3 * cc + 2] + h * h;
            row += SWING_ROWS;
          }
        }
        ncOut = row;   // = constraintCount(mode)
        for (int r = row; r < NCMAX; ++r) eRow[r] = 0.0_r;
      }
#pragma unroll
      for (int i = 0; i < 12; ++i) { k1[i] = f[i]; phi[i] = 0.5_r * dt * f[i]; }
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i) phi[i] += 0.5_r * dt * f[i];
    }
  }
  if (terminal) return;
  for (int i = 0; i < 12; ++i) { const real d = x[i] + phi[i] - xnext[i]; dRow[i] = d; dyn += d * d; }
  for (int j = 0; j < 18; ++j) { const real d = x[12 + j] + dt * u[12 + j] - xnext[12 + j]; dRow[12 + j] = d; dyn += d * d; }
  // tracking cost: the deviations once, in registers, then the two quadratic forms with the weights from LDS
  int tIdx; real tAlpha;
  timeSegment(tTimes, K, t, tIdx, tAlpha);
  const real fzNom = nominalNormalForce(md.total_mass, st.gravity, mode);
  real dx[30], du[30];
#pragma unroll
  for (int j = 0; j < 30; ++j) {
    dx[j] = x[j] - xReference(tStates, K, tIdx, tAlpha, j);
    du[j] = u[j] - nominalInputEntry(mode, j, fzNom);
  }
  real cq = 0.0_r, cr = 0.0_r;
#pragma unroll
  for (int i = 0; i < 30; ++i) {
    real qs = 0.0_r, rs = 0.0_r;
#pragma unroll
    for (int j = 0; j < 30; ++j) { qs += Qw[i * 30 + j] * dx[j]; rs += Rw[i * 30 + j] * du[j]; }
    cq += 0.5_r * dx[i] * qs; cr += 0.5_r * du[i] * rs;
    QM_SCHED_FENCE();   // one row of weights at a time: unfenced, the scheduler hoists all 1800 LDS reads in front of the first multiply-add and parks them in scratch (14 KB per lane)
  }
  terms[0] = cq; terms[1] = cr;
  const Barrier bp{st.joint_pos_barrier_mu, st.joint_pos_barrier_delta}, bv{st.joint_vel_barrier_mu, st.joint_vel_barrier_delta}, bf{st.friction_barrier_mu, st.friction_barrier_delta};
  real cp = 0.0_r, cv = 0.0_r, cf = 0.0_r;
  for (int i = 0; i < 6; ++i) {
    const real lo = md.q_lower[12 + i], up = md.q_upper[12 + i];
    // (bc: log(delta) of the three barriers and the constant value(-lower) + value(upper) of every limit, formed once by input_weight_kernel, layout.h)
    cp += bp.valueL(x[24 + i] - lo, bc[QM_BC_LOGD_POS]) + bp.valueL(up - x[24 + i], bc[QM_BC_LOGD_POS]) - bc[QM_BC_POS0 + i];
    cv += bv.valueL(u[24 + i] - st.arm_vel_lower[i], bc[QM_BC_LOGD_VEL]) + bv.valueL(st.arm_vel_upper[i] - u[24 + i], bc[QM_BC_LOGD_VEL]) - bc[QM_BC_VEL0 + i];
  }
  for (int cc = 0; cc < FEET; ++cc) if (contactOf(mode, cc)) {
    const real fx = u[3 * cc], fy = u[3 * cc + 1], fz = u[3 * cc + 2];
    cf += bf.valueL(st.friction_coefficient * fz - sqrt(fx * fx + fy * fy + st.friction_regularization), bc[QM_BC_LOGD_FRIC]);
  }
  terms[3] = cp; terms[4] = cv; terms[5] = cf;
}

__global__ void __launch_bounds__(METRICS_THREADS) metrics_kernel(MetricsArgs a) {
  QM_DYNAMIC_LDS(lds);
  QM_POISON_LDS(lds, METRICS_LDS_REALS);
  const int inst = blockIdx.x, tid = threadIdx.x, N = a.N;
  if (inst >= a.batch) return;
  constexpr int T = METRICS_THREADS;
  real* Qs = lds + ML_Q.off; real* Rs = lds + ML_R.off;
  real* XS = lds + ML_X.off; real* US = lds + ML_U.off; real* DS = lds + ML_D.off; real* ES = lds + ML_E.off; real* TS = lds + ML_T.off; real* red = lds + ML_RED.off;
  const ModelR& mdS = *reinterpret_cast<const ModelR*>(lds + ML_MODEL.off);
  const SettingsR& st = a.P->settings;
  const real* tg = a.tgrid + size_t(inst) * (N + 1);
  const Schedule sched{a.schedNum[inst], a.schedTimes + size_t(inst) * QMGPU_MAX_EVENTS, a.schedModes + size_t(inst) * (QMGPU_MAX_EVENTS + 1)};
  const real* tTimes = a.targetTimes + size_t(inst) * a.K;
  const real* tStates = a.targetStates + size_t(inst) * a.K * QMGPU_NTARGET;
  const real* contact = a.eeContact ? a.eeContact + size_t(inst) * a.K * 6 : nullptr;
  const real* X = a.X + size_t(inst) * (N + 1) * NX; const real* U = a.U + size_t(inst) * N * NU;

  // ---- the weights and the model constants into LDS, once
  for (int e = tid; e < NX * NX; e += T) { Qs[e] = st.Q[e]; Rs[e] = a.Rw[e]; }
  {
    const int* src = reinterpret_cast<const int*>(&a.P->model);
    int* dst = reinterpret_cast<int*>(lds + ML_MODEL.off);
    for (int e = tid; e < ML_MODEL.count; e += T) dst[e] = src[e];
  }
  real cs = 0.0_r, ds = 0.0_r, es = 0.0_r;
#pragma unroll 1
  for (int base = 0; base <= N; base += T) {
    const int nodes = N + 1 - base < T ? N + 1 - base : T;               // nodes of this pass: base .. base + nodes - 1
    const int inter = N - base < T ? N - base : T;                       // of them intermediate (k < N)
    const int xRows = N + 1 - base < T + 1 ? N + 1 - base : T + 1;       // their states and the one behind the last
    // ---- S1
    metricsLoadRows(XS, ML_XROW, X + size_t(base) * NX, xRows, NX, tid);
    metricsLoadRows(US, ML_XROW, U + size_t(base) * NU, inter, NU, tid);
    if (inter < nodes) for (int c = tid; c < NU; c += T) US[inter * ML_XROW + c] = 0.0_r;   // the terminal node has no input: its sweep runs on zeros
    __syncthreads();
    // ---- S2
    const int k = base + tid;
    if (k <= N) {
      const bool term = k == N;
      const real t = tg[k], dt = term ? 0.0_r : tg[k + 1] - t;
      const int phase = nodePhaseAt(sched, t);
      real terms[METRICS_TERMS];
      real d, e; int nc;
      QM_OPAQUE_LDS(const real, Qp, Qs);
      QM_OPAQUE_LDS(const real, Rp, Rs);
      metricsNode(mdS, st, Qp, Rp, a.Rw + QM_RW_DERIVED, sched, tTimes, tStates, contact, a.K, t, dt, phase, term, XS + tid * ML_XROW, US + tid * ML_XROW,
                  XS + (term ? tid : tid + 1) * ML_XROW, terms, DS + tid * ML_XROW, ES + tid * ML_EROW, nc, d, e);
      const real cost = ((((((terms[0] + terms[1]) + terms[2]) + terms[3]) + terms[4]) + terms[5]) + terms[6]);
#pragma unroll
      for (int i = 0; i < METRICS_TERMS; ++i) TS[tid * ML_TROW + i] = terms[i];
      if (a.nodeCost) a.nodeCost[size_t(inst) * (N + 1) + k] = cost;
      if (a.nc && !term) a.nc[size_t(inst) * N + k] = nc;
      cs += term ? cost : dt * cost; ds += dt * d; es += dt * e;
    }
    __syncthreads();
    // ---- S3
    if (a.costTerms) metricsStoreRows(a.costTerms + (size_t(inst) * (N + 1) + base) * METRICS_TERMS, TS, ML_TROW, nodes, METRICS_TERMS, tid);
    if (a.defect) metricsStoreRows(a.defect + (size_t(inst) * N + base) * NX, DS, ML_XROW, inter, NX, tid);
    if (a.eq) metricsStoreRows(a.eq + (size_t(inst) * N + base) * NCMAX, ES, ML_EROW, inter, NCMAX, tid);
    // (the next pass's S1 writes XS / US only, which no lane reads behind the barrier above; its S2 writes DS / ES / TS behind its own first barrier)
  }
  if (!a.performance) return;
  // ---- the sums: a fixed pairwise tree over the METRICS_THREADS partial sums of each row (threads beyond the last node hold exact zeros).  The pairing depends on the
  // thread count alone, so the order of summation depends on N only.  Row 3: the entries of upstream's initial-state constraint |x0 - X_0|^2 (not dt-scaled), one per lane
  real x0sq = 0.0_r;
  if (a.x0 && tid < NX) { const real d = a.x0[size_t(inst) * NX + tid] - X[tid]; x0sq = d * d; }
  red[tid] = cs; red[T + tid] = ds; red[2 * T + tid] = es; red[3 * T + tid] = x0sq;
  __syncthreads();
#pragma unroll 1
  for (int s = T / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int r = 0; r < METRICS_RED_ROWS; ++r) red[r * T + tid] += red[r * T + tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const real s0 = red[0], s1 = red[T] + red[3 * T], s2 = red[2 * T];
    real* p = a.performance + size_t(inst) * METRICS_PERF;
    p[0] = s0; p[1] = s0; p[2] = 0.0_r; p[3] = s1; p[4] = s2; p[5] = 0.0_r; p[6] = 0.0_r; p[7] = 0.0_r;
  }
}

}  // namespace qmk
