// taskspace_kernel -- the planned trajectory in task space: per node the four foot positions, the end-effector pose and the centre of mass; per intermediate node the
// foot velocities, the base twist and the centre of pressure; per mode-schedule event the footholds of the feet that land there.  Stateless: it reads the model behind
// the handle and the caller's arrays, nothing a solve leaves.
//
// Replaces the host-side kinematics of upstream's QmVisualizer: publishOptimizedStateTrajectory (qm_interface/src/visualization/qm_visualization.cpp:90-189: forward
// kinematics on every state of the plan for the feet, CoM and EE lines, and on the state interpolated at every event inside the horizon where a foot lands for the
// "future footholds", :158-181) and what publishObservation / publishCartesianMarkers (:267-317) draw of one state and input.  Every quantity is an output of the tree
// sweep the solve runs anyway (sweep_dev.h: onFoot, onEE, BaseMotion); nothing is derived a second time.
//
// The shape of metrics_kernel: one workgroup per instance, ONE SHOOTING NODE PER LANE (value-only evaluation, T = real instantiation of the tree sweep, DblIn with a
// zero step), lanes striding over the horizon in passes of TASKSPACE_THREADS nodes.  Per pass
//   S1  the states and inputs of the pass's nodes land in LDS as flat, coalesced copies (a lane reading its own node's rows from HBM touches 60 places 240 bytes apart)
//   S2  every lane sweeps its node and leaves its seven output rows in LDS; the terminal node, and every node without U, evaluates the positions only
//   S3  the row arrays leave as flat copies: consecutive threads, consecutive addresses
// and then the footholds
//   F1  per event inside the horizon where a foot lands (wave-uniform; the wavefronts take the events in turn): index and weight of timeSegment on the time grid by
//       ballots, as policy_eval_kernel; lanes 0..29 interpolate the state into row e of TL_X, lanes 30..59 clear row e of TL_U
//   F2  lane e sweeps event e's state with zero input, keeps the landing feet of its row and writes the event's four flags
//   F3  the foothold rows leave as one flat copy
#pragma once
#include "gpu_rt.h"
#include "layout.h"
#include "contact_rows.h"
#include "schedule_dev.h"
#include "sweep_dev.h"
#include "linesearch_kernel.h"   // DblIn
#include "taskspace_lds.h"

namespace qmk {

struct TaskspaceArgs {
  const ProblemR* P;
  int batch, N;
  const real* tgrid;       // [batch][N+1]
  const real* X;           // [batch][N+1][30]
  const real* U;           // [batch][N][30] or null: positions only
  const int* schedNum; const real* schedTimes; const int* schedModes;   // read for the footholds only
  // outputs, each may be null
  real* feetPos;           // [batch][N+1][4][3]
  real* eePos;             // [batch][N+1][3]
  real* eeQuat;            // [batch][N+1][4]
  real* com;               // [batch][N+1][3]
  real* feetVel;           // [batch][N][4][3]
  real* baseTwist;         // [batch][N][6]
  real* cop;               // [batch][N][3]
  real* footholdPos;       // [batch][QMGPU_MAX_EVENTS][4][3]
  int* footholdFlag;       // [batch][QMGPU_MAX_EVENTS][4]
};

// rows [first, first + rows) of a [.][width] HBM array <-> LDS rows of `stride` reals, flat: thread t takes elements t, t + THREADS, ...
__device__ __forceinline__ void taskspaceLoadRows(real* ldsRows, int stride, const real* src, int rows, int width, int tid) {
  for (int e = tid; e < rows * width; e += TASKSPACE_THREADS) { const int r = e / width, c = e - r * width; ldsRows[r * stride + c] = src[e]; }
}
__device__ __forceinline__ void taskspaceStoreRows(real* dst, const real* ldsRows, int stride, int rows, int width, int tid) {
  for (int e = tid; e < rows * width; e += TASKSPACE_THREADS) { const int r = e / width, c = e - r * width; dst[e] = ldsRows[r * stride + c]; }
}

// The task-space quantities of one point (x, u), all in world axes: fp [4][3] = base position + r_c, ee = base position + r_ee, qe = matrixToQuaternion(R_ee) as the
// end-effector cost forms it, cm = base position + BaseMotion::com; with `velocities` also fv [4][3] = dp + omega x r_c + v_c (the value a stance foot contributes to
// the equality rows, metricsNode's vf), tw = [dp ; omega] and cp, the centre of pressure of the four normal forces (zero unless their sum, added left to right, is
// positive).  x, u and the seven rows: LDS.  u is read for the joint rates and the normal forces only.
// INLINED at its two call sites (a node, a foothold), unlike metricsNode and nodePerformance.  Their reasons do not hold here: the body is one value-only sweep, without
// the 1800 weight reads that took metricsNode to 14 KB of scratch when inlined, and the kernel is compiled in fp64 only, 5 k instructions, not the 35 k-instruction fp32
// line search that was miscompiled.  Measured on the gfx950 cross-compile: inlined 256 + 50 registers, 168 B of scratch per lane (the foot table
// the sweep's leg loop fills by a runtime index; no register spilled), 29.6 KB of code; as a called function 256 + 32 registers and 600 B of scratch, the callee-saved
// registers the call saves and restores with the interprocedural register allocation off (261 scratch instructions in the callee against 78), 24.3 KB of code.
__device__ __forceinline__ void taskspacePoint(const ModelR& md, real gravity, const real* x, const real* u, bool velocities, real* fp, real* ee, real* qe, real* cm,
                                                         real* fv, real* tw, real* cp) {
  const real k1[12] = {0.0_r, 0.0_r, 0.0_r, 0.0_r, 0.0_r, 0.0_r, 0.0_r, 0.0_r, 0.0_r, 0.0_r, 0.0_r, 0.0_r};
  const DblIn in{x, u, 0.0_r, k1};
  Feet<real> feet;
  Vec3<real> rEE;
  Mat3<real> REE;
  real f[12];
  BaseMotion<real> bm;
  centroidalSweep<real>(
      md, gravity, in, [&](int cc, Vec3<real> r, Vec3<real> v) { feet.set(cc, r, v); },
      [&](Vec3<real> r, const Mat3<real>& R) { rEE = r; REE = R; return Vec3<real>(0.0_r, 0.0_r, 0.0_r); }, f, bm);
  const real px = x[6], py = x[7], pz = x[8];
  Vec3<real> p[FEET];
#pragma unroll
  for (int cc = 0; cc < FEET; ++cc) {
    const Vec3<real> r = feet.r(cc);
    p[cc] = Vec3<real>(px + r.x, py + r.y, pz + r.z);
    fp[3 * cc] = p[cc].x; fp[3 * cc + 1] = p[cc].y; fp[3 * cc + 2] = p[cc].z;
  }
  ee[0] = px + rEE.x; ee[1] = py + rEE.y; ee[2] = pz + rEE.z;
  real q[4];
  matrixToQuaternion(REE, q);
  qe[0] = q[0]; qe[1] = q[1]; qe[2] = q[2]; qe[3] = q[3];
  cm[0] = px + bm.com.x; cm[1] = py + bm.com.y; cm[2] = pz + bm.com.z;
  if (!velocities) return;
#pragma unroll
  for (int cc = 0; cc < FEET; ++cc) {
    const Vec3<real> vf = bm.dp + cross(bm.omega, feet.r(cc)) + feet.v(cc);
    fv[3 * cc] = vf.x; fv[3 * cc + 1] = vf.y; fv[3 * cc + 2] = vf.z;
  }
  tw[0] = bm.dp.x; tw[1] = bm.dp.y; tw[2] = bm.dp.z; tw[3] = bm.omega.x; tw[4] = bm.omega.y; tw[5] = bm.omega.z;
  const real fz0 = u[2], fz1 = u[5], fz2 = u[8], fz3 = u[11];
  const real s = ((fz0 + fz1) + fz2) + fz3;   // this order is the contract (qmgpu.h): a reference takes the same branch on the same bits
  if (s > 0.0_r) {
    cp[0] = (((fz0 * p[0].x + fz1 * p[1].x) + fz2 * p[2].x) + fz3 * p[3].x) / s;
    cp[1] = (((fz0 * p[0].y + fz1 * p[1].y) + fz2 * p[2].y) + fz3 * p[3].y) / s;
    cp[2] = (((fz0 * p[0].z + fz1 * p[1].z) + fz2 * p[2].z) + fz3 * p[3].z) / s;
  } else {
    cp[0] = 0.0_r; cp[1] = 0.0_r; cp[2] = 0.0_r;
  }
}

// the feet that land at event e, bit c for foot c (contact order): the event lies strictly inside (t0, tN), foot c is off the ground in the mode before it and on the
// ground in the mode after it (qm_visualization.cpp:163-175).  Zero for e >= numEvents.  Wave-uniform for a wave-uniform e.
__device__ __forceinline__ int landingFeet(const Schedule& s, int e, real t0, real tN) {
  if (e >= s.numEvents) return 0;
  const real t = s.eventTimes[e];
  if (!(t0 < t && t < tN)) return 0;
  const int before = s.modes[e], after = s.modes[e + 1];
  int m = 0;
  for (int cc = 0; cc < FEET; ++cc) if (!contactOf(before, cc) && contactOf(after, cc)) m |= 1 << cc;
  return m;
}

__global__ void __launch_bounds__(TASKSPACE_THREADS) taskspace_kernel(TaskspaceArgs a) {
  QM_DYNAMIC_LDS(lds);
  QM_POISON_LDS(lds, TASKSPACE_LDS_REALS);
  const int inst = blockIdx.x, tid = threadIdx.x, N = a.N;
  if (inst >= a.batch) return;
  constexpr int T = TASKSPACE_THREADS;
  real* XS = lds + TL_X.off; real* US = lds + TL_U.off;
  real* FP = lds + TL_FP.off; real* EE = lds + TL_EE.off; real* QE = lds + TL_Q.off; real* CM = lds + TL_COM.off;
  real* FV = lds + TL_FV.off; real* TW = lds + TL_TW.off; real* CP = lds + TL_COP.off; real* FH = lds + TL_FH.off;
  const ModelR& mdS = *reinterpret_cast<const ModelR*>(lds + TL_MODEL.off);
  const real gravity = a.P->settings.gravity;
  const real* tg = a.tgrid + size_t(inst) * (N + 1);
  const real* X = a.X + size_t(inst) * (N + 1) * NX;
  const real* U = a.U ? a.U + size_t(inst) * N * NU : nullptr;

  // ---- the model constants into LDS, once
  {
    const int* src = reinterpret_cast<const int*>(&a.P->model);
    int* dst = reinterpret_cast<int*>(lds + TL_MODEL.off);
    for (int e = tid; e < TL_MODEL.count; e += T) dst[e] = src[e];
  }
#pragma unroll 1
  for (int base = 0; base <= N; base += T) {
    const int nodes = N + 1 - base < T ? N + 1 - base : T;               // nodes of this pass: base .. base + nodes - 1
    const int inter = N - base < T ? N - base : T;                       // of them intermediate (k < N)
    const int withU = U ? inter : 0;                                     // of them with an input
    // ---- S1
    taskspaceLoadRows(XS, TL_XROW, X + size_t(base) * NX, nodes, NX, tid);
    if (U) taskspaceLoadRows(US, TL_XROW, U + size_t(base) * NU, inter, NU, tid);
    for (int e = tid; e < (nodes - withU) * NU; e += T) { const int r = e / NU, c = e - r * NU; US[(withU + r) * TL_XROW + c] = 0.0_r; }   // no input: the sweep runs on zeros
    __syncthreads();
    // ---- S2
    const int k = base + tid;
    if (k <= N)
      taskspacePoint(mdS, gravity, XS + tid * TL_XROW, US + tid * TL_XROW, U && k < N, FP + tid * TL_FROW, EE + tid * TL_VROW, QE + tid * TL_QROW, CM + tid * TL_VROW,
                     FV + tid * TL_FROW, TW + tid * TL_TWROW, CP + tid * TL_VROW);
    __syncthreads();
    // ---- S3
    const size_t node0 = size_t(inst) * (N + 1) + base, step0 = size_t(inst) * N + base;
    if (a.feetPos) taskspaceStoreRows(a.feetPos + node0 * TASKSPACE_FEET_W, FP, TL_FROW, nodes, TASKSPACE_FEET_W, tid);
    if (a.eePos) taskspaceStoreRows(a.eePos + node0 * TASKSPACE_VEC_W, EE, TL_VROW, nodes, TASKSPACE_VEC_W, tid);
    if (a.eeQuat) taskspaceStoreRows(a.eeQuat + node0 * TASKSPACE_QUAT_W, QE, TL_QROW, nodes, TASKSPACE_QUAT_W, tid);
    if (a.com) taskspaceStoreRows(a.com + node0 * TASKSPACE_VEC_W, CM, TL_VROW, nodes, TASKSPACE_VEC_W, tid);
    if (a.feetVel) taskspaceStoreRows(a.feetVel + step0 * TASKSPACE_FEET_W, FV, TL_FROW, withU, TASKSPACE_FEET_W, tid);
    if (a.baseTwist) taskspaceStoreRows(a.baseTwist + step0 * TASKSPACE_TWIST_W, TW, TL_TWROW, withU, TASKSPACE_TWIST_W, tid);
    if (a.cop) taskspaceStoreRows(a.cop + step0 * TASKSPACE_VEC_W, CP, TL_VROW, withU, TASKSPACE_VEC_W, tid);
    // (the next pass's S1, and F1, write XS / US only, which no lane reads behind the barrier above; the next S2, and F2, write output rows behind a barrier of their own)
  }
  if (!a.footholdPos && !a.footholdFlag) return;
  // ---- the footholds
  const Schedule sched{a.schedNum[inst], a.schedTimes + size_t(inst) * QMGPU_MAX_EVENTS, a.schedModes + size_t(inst) * (QMGPU_MAX_EVENTS + 1)};
  const real t0 = tg[0], tN = tg[N];
  // ---- F1
  const int wave = tid / 64, lane = tid & 63;
#pragma unroll 1
  for (int e = wave; e < QMGPU_MAX_EVENTS; e += T / 64) {
    if (!landingFeet(sched, e, t0, tN)) continue;   // wave-uniform
    int idx; real alpha;
    timeSegmentWave(tg, N + 1, sched.eventTimes[e], lane, idx, alpha);   // t0 < t_e < tN: idx + 1 <= N
    if (lane < NX) {
      const real* xl = X + size_t(idx) * NX;
      XS[e * TL_XROW + lane] = alpha * xl[lane] + (1.0_r - alpha) * xl[NX + lane];
    } else if (lane < 2 * NX) {
      US[e * TL_XROW + lane - NX] = 0.0_r;
    }
  }
  __syncthreads();
  // ---- F2
  if (tid < QMGPU_MAX_EVENTS) {
    const int land = landingFeet(sched, tid, t0, tN);
    real* row = FH + tid * TL_FROW;
    // (the six rows a foothold does not need go to this lane's own output rows, which nothing reads any more)
    if (land)
      taskspacePoint(mdS, gravity, XS + tid * TL_XROW, US + tid * TL_XROW, false, row, EE + tid * TL_VROW, QE + tid * TL_QROW, CM + tid * TL_VROW, FV + tid * TL_FROW,
                     TW + tid * TL_TWROW, CP + tid * TL_VROW);
#pragma unroll
    for (int cc = 0; cc < FEET; ++cc) {
      const bool lands = (land >> cc) & 1;
      if (!lands) { row[3 * cc] = 0.0_r; row[3 * cc + 1] = 0.0_r; row[3 * cc + 2] = 0.0_r; }
      if (a.footholdFlag) a.footholdFlag[(size_t(inst) * QMGPU_MAX_EVENTS + tid) * FEET + cc] = lands ? 1 : 0;
    }
  }
  __syncthreads();
  // ---- F3
  if (a.footholdPos) taskspaceStoreRows(a.footholdPos + size_t(inst) * QMGPU_MAX_EVENTS * TASKSPACE_FEET_W, FH, TL_FROW, QMGPU_MAX_EVENTS, TASKSPACE_FEET_W, tid);
}

}  // namespace qmk
