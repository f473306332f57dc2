// The launch chain of one MPC solve and the HBM scratch it runs in, in the kernels' arithmetic type (real.h).  Shared by the fp64
// path (qmgpu_api.hip) and the fp32 path (qmgpu_mpc32.hip, where the caller's fp64 arrays are converted on the way in and out).
//     mpc_init -> ad_node (3 nodes per wavefront) -> lq_node (1 node per wavefront) -> riccati (1 instance per workgroup) -> linesearch
// repeated sqp.sqpIteration times on one stream, no host synchronisation in between.  Both paths build the call's MpcIo with makeMpcIo and
// enqueue it with enqueueMpcSolve; failures leave as the exceptions of host/host_error.h.
#pragma once
#include <vector>

#include "../host/host_error.h"
#include "aux_kernels.h"
#include "ddp_kernel.h"
#include "gpu_rt.h"
#include "layout.h"
#include "linesearch_kernel.h"
#include "lq_kernel.h"
#include "riccati_kernel.h"

namespace qmk {

struct MpcBuffers {
  ProblemR* dP = nullptr;
  real *dRw = nullptr, *dZeros = nullptr;
  real *dTgrid = nullptr, *dDtgrid = nullptr, *dX = nullptr, *dU = nullptr, *dStages = nullptr, *dAdRows = nullptr, *dMetrics = nullptr, *dGains = nullptr, *ddX = nullptr, *ddU = nullptr;
  real *dXt = nullptr, *dUt = nullptr, *dInstStats = nullptr, *dDebug = nullptr;
  int *dStageNc = nullptr, *dNodeMode = nullptr, *dNodePhase = nullptr, *dDone = nullptr;
  real *dDdpX = nullptr, *dDdpU = nullptr, *dDdpMerit = nullptr;   // DDP variant: trial trajectories / merits, allocated on first use
  int cus = 256;                                                   // compute units of the device the buffers live on (allocateMpcBuffers): launch shapes that depend on batch > CUs
  size_t maxBatch = 0, maxNodes = 0;                               // capacity the buffers were allocated for (allocateMpcBuffers)
};

// the arguments of one call (qmgpu_mpc_args) as `real` device arrays
struct MpcIo {
  int batch, N, K, lineSearch;
  double dtD;                                           // settings.dt in fp64
  const double *t0D, *timeGridD, *schedTimesD;          // the caller's fp64 times (mpc_init_kernel forms the grid and the node phases from them)
  const real *x0, *targetTimes, *targetStates;
  const int* schedNum; const real* schedTimes; const int* schedModes;
  const real *warmX, *warmU;
  real *outT, *outX, *outU; int* outMode; real* outStats;
  const real* eeContact;                                // [batch][K][6] or null (force tracking)
  int algorithm;                                        // QMGPU_ALG_SQP / QMGPU_ALG_DDP
};

// Alloc: callable (size_t count, size_t elemSize, bool scratch) -> void*
template <class Alloc> inline void allocateMpcBuffers(MpcBuffers& m, size_t B, size_t N, Alloc&& alloc) {
  const size_t N1 = N + 1;
  m.maxBatch = B; m.maxNodes = N;
  auto R = [&](size_t n, bool scratch = true) { return static_cast<real*>(alloc(n, sizeof(real), scratch)); };
  auto I = [&](size_t n) { return static_cast<int*>(alloc(n, sizeof(int), true)); };
  m.dP = static_cast<ProblemR*>(alloc(1, sizeof(ProblemR), false));
  m.dRw = R(QM_RW_DOUBLES, false);
  m.dZeros = R(64, false);
  m.dTgrid = R(B * N1);
  m.dDtgrid = R(B * N1);
  m.dNodePhase = I(B * N1);
  m.dX = R(B * N1 * 30);
  m.dU = R(B * N * 30);
  m.dStages = R(B * N1 * STAGE_DOUBLES);
  m.dAdRows = R(B * N1 * AD_DOUBLES);
  m.dMetrics = R(B * N1 * NODE_METRICS);
  m.dGains = R(B * N * GAIN_DOUBLES);
  m.ddX = R(B * N1 * 30);
  m.ddU = R(B * N * 30);
  m.dXt = R(2 * B * N1 * 30);   // two trial steps are evaluated side by side (linesearch_kernel)
  m.dUt = R(2 * B * N * 30);
  m.dInstStats = R(B * 4);
  m.dStageNc = I(B * N1);
  m.dNodeMode = I(B * N1);
  m.dDone = I(B);
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) m.cus = cus;
}

template <class Alloc> inline void ensureDdpBuffers(MpcBuffers& m, Alloc&& alloc) {
  if (m.dDdpX) return;
  const size_t B = m.maxBatch, N = m.maxNodes;
  m.dDdpX = static_cast<real*>(alloc(size_t(DDP_MAX_TRIALS) * B * (N + 1) * 30, sizeof(real), true));
  m.dDdpU = static_cast<real*>(alloc(size_t(DDP_MAX_TRIALS) * B * N * 30, sizeof(real), true));
  m.dDdpMerit = static_cast<real*>(alloc(size_t(DDP_MAX_TRIALS) * B * 2, sizeof(real), true));
}

inline hipError_t prepareMpcKernels() {
  const hipError_t e = QM_ALLOW_DYNAMIC_LDS(riccati_kernel<RICCATI_WAVES>, RICCATI_LDS_BYTES);
  return e != hipSuccess ? e : QM_ALLOW_DYNAMIC_LDS(linesearch_kernel, QM_CU_LDS_BYTES - LS_STATIC_LDS_BYTES);
}

// Where the fp32 build stages the fp64 arrays of a call (one array per converted argument); the fp64 build passes the caller's arrays on and has none.
struct MpcStaging {
  real *x0 = nullptr, *targetTimes = nullptr, *targetStates = nullptr, *schedTimes = nullptr, *warmX = nullptr, *warmU = nullptr, *eeContact = nullptr;
};

// The MpcIo of one call.  in(caller's fp64 array, its staging array, element count) -> the array as `const real*`: the identity in the fp64 build, the
// narrowing copy into the staging array in the fp32 build (null stays null).  out*: where the chain writes its results.
template <class In> inline MpcIo makeMpcIo(const qmgpu_mpc_args& a, double dt, const MpcStaging& st, In&& in, real* outT, real* outX, real* outU, real* outStats) {
  const size_t B = size_t(a.batch), N = size_t(a.num_nodes), N1 = N + 1, K = size_t(a.num_target_knots);
  MpcIo io{};
  io.batch = a.batch; io.N = a.num_nodes; io.K = a.num_target_knots; io.lineSearch = a.line_search;
  io.dtD = dt; io.t0D = a.t0; io.timeGridD = a.time_grid; io.schedTimesD = a.sched_event_times;
  io.x0 = in(a.x0, st.x0, B * 30);
  io.targetTimes = in(a.target_times, st.targetTimes, B * K);
  io.targetStates = in(a.target_states, st.targetStates, B * K * QMGPU_NTARGET);
  io.schedNum = a.sched_num_events;
  io.schedTimes = in(a.sched_event_times, st.schedTimes, B * QMGPU_MAX_EVENTS);   // fp32: the 1e300 padding becomes +inf, still "never"
  io.schedModes = a.sched_modes;
  io.warmX = in(a.warm_x, st.warmX, B * N1 * 30);
  io.warmU = in(a.warm_u, st.warmU, B * N * 30);
  io.eeContact = in(a.ee_contact_ref, st.eeContact, B * K * 6);
  io.outT = outT; io.outX = outX; io.outU = outU; io.outMode = a.out_mode; io.outStats = outStats;
  io.algorithm = a.algorithm;
  return io;
}

// The HIP events of one timed call, in the order they are recorded: the chain below records the first five, qmgpu_api.hip the two around the WBC and reads
// them all back (readTiming).  A handle keeps TIMING_EVENTS events per call.
enum TimingEvent { EV_START, EV_AD_NODE, EV_LQ_NODE, EV_RICCATI, EV_LINE_SEARCH, EV_WBC_START, EV_WBC_END, TIMING_EVENTS = EV_WBC_END + 1 };
inline void recordTiming(hipEvent_t* ev, TimingEvent which, hipStream_t s) { if (ev) (void)hipEventRecord(ev[which], s); }

// The part both solvers share: linearisation along (dX, dU) -> projected stage records -> Riccati sweep.  debug: the per-node LQ dump or null.
inline void enqueueLqRiccati(hipStream_t s, const MpcBuffers& m, const MpcIo& io, real* debug, hipEvent_t* ev) {
  const int B = io.batch, N = io.N;
  LqArgs la{m.dP, m.dRw, B, N, io.K, m.dTgrid, m.dDtgrid, m.dNodePhase, m.dX, m.dU, io.targetTimes, io.targetStates, io.schedNum, io.schedTimes,
            io.schedModes, m.dZeros, m.dStages, m.dStageNc, m.dNodeMode, m.dMetrics, debug, m.dAdRows, m.dDone, io.eeContact};
  QM_LAUNCH(ad_node_kernel, adGridFor(B * (N + 1)), 64, s, la);
  recordTiming(ev, EV_AD_NODE, s);
  QM_LAUNCH(lq_node_kernel, B * (N + 1), 64, s, la);
  recordTiming(ev, EV_LQ_NODE, s);
  RiccatiArgs ra{B, N, m.dStages, m.dStageNc, m.dDtgrid, io.x0, m.dX, m.dGains, m.ddX, m.ddU, m.dInstStats, m.dDone};
  QM_LAUNCH_DYN(riccati_kernel<RICCATI_WAVES>, B, RICCATI_WAVES * 64, RICCATI_LDS_BYTES, s, ra);
  recordTiming(ev, EV_RICCATI, s);
}

// ev: the call's timing events or null
inline void enqueueMpcKernels(hipStream_t s, const MpcBuffers& m, const MpcIo& io, int iterations, bool debugLq, hipEvent_t* ev) {
  const int B = io.batch, N = io.N;
  recordTiming(ev, EV_START, s);
  // sqp.sqpIteration iterations (task.info:77; 1 in the reference's configuration): later iterations warm-start from the iterate the
  // line search just wrote to the output buffers.  After every iteration the line-search kernel applies upstream's convergence
  // test per instance; the kernels of the following iterations return at once for the instances that have converged.
  for (int it = 0; it < iterations; ++it) {
    InitArgs ia{m.dP, B, N, io.dtD, io.t0D, io.timeGridD, io.schedTimesD, io.x0, it == 0 ? io.warmX : io.outX, it == 0 ? io.warmU : io.outU, io.schedNum, io.schedModes,
                m.dTgrid, m.dDtgrid, m.dNodePhase, m.dX, m.dU, it, m.dDone};
    QM_LAUNCH(mpc_init_kernel, B, 128, s, ia);
    enqueueLqRiccati(s, m, io, debugLq ? m.dDebug : nullptr, ev);
    const LsLaunch shape = lsLaunch(B, N, m.cus);
    LsArgs ls{m.dP, m.dRw, B, N, io.K, io.lineSearch, io.eeContact, m.dTgrid, m.dDtgrid, m.dNodePhase, m.dX, m.dU, m.ddX, m.ddU, io.targetTimes, io.targetStates, io.schedNum,
              io.schedTimes, io.schedModes, m.dMetrics, m.dInstStats, m.dNodeMode, m.dXt, m.dUt, io.outT, io.outX, io.outU, io.outMode, io.outStats, it, shape.trialInLds, m.dDone};
    QM_LAUNCH_DYN(linesearch_kernel, B, shape.threads, shape.dynamicLdsBytes, s, ls);
    recordTiming(ev, EV_LINE_SEARCH, s);
  }
}

// One DDP iteration (ddp_kernel.h): rollout -> LQ approximation along it -> Riccati -> policy rollouts for every step length -> selection.
// `trials` = number of step lengths maxStep * 2^-i >= minStep (host side, <= DDP_MAX_TRIALS).
inline void enqueueDdpKernels(hipStream_t s, const MpcBuffers& m, const MpcIo& io, int trials, hipEvent_t* ev) {
  const int B = io.batch, N = io.N;
  recordTiming(ev, EV_START, s);
  InitArgs ia{m.dP, B, N, io.dtD, io.t0D, io.timeGridD, io.schedTimesD, io.x0, io.warmX, io.warmU, io.schedNum, io.schedModes, m.dTgrid, m.dDtgrid, m.dNodePhase, m.dX, m.dU, 0, m.dDone};
  QM_LAUNCH(mpc_init_kernel, B, 128, s, ia);
  DdpArgs ra{m.dP, m.dRw, B, N, io.K, 0, io.eeContact, m.dTgrid, m.dDtgrid, m.dNodePhase, io.x0, m.dX, m.dU, io.targetTimes, io.targetStates, io.schedNum, io.schedTimes, io.schedModes,
             m.dStages, m.dStageNc, m.dGains, m.dX, m.dU, m.dDdpMerit};
  if (!io.warmX) QM_LAUNCH(ddp_rollout_kernel, (B + 63) / 64, 64, s, ra);   // no warm states: the nominal trajectory is the open-loop rollout of the inputs
  enqueueLqRiccati(s, m, io, nullptr, ev);
  ra.trials = trials; ra.Xout = m.dDdpX; ra.Uout = m.dDdpU;
  QM_LAUNCH(ddp_rollout_kernel, (B * trials + 63) / 64, 64, s, ra);
  DdpSelectArgs sa{m.dP, B, N, trials, m.dTgrid, m.dNodeMode, m.dX, m.dU, m.dMetrics, m.dInstStats, m.dDdpX, m.dDdpU, m.dDdpMerit, io.outT, io.outX, io.outU, io.outMode, io.outStats, m.dDone};
  QM_LAUNCH(ddp_select_kernel, B, 256, s, sa);
  recordTiming(ev, EV_LINE_SEARCH, s);
}

inline int ddpTrialCount(double minStep, double maxStep) {
  int n = 0;
  for (double a = maxStep; a >= minStep && n < DDP_MAX_TRIALS; a *= 0.5) ++n;
  return n > 0 ? n : 1;
}

// One solve with the solver io.algorithm names, on stream s.  alloc: as allocateMpcBuffers (the DDP buffers are allocated by the first DDP solve).
template <class Alloc> inline void enqueueMpcSolve(hipStream_t s, MpcBuffers& m, const MpcIo& io, const qmgpu_settings& settings, bool debugLq, hipEvent_t* ev, Alloc&& alloc) {
  if (io.algorithm != QMGPU_ALG_SQP && io.algorithm != QMGPU_ALG_DDP) throw std::invalid_argument("unknown qmgpu_mpc_args::algorithm");
  if (io.algorithm == QMGPU_ALG_DDP) {
    ensureDdpBuffers(m, alloc);
    enqueueDdpKernels(s, m, io, ddpTrialCount(settings.ddp_min_step, settings.ddp_max_step), ev);
  } else {
    enqueueMpcKernels(s, m, io, settings.sqp_iterations > 1 ? settings.sqp_iterations : 1, debugLq, ev);
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace qmk
