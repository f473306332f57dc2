// fp32 build of the MPC kernels (BASELINE.json configs[4]: "fp32 vs fp64 tolerance sweep").  This translation unit is compiled with
//     -DQM_REAL=float -Dqmk=qmk32
// so that the SAME kernel sources as the fp64 path (kernels/*.h, written in terms of `real`) are instantiated a second time in
// namespace qmk32 with v_mfma_f32_16x16x4_f32, fp32 LDS / HBM scratch (half the bytes) and fp32 vector arithmetic.  The boundary of
// the library stays fp64 (the reference's ocs2::scalar_t): the caller's arrays are converted on the device on the way in and out.
// The WBC is not part of this build: its interior point works at complementarity / pivot tolerances of 1e-9 .. 1e-13 that have no
// fp32 counterpart, and it always runs in fp64 on the (converted) policy of either MPC path.
#include "mpc32.h"

#include <memory>

#include "kernels/mpc_pipeline.h"

static_assert(sizeof(qmk::real) == 4, "compile this file with -DQM_REAL=float -Dqmk=qmk32");

namespace qmk {   // = qmk32 in this translation unit

constexpr int kMaxKnots32 = QMGPU_F32_MAX_TARGET_KNOTS;   // include/qmgpu.h; checked by checkMpcArgs (QMGPU_ERR_CAPACITY) before this translation unit is reached

__global__ void __launch_bounds__(256) narrow_kernel(const double* src, float* dst, size_t n) {
  for (size_t i = size_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += size_t(gridDim.x) * 256) dst[i] = float(src[i]);
}
__global__ void __launch_bounds__(256) widen_kernel(const float* src, double* dst, size_t n) {
  for (size_t i = size_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += size_t(gridDim.x) * 256) dst[i] = double(src[i]);
}

struct Mpc32 {
  MpcBuffers m;
  MpcStaging in;   // fp32 staging of one call's arguments
  float *outT = nullptr, *outX = nullptr, *outU = nullptr, *outStats = nullptr;
};

void updateProblem(Mpc32* p, const qmgpu_problem& problem, hipStream_t stream) {
  ProblemR host;
  convert(problem, host);
  HIP_CHECK(hipStreamSynchronize(stream));
  HIP_CHECK(hipMemcpy(p->m.dP, &host, sizeof(ProblemR), hipMemcpyHostToDevice));
  QM_LAUNCH(input_weight_kernel, 1, 64, stream, p->m.dP, p->m.dZeros, p->m.dRw);
  HIP_CHECK(hipGetLastError());
}

Mpc32* create(const qmgpu_problem& problem, int maxBatch, int maxNodes, hipStream_t stream, const RawAlloc& alloc) {
  auto p = std::make_unique<Mpc32>();
  const size_t B = size_t(maxBatch), N = size_t(maxNodes), N1 = N + 1;
  allocateMpcBuffers(p->m, B, N, alloc);
  auto F = [&](size_t n) { return static_cast<float*>(alloc(n, sizeof(float), true)); };
  p->in.x0 = F(B * 30); p->in.targetTimes = F(B * kMaxKnots32); p->in.targetStates = F(B * kMaxKnots32 * QMGPU_NTARGET); p->in.schedTimes = F(B * QMGPU_MAX_EVENTS);
  p->in.warmX = F(B * N1 * 30); p->in.warmU = F(B * N * 30);
  p->outT = F(B * N1); p->outX = F(B * N1 * 30); p->outU = F(B * N * 30); p->outStats = F(B * QMGPU_NSTATS); p->in.eeContact = F(B * kMaxKnots32 * 6);
  HIP_CHECK(hipMemsetAsync(p->m.dZeros, 0, 64 * sizeof(float), stream));
  HIP_CHECK(prepareMpcKernels());
  updateProblem(p.get(), problem, stream);
  HIP_CHECK(hipStreamSynchronize(stream));
  return p.release();
}

void destroy(Mpc32* p) { delete p; }

void enqueue(Mpc32* p, hipStream_t s, const qmgpu_mpc_args* a, const qmgpu_settings& settings, hipEvent_t* ev, const RawAlloc& alloc) {
  if (a->num_target_knots > kMaxKnots32) throw qmhost::CapacityError("more target knots than the fp32 staging holds");
  const size_t B = size_t(a->batch), N = size_t(a->num_nodes), N1 = N + 1;
  auto narrow = [&](const double* src, float* dst, size_t n) {
    if (!src) return static_cast<const float*>(nullptr);
    QM_LAUNCH(narrow_kernel, unsigned((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024), 256, s, src, dst, n);
    return static_cast<const float*>(dst);
  };
  const MpcIo io = makeMpcIo(*a, settings.dt, p->in, narrow, p->outT, p->outX, p->outU, a->out_stats ? p->outStats : nullptr);
  enqueueMpcSolve(s, p->m, io, settings, false, ev, alloc);
  auto widen = [&](const float* src, double* dst, size_t n) { QM_LAUNCH(widen_kernel, unsigned((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024), 256, s, src, dst, n); };
  widen(p->outT, a->out_t, B * N1);
  widen(p->outX, a->out_x, B * N1 * 30);
  widen(p->outU, a->out_u, B * N * 30);
  if (a->out_stats) widen(p->outStats, a->out_stats, B * QMGPU_NSTATS);
  HIP_CHECK(hipGetLastError());
}

}  // namespace qmk
