// wbc_report_kernel -- the WBC solution report: task residuals, limit margins and the commanded torque of ANY decision vector x = [accelerations (24), contact
// forces (12)] under the tasks of one tick of the whole-body controller.  One wavefront per robot instance, every array in (dynamic) LDS.  Stateless: nothing is read
// out of wbc_kernel; the tick's model terms and stacked tasks are rebuilt from the inputs of the tick (include/qmgpu.h: qmgpu_wbc_report_batch).
//
// The model update and the task rows are wbc_kernel.h's device functions, called as they are:
//   R1  wbcLoadInputs, wbcCoordinates                      (S1, S2)
//   R2  wbcMeasuredPass, wbcInertiaAndJacobians            (S3, S4: M, nle with -J_ee' f_e, the feet and arm Jacobians)
//   R3  wbcDesiredPass                                     (S5, on this same wavefront, with body / dof tables of its own)
//   R4  wbcTask0Rows: D0, f0;  wbcAssembleTask per level: A, b (rebuilt in place once the level's residual is formed)
// This kernel's own work is the products and the reductions:
//   R5  D0 x  ->  ineq_margin = f0 - D0 x;  tau_i = (D0 x)_i + nle_j,i  (rows 0..17 of D0 are [M_j | -J_j'], the row wbcUpdateCmd multiplies)
//   R6  A_l x ->  eq_residual[l] = A_l x - b_l
//   R7  summary: norms per level, minimum margins, counts against active_tol, the row of minimum margin
// Products: rows of A and D0 have a stride of ND = 36 doubles.  One lane per row would walk 72-dword strides, eight distinct banks for a group of 32 lanes
// (four-way conflicts).  A row is instead cut into four chunks of nine: the partial product (row, chunk) = e starts at double 9 e of the array, lane e takes
// it, so the 32 lanes of a group read doubles 9 lane + k -- 32 distinct even banks, conflict-free (9 is odd) -- and sixteen rows are done per pass.  The four
// partials of a row are added as (p0 + p1) + (p2 + p3) by one lane through LDS: the same order for every row, instance and batch.
//
// QM_WBCREPORT_EXTERN (the product build of qmgpu_api.hip, qm_door_amd/build.py): only the argument record and the kernel's declaration; the kernel is DEFINED in
// qmgpu_wbcreport.hip, a translation unit of its own (as plant_kernel: plant_kernel.h says why), compiled with its kernel namespace renamed; the report kernel and
// its arguments live in namespace qmwbcreport, which the rename does not touch.
#pragma once
#include "../../../include/qmgpu.h"
#include "wbc_report_lds.h"

namespace qmwbcreport {

struct ReportArgs {
  const qmgpu_problem* P;
  int batch, variant, xStride;
  const double* xDes; const double* uDes; const double* rbd; const int* mode; const double* period; const double* time; const double* eeForce;
  const double* inputLast; const double* x;
  double activeTol;
  double* eqResidual; double* ineqMargin; double* tau; int* rows; double* summary;
};

}  // namespace qmwbcreport

#if defined(QM_WBCREPORT_EXTERN) && !defined(QM_RICCATI_TIMING)
#include "gpu_rt.h"
namespace qmwbcreport {
__global__ void __launch_bounds__(qmk::WBCREPORT_THREADS) wbc_report_kernel(ReportArgs a);
}
#else
#include "contact_rows.h"
#include "wbc_kernel.h"

namespace qmk {

// out[i] = (row i of Mx) . x for i < nrows; Mx row-major with stride ND, x[ND].  The lane assignment of the header: partial e = 4 row + chunk is the nine doubles from
// 9 e on, times x[9 chunk ..]; part: one double per lane.  Ends with the results visible to every lane.
__device__ __forceinline__ void reportRowDots(const double* Mx, int nrows, const double* x, double* part, double* out, int lane) {
  const int chunk = lane % WBCREPORT_CHUNKS;
  const int rowsPerPass = WBCREPORT_THREADS / WBCREPORT_CHUNKS;
#pragma unroll 1
  for (int r0 = 0; r0 < nrows; r0 += rowsPerPass) {
    const int row = r0 + lane / WBCREPORT_CHUNKS;
    double s = 0.0;
    if (row < nrows) {
      const double* m = Mx + (r0 * WBCREPORT_CHUNKS + lane) * WBCREPORT_CHUNK;
      const double* xc = x + chunk * WBCREPORT_CHUNK;
#pragma unroll
      for (int k = 0; k < WBCREPORT_CHUNK; ++k) s += m[k] * xc[k];
    }
    part[lane] = s;
    QM_WAVE_SYNC();
    if (lane < rowsPerPass && r0 + lane < nrows) {
      const double* p = part + lane * WBCREPORT_CHUNKS;
      out[r0 + lane] = (p[0] + p[1]) + (p[2] + p[3]);
    }
    QM_WAVE_SYNC();
  }
}

__device__ __forceinline__ void reportInstance(const qmwbcreport::ReportArgs& a) {
  QM_DYNAMIC_LDS(lds);
  QM_POISON_LDS(lds, WBCREPORT_LDS_DOUBLES);
  const int lane = threadIdx.x & 63, inst = blockIdx.x;
  if (inst >= a.batch) return;
  const qmgpu_model& md = a.P->model;
  const qmgpu_settings& st = a.P->settings;
  double* in = lds + RL_IN.off; double* rbd = in + IN_RBD; double* xDes = in + IN_XDES; double* uDes = in + IN_UDES; double* il = in + IN_LAST;
  double* qM = lds + RL_Q.off; double* vM = qM + NVV; double* qD = qM + 2 * NVV; double* vD = qM + 3 * NVV;
  double* xs = lds + RL_X.off;
  double* body = lds + RL_BODY.off; double* dof = lds + RL_DOF.off; double* wr = lds + RL_WR.off; double* M = lds + RL_M.off; double* nle = lds + RL_NLE.off;
  double* Jf = lds + RL_JF.off; double* Ja = lds + RL_JA.off; double* mi = lds + RL_MISC.off; double* part = lds + RL_PART.off; double* dot = lds + RL_DOT.off;
  double* JL = lds + RO_JL.off; double* A = lds + RL_A.off; double* bvec = lds + RL_B.off; double* D0 = lds + RL_D0.off; double* f0 = lds + RL_F0.off;
  double fe[3] = {0.0, 0.0, 0.0};
  if (a.eeForce) for (int i = 0; i < 3; ++i) fe[i] = a.eeForce[size_t(inst) * 3 + i];
  const int mode = a.mode[inst];
  const double period = a.period[inst], time = a.time[inst];
  bool contact[4]; int nst = 0;
  for (int c = 0; c < 4; ++c) { contact[c] = contactOf(mode, c); nst += contact[c] ? 1 : 0; }
  const int nsw = 4 - nst;
  const int m0 = 36 + 5 * nst + 3 * nsw;

  // ---- R1: the inputs of the tick through wbc_kernel's own loader (it reads inputLast, never writes it: the write of WbcBase.cpp:225 is wbc_kernel's), and x
  WbcArgs wa{};
  wa.P = a.P; wa.batch = a.batch; wa.variant = a.variant; wa.xDes = a.xDes; wa.uDes = a.uDes; wa.rbd = a.rbd; wa.mode = a.mode; wa.period = a.period; wa.time = a.time;
  wa.inputLast = const_cast<double*>(a.inputLast); wa.eeForce = a.eeForce;
  wbcLoadInputs(wa, inst, rbd, xDes, uDes, il, lane);
  if (lane < ND) xs[lane] = a.x[size_t(inst) * a.xStride + lane];
  QM_WAVE_SYNC();
  wbcCoordinates(rbd, xDes, uDes, il, period, qM, vM, qD, vD, mi, lane);
  QM_WAVE_SYNC();
  // ---- R2: the model at the measured state
  wbcMeasuredPass(md, st, qM, vM, body, dof, wr, lane);
  QM_WAVE_SYNC();
  wbcInertiaAndJacobians(md, fe, body, dof, wr, JL, M, nle, Jf, Ja, mi, lane);
  QM_WAVE_SYNC();
  // ---- R3: the desired pass (ends with its own hand-off)
  wbcDesiredPass(md, st, xDes, uDes, fe, qD, vD, mi, lds + RL_BODY2.off, lds + RL_DOF2.off, lane);

  // ---- R4 / R5: the inequality rows of level 0, their margins and the torque
  wbcTask0Rows(md, st, contact, m0, M, Jf, nle, D0, f0, lane);
  QM_WAVE_SYNC();
  reportRowDots(D0, MAXM, xs, part, dot, lane);
  const bool ineqRow = lane < m0;
  const double f0i = ineqRow ? f0[lane] : 0.0;
  const double margin = ineqRow ? f0i - dot[lane] : 0.0;
  if (a.ineqMargin && lane < MAXM) a.ineqMargin[size_t(inst) * MAXM + lane] = margin;
  if (a.tau && lane < 18) a.tau[size_t(inst) * 18 + lane] = dot[lane] + nle[6 + lane];
  const double inf = __builtin_huge_val();
  const double minTorque = qmAllMin(lane < 36 ? margin : inf);
  const double minFriction = qmAllMin(lane >= 36 && lane < 36 + 5 * nst ? margin : inf);
  const double minAll = qmAllMin(ineqRow ? margin : inf);
  const unsigned long long atMin = qmBallot(ineqRow && margin == minAll);
  const double band = a.activeTol * (1.0 + fabs(f0i));
  const int nActive = qmPopCount(qmBallot(ineqRow && margin <= band));
  const int nViolated = qmPopCount(qmBallot(ineqRow && margin < -band));
  QM_WAVE_SYNC();   // dot is rewritten below

  // ---- R4 / R6: the stacked equality task of every level
  double norm2[WBCREPORT_LEVELS], normInf[WBCREPORT_LEVELS];
  int rl[WBCREPORT_LEVELS];
#pragma unroll 1
  for (int level = 0; level < WBCREPORT_LEVELS; ++level) {
    const int r = wbcAssembleTask(level, a.variant, time, st, contact, nsw, M, nle, Jf, Ja, mi, qM, vM, qD, vD, uDes, A, bvec, lane);
    QM_WAVE_SYNC();
    reportRowDots(A, r, xs, part, dot, lane);
    const double res = lane < r ? dot[lane] - bvec[lane] : 0.0;
    if (a.eqResidual && lane < MAXR) a.eqResidual[(size_t(inst) * WBCREPORT_LEVELS + level) * MAXR + lane] = res;
    const double n2 = sqrt(qmAllSum(res * res)), ni = qmAllMax(fabs(res));
    // (level is a loop counter: the three slots are written through a chain of selects, not an indexed private array)
    for (int l = 0; l < WBCREPORT_LEVELS; ++l) if (l == level) { norm2[l] = n2; normInf[l] = ni; rl[l] = r; }
    QM_WAVE_SYNC();   // A, b and dot are rewritten by the next level
  }

  // ---- R7
  if (a.rows && lane < 4) a.rows[size_t(inst) * 4 + lane] = lane == 0 ? rl[0] : lane == 1 ? rl[1] : lane == 2 ? rl[2] : m0;
  if (a.summary && lane < WBCREPORT_SUMMARY) {
    double v = 0.0;
    switch (lane) {
      case 0: v = norm2[0]; break; case 1: v = norm2[1]; break; case 2: v = norm2[2]; break;
      case 3: v = normInf[0]; break; case 4: v = normInf[1]; break; case 5: v = normInf[2]; break;
      case 6: v = minTorque; break; case 7: v = minFriction; break; case 8: v = double(nActive); break; case 9: v = double(nViolated); break;
      case 10: v = atMin ? double(qmFirstBit(atMin)) : -1.0; break;
      default: break;
    }
    a.summary[size_t(inst) * WBCREPORT_SUMMARY + lane] = v;
  }
}

}  // namespace qmk

namespace qmwbcreport {
__global__ void __launch_bounds__(qmk::WBCREPORT_THREADS) wbc_report_kernel(ReportArgs a) { qmk::reportInstance(a); }
}
#endif   // QM_WBCREPORT_EXTERN
