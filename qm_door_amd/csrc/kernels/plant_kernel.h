// plant_kernel -- the plant step: hybrid joint law and rigid-contact forward dynamics of the 24-DoF model the WBC evaluates, driven by joint torques, the feet
// named by the contact mode pinned.  One wavefront per robot instance, every matrix in (dynamic) LDS, the substeps a loop inside the kernel.
//
// The joint law stands in for QMHWSim::writeSim (qm_gazebo/src/QMHWSim.cpp:98-114; the gains come from QMController::updateControlLaw,
// qm_controllers/src/QMController.cpp:178-191).  Everything else -- the simulator behind QMHWSim in the reference -- is this project's OWN FORMULATION
// (include/qmgpu.h).  Per substep of h = dt / S, in the WBC's coordinates q = [p, zyx, q_j], v = dq/dt:
//   P1  tau_j = kp_j (pos_des_j - q_j) + kd_j (vel_des_j - v_j) + tau_ff_j, clamped to the effort limits if asked
//   P2  M(q), nle(q, v) (with -J_ee' f_e), the feet Jacobian: wbc_kernel's S3 and S4, called as they are (wbcMeasuredPass, wbcInertiaAndJacobians)
//   P3  M = L L';  [Y | w] = L^-1 [Jc' | b], b = S' tau - nle, one right-hand side per lane;  G = Y'Y, its Cholesky factor,  G F = -(Jc v / h + Y'w)
//   P4  v+ = v + h M^-1 (b + Jc' F)  (ldsCholSolve),  q+ = q + h v+
// and after the last substep one more kinematic pass (bodyPass) for the end-effector slots of rbd_next.
//
// QM_PLANT_EXTERN (the product build of qmgpu_api.hip, qm_door_amd/build.py): only the argument record and the kernel's declaration; the kernel is DEFINED in
// qmgpu_plant.hip, a translation unit of its own, so that the translation units of the other kernels compile from unchanged input (wbc_kernel's results have
// depended on its surroundings twice).  That unit includes wbc_kernel.h for the device functions and is compiled with its kernel
// namespace renamed (-Dqmk=..., as qmgpu_mpc32.hip), so the copy of wbc_kernel it carries has a name of its own; the plant kernel and its arguments live in
// namespace qmplant, which the rename does not touch.
#pragma once
#include "../../../include/qmgpu.h"
#include "plant_lds.h"

namespace qmplant {

struct PlantArgs {
  const qmgpu_problem* P;
  int batch, substeps, clampEffort;
  const double* rbd; const double* tauFf; const double* posDes; const double* velDes; const double* kp; const double* kd;
  const int* mode; const double* dt; const double* eeForce;
  double* rbdNext; double* contactForce; double* tauApplied; int* status;
};
enum { PLANT_FAILED = 1, PLANT_PULL = 2, PLANT_FRICTION = 4 };   // qmgpu_plant_args::status

}  // namespace qmplant

#if defined(QM_PLANT_EXTERN) && !defined(QM_RICCATI_TIMING)
#include "gpu_rt.h"
namespace qmplant {
__global__ void __launch_bounds__(qmk::PLANT_THREADS) plant_kernel(PlantArgs a);
}
#else
#include "contact_rows.h"
#include "wbc_kernel.h"

namespace qmk {

// false for NaN and for +-inf
__device__ __forceinline__ bool plantFinite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// the row of the feet Jacobian Jf [12][24] that contact row r of Jc is: the rows of the feet in contact by `mode`, in foot order (0 for r >= 3 stanceCount(mode))
__device__ __forceinline__ int plantJfRow(int mode, int r) {
  int cnt = 0, row = 0;
  for (int c = 0; c < FEET; ++c) if (contactOf(mode, c)) { if (r / 3 == cnt) row = 3 * c + r % 3; ++cnt; }
  return row;
}
// the first contact row of foot c (meaningful for a foot in contact)
__device__ __forceinline__ int plantRowOfFoot(int mode, int c) {
  int cnt = 0;
  for (int k = 0; k < c; ++k) cnt += contactOf(mode, k) ? 1 : 0;
  return 3 * cnt;
}

// Euler rates v[3..5] of the world angular velocity w at the angles q[3..5], and back: the map of wbcCoordinates (wbc_kernel.h) and its inverse, the map of bodyPass
__device__ __forceinline__ void plantEulerRates(const double* q, const double* w, double* v) {
  double sz, cz, sy, cy;
  sincos(q[3], &sz, &cz); sincos(q[4], &sy, &cy);
  const double wx = w[0], wy = w[1], wz = w[2];
  const double tmp = cz * wx / cy + sz * wy / cy;
  v[3] = sy * tmp + wz; v[4] = -sz * wx + cz * wy; v[5] = tmp;
}
__device__ __forceinline__ void plantAngularVelocity(const double* q, const double* v, double* w) {
  double sz, cz, sy, cy;
  sincos(q[3], &sz, &cz); sincos(q[4], &sy, &cy);
  const double* de = v + 3;
  w[0] = -sz * de[1] + cy * cz * de[2]; w[1] = cz * de[1] + cy * sz * de[2]; w[2] = de[0] - sy * de[2];
}
// Pinocchio coordinates of an rbd state: the measured half of wbcCoordinates (wbc_kernel.h), restated because that function also forms the desired coordinates
// from a plan this kernel does not have.  Same expressions, same order.
__device__ __forceinline__ void plantCoordinates(const double* rbd, double* q, double* v, int lane) {
  if (lane == 0) {
    for (int i = 0; i < 3; ++i) { q[i] = rbd[3 + i]; q[3 + i] = rbd[i]; v[i] = rbd[24 + 3 + i]; }
    for (int j = 0; j < 18; ++j) { q[6 + j] = rbd[6 + j]; v[6 + j] = rbd[24 + 6 + j]; }
    plantEulerRates(q, rbd + 24, v);
  }
}

// L (lower triangle, row stride LDK: what ldsCholSolve reads) of A = L L', A n x n symmetric with row stride lda (its lower triangle is read); lane = row, column by
// column.  Returns false, wave-uniformly, at the first pivot that is not positive and finite.
__device__ inline bool plantCholFactor(const double* A, int n, int lda, double* L, int lane) {
#pragma unroll 1
  for (int j = 0; j < n; ++j) {
    if (lane >= j && lane < n) {
      double s = A[lane * lda + j];
      for (int k = 0; k < j; ++k) s -= L[lane * LDK + k] * L[j * LDK + k];
      L[lane * LDK + j] = s;
    }
    QM_WAVE_SYNC();
    const double d = L[j * LDK + j];
    if (!(d > 0.0) || !plantFinite(d)) return false;
    const double r = sqrt(d);
    QM_WAVE_SYNC();
    if (lane == j) L[j * LDK + j] = r;
    else if (lane > j && lane < n) L[lane * LDK + j] /= r;
    QM_WAVE_SYNC();
  }
  return true;
}

// rbd_next of (q, v) except its angular velocity (out[24..26], which every substep leaves there): the inverse of plantCoordinates, and the end-effector slots from the
// body table of a pass at q (StateEstimateBase.cpp:89-102)
__device__ __forceinline__ void plantStateRecord(const qmgpu_model& md, const double* q, const double* v, const double* body, double* out, int lane) {
  if (lane == 0) {
    for (int i = 0; i < 3; ++i) { out[i] = q[3 + i]; out[3 + i] = q[i]; out[24 + 3 + i] = v[i]; }
    for (int j = 0; j < 18; ++j) { out[6 + j] = q[6 + j]; out[24 + 6 + j] = v[6 + j]; }
    double pos[3], vel[3], acc[3];
    pointKin(md, body, md.ee_body, md.ee_offset, pos, vel, acc);
    const double* o = body + md.ee_body * WBC_BODY_STRIDE;
    Mat3<double> R;
    R.c0 = Vec3<double>(o[0], o[3], o[6]); R.c1 = Vec3<double>(o[1], o[4], o[7]); R.c2 = Vec3<double>(o[2], o[5], o[8]);
    double qe[4];
    matrixToQuaternion(R, qe);
    for (int i = 0; i < 3; ++i) out[48 + i] = pos[i];
    for (int i = 0; i < 4; ++i) out[51 + i] = qe[i];
  }
}

__device__ __forceinline__ void plantInstance(const qmplant::PlantArgs& a) {
  QM_DYNAMIC_LDS(lds);
  QM_POISON_LDS(lds, PLANT_LDS_DOUBLES);
  const int lane = threadIdx.x & 63, inst = blockIdx.x;
  if (inst >= a.batch) return;
  const qmgpu_model& md = a.P->model;
  const qmgpu_settings& st = a.P->settings;
  double* rbd = lds + PL_IN.off; double* out = lds + PL_OUT.off; double* q = lds + PL_Q.off; double* v = q + NVV; double* cmd = lds + PL_CMD.off;
  double* body = lds + PL_BODY.off; double* dof = lds + PL_DOF.off; double* wr = lds + PL_WR.off; double* M = lds + PL_M.off; double* nle = lds + PL_NLE.off;
  double* Jf = lds + PL_JF.off; double* Ja = lds + PL_JA.off; double* mi = lds + PL_MISC.off; double* bv = lds + PL_B.off; double* uv = lds + PL_U.off; double* F = lds + PL_F.off;
  double* JL = lds + PL_JL.off; double* L = lds + PO_L.off; double* YT = lds + PO_YT.off; double* G = lds + PO_G.off; double* LG = lds + PO_LG.off;
  double fe[3] = {0.0, 0.0, 0.0};
  if (a.eeForce) for (int i = 0; i < 3; ++i) fe[i] = a.eeForce[size_t(inst) * 3 + i];
  const int mode = a.mode[inst] & 15;
  const int nc = 3 * stanceCount(mode);
  const double h = a.dt[inst] / double(a.substeps);
  const double mu = st.wbc_friction_coefficient;

  if (lane < 55) rbd[lane] = a.rbd[size_t(inst) * 55 + lane];
  if (lane < 18) {
    const size_t e = size_t(inst) * 18 + lane;
    cmd[CMD_FF + lane] = a.tauFf[e];
    cmd[CMD_PD + lane] = a.posDes ? a.posDes[e] : 0.0; cmd[CMD_VD + lane] = a.velDes ? a.velDes[e] : 0.0;
    cmd[CMD_KP + lane] = a.kp ? a.kp[e] : 0.0; cmd[CMD_KD + lane] = a.kd ? a.kd[e] : 0.0;
    cmd[CMD_TAU + lane] = 0.0;
  }
  if (lane < PLANT_NC) F[lane] = 0.0;
  QM_WAVE_SYNC();
  plantCoordinates(rbd, q, v, lane);
  QM_WAVE_SYNC();

  int status = 0;
  bool failed = false;
#pragma unroll 1
  for (int s = 0; s < a.substeps; ++s) {
    // ---- P1: the joint law (QMHWSim.cpp:112-113: position term, plus velocity term, plus feed-forward) and the clamp (the limits of wbcTask0Rows)
    if (lane < 18) {
      double t = cmd[CMD_KP + lane] * (cmd[CMD_PD + lane] - q[6 + lane]) + cmd[CMD_KD + lane] * (cmd[CMD_VD + lane] - v[6 + lane]) + cmd[CMD_FF + lane];
      if (a.clampEffort) {
        const double lim = lane < 12 ? md.effort_limit[lane % 3] : md.effort_limit[lane];
        t = t > lim ? lim : (t < -lim ? -lim : t);
      }
      cmd[CMD_TAU + lane] = t;
    }
    QM_WAVE_SYNC();
    // ---- P2: the model
    wbcMeasuredPass(md, st, q, v, body, dof, wr, lane);
    QM_WAVE_SYNC();
    wbcInertiaAndJacobians(md, fe, body, dof, wr, JL, M, nle, Jf, Ja, mi, lane);
    QM_WAVE_SYNC();
    // ---- P3: M = L L' (over JL, which nobody reads any more), b, [Y | w]
    if (!plantCholFactor(M, NVV, NVV, L, lane)) { failed = true; break; }
    if (lane < NVV) bv[lane] = (lane >= 6 ? cmd[CMD_TAU + lane - 6] : 0.0) - nle[lane];
    QM_WAVE_SYNC();
    if (lane < nc || lane == PLANT_NC) {   // forward substitution, one right-hand side per lane, the column in registers
      const double* rhs = lane < nc ? Jf + plantJfRow(mode, lane) * NVV : bv;
      double y[NVV];
#pragma unroll
      for (int k = 0; k < NVV; ++k) {
        double acc = rhs[k];
#pragma unroll
        for (int m = 0; m < k; ++m) acc -= L[k * LDK + m] * y[m];
        y[k] = acc / L[k * LDK + k];
      }
#pragma unroll
      for (int k = 0; k < NVV; ++k) YT[lane * NVV + k] = y[k];
    }
    QM_WAVE_SYNC();
    if (nc > 0) {   // (wave-uniform; in flight there is no G)
      for (int e = lane; e < nc * nc; e += 64) {
        const int i = e / nc, j = e - i * nc;
        double acc = 0.0;
        for (int k = 0; k < NVV; ++k) acc += YT[i * NVV + k] * YT[j * NVV + k];
        G[i * PLANT_NC + j] = acc;
      }
      if (lane < nc) {
        const double* jr = Jf + plantJfRow(mode, lane) * NVV;
        double jv = 0.0, yw = 0.0;
        for (int k = 0; k < NVV; ++k) { jv += jr[k] * v[k]; yw += YT[lane * NVV + k] * YT[PLANT_NC * NVV + k]; }
        F[lane] = -(jv / h + yw);
      }
      QM_WAVE_SYNC();
      if (!plantCholFactor(G, nc, PLANT_NC, LG, lane)) { failed = true; break; }
      ldsCholSolve(LG, nc, F, lane);
    }
    // ---- P4: v+ = v + h M^-1 (b + Jc' F), q+ = q + h v+
    if (lane < NVV) {
      double acc = bv[lane];
      for (int i = 0; i < nc; ++i) acc += Jf[plantJfRow(mode, i) * NVV + lane] * F[i];
      uv[lane] = acc;
    }
    QM_WAVE_SYNC();
    ldsCholSolve(L, NVV, uv, lane);
    double vn = 0.0, qn = 0.0;
    if (lane < NVV) { vn = v[lane] + h * uv[lane]; qn = q[lane] + h * vn; }
    const bool bad = (lane < NVV && !(plantFinite(vn) && plantFinite(qn))) || (lane < nc && !plantFinite(F[lane])) || (lane < 18 && !plantFinite(cmd[CMD_TAU + lane]));
    if (qmBallot(bad) != 0ull) { failed = true; break; }
    if (lane < NVV) { v[lane] = vn; q[lane] = qn; }
    QM_WAVE_SYNC();
    // the state passes through its rbd form between substeps, as it does between calls: S substeps are S calls of dt / S, bit for bit
    if (lane == 0) { plantAngularVelocity(q, v, out + 24); plantEulerRates(q, out + 24, v); }
    // the reports: a stance foot that pulls, a stance foot outside the friction pyramid
    bool pull = false, slip = false;
    if (lane < FEET && contactOf(mode, lane)) {
      const double* f = F + plantRowOfFoot(mode, lane);
      pull = f[2] < 0.0;
      slip = fabs(f[0]) > mu * f[2] || fabs(f[1]) > mu * f[2];
    }
    if (qmBallot(pull) != 0ull) status |= qmplant::PLANT_PULL;
    if (qmBallot(slip) != 0ull) status |= qmplant::PLANT_FRICTION;
    QM_WAVE_SYNC();
  }

  QM_WAVE_SYNC();
  if (!failed) {   // the end-effector slots at q+: one more kinematic pass
    bodyPass(md, q, v, nullptr, body, dof, lane);
    QM_WAVE_SYNC();
    plantStateRecord(md, q, v, body, out, lane);
    QM_WAVE_SYNC();
    if (lane < 55 && !plantFinite(out[lane])) failed = true;
    failed = qmBallot(failed) != 0ull;
  }
  if (failed) status |= qmplant::PLANT_FAILED;
  if (lane < 55) a.rbdNext[size_t(inst) * 55 + lane] = failed ? rbd[lane] : out[lane];
  if (a.contactForce && lane < PLANT_NC) {
    const int c = lane / 3;
    a.contactForce[size_t(inst) * PLANT_NC + lane] = (!failed && contactOf(mode, c)) ? F[plantRowOfFoot(mode, c) + lane % 3] : 0.0;
  }
  if (a.tauApplied && lane < 18) a.tauApplied[size_t(inst) * 18 + lane] = failed ? 0.0 : cmd[CMD_TAU + lane];
  if (a.status && lane == 0) a.status[inst] = status;
}

}  // namespace qmk

namespace qmplant {
__global__ void __launch_bounds__(qmk::PLANT_THREADS) plant_kernel(PlantArgs a) { qmk::plantInstance(a); }
}
#endif   // QM_PLANT_EXTERN
