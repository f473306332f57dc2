// wbc_report_lds.h -- the dynamic LDS of one wbc_report_kernel workgroup (one wavefront, one robot): every region once (name, element type, extent) and the
// overlay of the Jacobian columns over the task rows, with the assertion that the guest fits its host.  The tables of the model update have the extents
// wbc_lds.h gives them (wbc_kernel's S1-S5 and its task builders run here unchanged); wbc_report_kernel.h takes every offset from here.
#pragma once
#include "layout.h"
#include "wbc_lds.h"

namespace qmk {

constexpr int WBCREPORT_THREADS = 64;                    // one wavefront per instance
constexpr int WBCREPORT_LEVELS = 3;                      // levels of the cascade
constexpr int WBCREPORT_SUMMARY = 12;                    // qmgpu_wbc_report_args::summary
constexpr int WBCREPORT_CHUNK = 9;                       // a row of ND = 36 doubles is four chunks of nine: partial (row, chunk) = 4 row + chunk starts at 9 (4 row + chunk)
constexpr int WBCREPORT_CHUNKS = ND / WBCREPORT_CHUNK;
static_assert(WBCREPORT_CHUNKS * WBCREPORT_CHUNK == ND && WBCREPORT_CHUNKS == 4 && WBCREPORT_CHUNK % 2 == 1, "four chunks of an odd number of doubles per row: the lanes' walks fall on distinct banks");
static_assert(WBCREPORT_LEVELS == QMGPU_WBC_REPORT_LEVELS && MAXR == QMGPU_WBC_REPORT_EQ_ROWS && MAXM == QMGPU_WBC_REPORT_INEQ_ROWS && WBCREPORT_SUMMARY == QMGPU_WBC_REPORT_SUMMARY, "widths of the outputs");

// ---- the carve, in address order
constexpr LdsRegion<double> RL_IN{0, WL_IN.count};                                         // inputs: rbd[55] xDes[30] uDes[30] inputLast[30] (+ pad), offsets IN_* of wbc_lds.h
constexpr auto RL_Q = ldsAfter<double>(RL_IN, WL_Q.count);                                 // qM vM qD vD [4][24]
constexpr auto RL_X = ldsAfter<double>(RL_Q, 40);                                          // x[36]: the decision vector under evaluation (+ pad)
constexpr auto RL_BODY = ldsAfter<double>(RL_X, WL_BODY.count);                            // body table of the measured pass [19][33] (+ pad)
constexpr auto RL_DOF = ldsAfter<double>(RL_BODY, WL_DOF.count);                           // dof axis[24][3], origin[24][3]
constexpr auto RL_WR = ldsAfter<double>(RL_DOF, WL_WR.count);                              // body wrench force[19][3] torque[19][3] (+ pad)
constexpr auto RL_BODY2 = ldsAfter<double>(RL_WR, WL_BODY.count);                          // body / dof tables of the desired pass (same wavefront, after S4)
constexpr auto RL_DOF2 = ldsAfter<double>(RL_BODY2, WL_DOF.count);
constexpr auto RL_M = ldsAfter<double>(RL_DOF2, WL_M.count);                               // M [24][24]
constexpr auto RL_NLE = ldsAfter<double>(RL_M, WL_NLE.count);                              // nle[24]
constexpr auto RL_JF = ldsAfter<double>(RL_NLE, WL_JF.count);                              // feet J [12][24]
constexpr auto RL_JA = ldsAfter<double>(RL_JF, WL_JA.count);                               // arm J [6][24]
constexpr auto RL_MISC = ldsAfter<double>(RL_JA, WL_MISC.count);                           // mi: the MI_* entries of wbc_kernel.h
constexpr auto RL_PART = ldsAfter<double>(RL_MISC, 64);                                    // partial dot products of one pass, one per lane
constexpr auto RL_DOT = ldsAfter<double>(RL_PART, 64);                                     // row products A x (MAXR) or D0 x (MAXM)
constexpr auto RL_TASK = ldsAfter<double>(RL_DOT, WL_A.count + WL_B.count + WL_D0.count + WL_F0.count);   // the task rows A | b | D0 | f0: sub-regions below; S4's Jacobian columns before them
constexpr int WBCREPORT_LDS_DOUBLES = RL_TASK.end();
constexpr int WBCREPORT_LDS_BYTES = WBCREPORT_LDS_DOUBLES * 8;
static_assert(ND <= RL_X.count && MAXM <= RL_DOT.count && MAXR <= RL_DOT.count && WBCREPORT_THREADS <= RL_PART.count, "x, the partials and the row products");
static_assert(3 * WBCREPORT_LDS_BYTES <= QM_CU_LDS_BYTES, "three instances share a CU's LDS");

// ---- the task rows (sub-regions of RL_TASK, absolute offsets)
constexpr LdsRegion<double> RL_A{RL_TASK.off, WL_A.count};                                 // task A [MAXR][36], rebuilt per level
constexpr auto RL_B = ldsAfter<double>(RL_A, WL_B.count);                                  // task b [MAXR] (+ pad)
constexpr auto RL_D0 = ldsAfter<double>(RL_B, WL_D0.count);                                // D0 [MAXM][36]
constexpr auto RL_F0 = ldsAfter<double>(RL_D0, WL_F0.count);                               // f0 [MAXM]
static_assert(MAXR * ND <= RL_A.count && MAXR <= RL_B.count && MAXM * ND <= RL_D0.count && MAXM <= RL_F0.count && RL_F0.end() == RL_TASK.end(), "sub-regions of the task rows");

// ---- overlay: the Jacobian columns JL [19][24][6] of S4 over the task rows.  S4 has read JL for the last time when M is complete; the task rows are first written
// (cleared) by wbcTask0Rows / wbcAssembleTask after it.
constexpr LdsRegion<double> RO_JL{RL_TASK.off, WO_JL.count};
static_assert(RO_JL.end() <= RL_TASK.end(), "the Jacobian columns fit the task rows");

}  // namespace qmk
