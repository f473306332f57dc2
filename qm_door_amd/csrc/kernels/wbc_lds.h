// wbc_lds.h -- the dynamic LDS of one wbc_kernel workgroup: every region once (name, element type, extent), the sub-regions of the exchange
// block, the control words, and every overlay with the assertion that the guest fits its host.  wbc_kernel.h (wbc_kernel, wbcNullSpace) and
// qp_dev.h (qpSolve and the helpers' shares) take every offset from here.
#pragma once
#include "../../../include/qmgpu.h"
#include "gpu_rt.h"
#include "lds_region.h"

namespace qmk {

constexpr int ND = 36, NVV = 24, MAXR = 22, MAXM = 56;   // decision variables, generalized velocities, task rows of a level, inequality rows
constexpr int LDZ = 37, LDK = 37;                        // row strides of the n-column (Z, A Z, D Z) and of the square (K, G) arrays
constexpr int QP_KMAX = 28;                              // pinned rows the small system of the level solver holds
constexpr int QP_SLD = QP_KMAX + 1;
constexpr int WBC_BODY_STRIDE = 33;                      // per body: R9 p3 c3 I6 w3 al3 vo3 ao3

// (LdsRegion, ldsAfter: lds_region.h; this kernel's regions count in doubles)
// An int region of LDS that is declared in doubles: the one place where the element type changes (a reinterpret_cast in effect, spelt through void*).  No int region shares storage with a double region.
__device__ __forceinline__ int* ldsInts(double* base, LdsRegion<int> r) { return static_cast<int*>(static_cast<void*>(base)) + 2 * r.off; }

// ---- the carve, in address order
constexpr LdsRegion<double> WL_IN{0, 160};                                                // inputs: rbd[55] xDes[30] uDes[30] inputLast[30] (+ pad)
constexpr int IN_RBD = 0, IN_XDES = 55, IN_UDES = 85, IN_LAST = 115;                     //   (offsets inside WL_IN)
constexpr auto WL_Q = ldsAfter<double>(WL_IN, 4 * NVV);                                    // qM vM qD vD [4][24]
constexpr auto WL_BODY = ldsAfter<double>(WL_Q, 640);                                      // body table of the measured pass [19][33] (+ pad)
constexpr auto WL_DOF = ldsAfter<double>(WL_BODY, 2 * NVV * 3);                            // dof axis[24][3], origin[24][3]
constexpr auto WL_WR = ldsAfter<double>(WL_DOF, 120);                                      // body wrench force[19][3] torque[19][3] (+ pad)
constexpr auto WL_M = ldsAfter<double>(WL_WR, NVV * NVV);                                  // M [24][24]
constexpr auto WL_NLE = ldsAfter<double>(WL_M, NVV);                                       // nle[24]
constexpr auto WL_JF = ldsAfter<double>(WL_NLE, 12 * NVV);                                 // feet J [12][24]
constexpr auto WL_JA = ldsAfter<double>(WL_JF, 6 * NVV);                                   // arm J [6][24]
constexpr auto WL_MISC = ldsAfter<double>(WL_JA, 144);                                     // mi: the MI_* entries of wbc_kernel.h
constexpr auto WL_A = ldsAfter<double>(WL_MISC, MAXR * ND);                                // task A [MAXR][36]
constexpr auto WL_B = ldsAfter<double>(WL_A, 24);                                          // task b [MAXR] (+ pad)
constexpr auto WL_D0 = ldsAfter<double>(WL_B, MAXM * ND);                                  // D0 [MAXM][36]
constexpr auto WL_F0 = ldsAfter<double>(WL_D0, MAXM);                                      // f0[56]
constexpr auto WL_V0 = ldsAfter<double>(WL_F0, MAXM);                                      // slack solution v0[56]
constexpr auto WL_Z = ldsAfter<double>(WL_V0, ND * LDZ);                                   // Z [36][LDZ]
constexpr auto WL_ZN = ldsAfter<double>(WL_Z, ND * LDZ);                                   // Z_new [36][LDZ]
constexpr auto WL_AZ = ldsAfter<double>(WL_ZN, MAXR * LDZ);                                // A Z [MAXR][LDZ]
constexpr auto WL_DZ = ldsAfter<double>(WL_AZ, MAXM * LDZ);                                // D0 Z [MAXM][LDZ]
constexpr auto WL_K = ldsAfter<double>(WL_DZ, ND * LDK);                                   // K / Cholesky / kernel basis N [36][LDK]
constexpr auto WL_G = ldsAfter<double>(WL_K, ND * LDK);                                    // G = (A Z)'(A Z) [36][LDK]
constexpr auto WL_VH = ldsAfter<double>(WL_G, MAXR * 40);                                  // table region: no contents of its own, see the overlays
constexpr auto WL_X = ldsAfter<double>(WL_VH, ND);                                         // x[36]
constexpr auto WL_ZS = ldsAfter<double>(WL_X, ND);                                         // z[36]: a level's solution in its own variables
constexpr auto WL_GS = ldsAfter<double>(WL_ZS, ND);                                        // (not used)
constexpr auto WL_RD = ldsAfter<double>(WL_GS, ND);                                        // rd[36]: z of the level, the residual of its canonical representative
constexpr auto WL_RHS = ldsAfter<double>(WL_RD, ND);                                       // (not used)
constexpr auto WL_DZS = ldsAfter<double>(WL_RHS, ND);                                      // dz[36]: right-hand side of the minimum-norm start
constexpr auto WL_FHAT = ldsAfter<double>(WL_DZS, MAXM);                                   // fhat[56]: margins of the inequality rows
constexpr auto WL_LAM = ldsAfter<double>(WL_FHAT, MAXM);                                   // (not used)
constexpr auto WL_WT = ldsAfter<double>(WL_LAM, MAXM);                                     // wt[56]: row weights of the K tiles, then 1 / L_cc
constexpr auto WL_TZ = ldsAfter<double>(WL_WT, MAXM);                                      // tz[56]: A x_prev - b of the level
constexpr auto WL_RED = ldsAfter<double>(WL_TZ, 1024);                                     // exchange block: sub-regions below
constexpr auto WL_CTL = ldsAfter<double>(WL_RED, 8);                                       // control words: CTL_* below
constexpr auto WL_BODY2 = ldsAfter<double>(WL_CTL, WL_BODY.count);                          // body / dof tables of the desired pass (wavefront 1)
constexpr auto WL_DOF2 = ldsAfter<double>(WL_BODY2, WL_DOF.count);
constexpr auto WL_TP = ldsAfter<double>(WL_DOF2, QP_KMAX * LDK);                           // T_P = L^-1 DZ_P' of the level solver's pinned rows [QP_KMAX][LDK]
constexpr int WBC_LDS_DOUBLES = WL_TP.end();
constexpr int WBC_LDS_BYTES = WBC_LDS_DOUBLES * 8;
static_assert(WBC_BODY_STRIDE * QMGPU_NB <= WL_BODY.count && 2 * 3 * QMGPU_NB <= WL_WR.count, "body and wrench tables");

// ---- the exchange block (offsets from its start: the level solver receives the block as one pointer)
constexpr LdsRegion<double> WX_BC{0, 64};                         // broadcast line of the level solver (z, multipliers, u, v ...)
constexpr auto WX_MS = ldsAfter<double>(WX_BC, 64);                // first the row of each slot, as a double; then the small system's right-hand side / solution by slot
constexpr auto WX_COLSUM = ldsAfter<double>(WX_MS, 4 * 64);        // partials of a 56-row column sum, one line per wavefront
constexpr auto WX_RES = ldsAfter<double>(WX_COLSUM, 64);           // task residual by task row; its absolute-value form is written into the same line afterwards
constexpr auto WX_RESABS = ldsAfter<double>(WX_RES, 64);           // free: once the line of the absolute-value form, nobody touches it
constexpr auto WX_FORKJOB = ldsAfter<double>(WX_RESABS, 10);       // the fork-join's product job: FJ_* below
// the ints of wbcNullSpace: regions of their own, never read or written as doubles.  Of the 1024 doubles of the block the level solver and the
// fork-join use 458 (and leave WX_RESABS alone); these take 98 more.
constexpr auto WX_COLPERM = ldsAfter<int>(WX_FORKJOB, 40);       // [36] the original column at every position
constexpr auto WX_ROWOF = ldsAfter<int>(WX_COLPERM, 24);         // [MAXR] the row that gave pivot k
constexpr auto WX_PIVOK = ldsAfter<int>(WX_ROWOF, 32);           // [MAXR] pivot k stands above the rank threshold
constexpr auto WX_FREEPOS = ldsAfter<int>(WX_PIVOK, 36);         // [36] the free column positions
constexpr auto WX_XCHGJ = ldsAfter<int>(WX_FREEPOS, 64);         // [64] the chunks' candidate columns (their magnitudes: WO_XCHGV)
constexpr auto WX_FREE = ldsAfter<double>(WX_XCHGJ, WL_RED.count - WX_XCHGJ.end());   // 404 doubles nobody touches (468 with WX_RESABS)
static_assert(MAXR <= WX_ROWOF.count && MAXR <= WX_PIVOK.count && ND <= WX_COLPERM.count && ND <= WX_FREEPOS.count, "index tables of the null-space step");
static_assert(WX_FREE.count >= 0 && WX_FREE.end() == WL_RED.count, "sub-regions of the exchange block");
enum { FJ_A = 0, FJ_LDA, FJ_B, FJ_LDB, FJ_M, FJ_N, FJ_K, FJ_D, FJ_LDD, FJ_DIAG, FJ_COUNT };   // C = op(A) B + diag: arrays as offsets from the LDS base
static_assert(FJ_COUNT == WX_FORKJOB.count, "fork job");

// ---- control words (WL_CTL): only the fork command is in use
constexpr int CTL_FORK = 4;      // command of the solving wavefront to the helpers: FORK_* below, or the size NP of the K tiles to share
static_assert(CTL_FORK < WL_CTL.count, "control words");
enum { FORK_LEAVE = 0, FORK_GEMM = 100, FORK_GEMM_T = 101, FORK_COLSUM = 200, FORK_JOIN = 300 };
constexpr int forkKTiles(int np) { return np; }   // the command that shares the K tiles of size NP (20 or 36) is NP itself

// ---- overlays: guest over host, and until when the host is dead
// Jacobian columns JL [19][24][6] over Z | Z_new | A Z: the three are first written when the cascade starts (Z = I), after S4 has read JL.
constexpr LdsRegion<double> WO_JL{WL_Z.off, QMGPU_NB * NVV * 6};
static_assert(WL_ZN.off == WL_Z.end() && WL_AZ.off == WL_ZN.end() && WO_JL.end() <= WL_AZ.end(), "Jacobian columns fit the Z / Z_new / A Z regions");
// scrA (rows of the implied-equality step, 24 rows of LDZ at a time) over BODY | DOF | WR, scrB (N_E, 18 rows) over BODY2 | DOF2: the tables of
// the model update are dead once both passes have joined (S5), for the rest of the kernel.
constexpr LdsRegion<double> WO_SCRA{WL_BODY.off, WL_BODY.count + WL_DOF.count + WL_WR.count};
constexpr LdsRegion<double> WO_SCRB{WL_BODY2.off, WL_BODY2.count + WL_DOF2.count};
static_assert(WL_DOF.off == WL_BODY.end() && WL_WR.off == WL_DOF.end() && WO_SCRA.end() == WL_M.off && 24 * LDZ <= WO_SCRA.count && MAXR * LDZ <= WO_SCRA.count, "scratch A of the implied-equality step");
static_assert(WL_DOF2.off == WL_BODY2.end() && WO_SCRB.end() == WL_TP.off && 18 * LDZ <= WO_SCRB.count, "scratch B of the implied-equality step");
// The table region WL_VH has two guests that take turns, each rebuilt from nothing by its owner on entry:
//   qpSolve: the small system S [QP_KMAX][QP_SLD] of the pinned rows, from factorisation to return;
//   wbcNullSpace: the magnitudes of the chunks' candidates, from entry to return.
constexpr LdsRegion<double> WO_S{WL_VH.off, QP_KMAX * QP_SLD};
static_assert(WO_S.end() <= WL_VH.end(), "the small system of the pinned rows fits the table region");
constexpr LdsRegion<double> WO_XCHGV{WL_VH.off, 64};
static_assert(WO_XCHGV.end() <= WL_VH.end(), "candidate exchange of the null-space step fits the table region");
// B = W^-1 (A Z)' [36][LDZ] of the minimum-norm start (levelQp) over Z_new: Z_new is first written by the level's own Z N product, after the level's solve.
constexpr LdsRegion<double> WO_MNB{WL_ZN.off, ND * LDZ};
static_assert(WO_MNB.end() <= WL_ZN.end() && MAXR <= LDZ, "B of the minimum-norm start (n <= 36 rows of r <= MAXR entries) fits Z_new");

}  // namespace qmk
