// plant_lds.h -- the dynamic LDS of one plant_kernel workgroup (one wavefront, one robot): every region once (name, element type, extent) and the
// overlay of the solve's arrays over the Jacobian columns, with the assertion that the guests fit their host.  The tables of the model update have the
// extents wbc_lds.h gives them (wbc_kernel's S2-S4 run here unchanged); plant_kernel.h takes every offset from here.
#pragma once
#include "layout.h"
#include "wbc_lds.h"

namespace qmk {

constexpr int PLANT_THREADS = 64;                        // one wavefront per instance
constexpr int PLANT_NC = 12;                             // contact rows at most: four feet of three
constexpr int PLANT_RHS = PLANT_NC + 1;                  // right-hand sides of the forward substitution: the rows of Jc and b

// ---- the carve, in address order
constexpr LdsRegion<double> PL_IN{0, 56};                                                  // rbd[55] of the call's input state, kept to the end (status bit 0 returns it) (+ pad)
constexpr auto PL_OUT = ldsAfter<double>(PL_IN, 56);                                       // rbd_next[55] (+ pad)
constexpr auto PL_Q = ldsAfter<double>(PL_OUT, 2 * NVV);                                   // q v [2][24]: the state the substeps advance
constexpr auto PL_CMD = ldsAfter<double>(PL_Q, 6 * 18);                                    // tau_ff pos_des vel_des kp kd tau [6][18]
constexpr int CMD_FF = 0, CMD_PD = 18, CMD_VD = 36, CMD_KP = 54, CMD_KD = 72, CMD_TAU = 90; //   (offsets inside PL_CMD)
constexpr auto PL_BODY = ldsAfter<double>(PL_CMD, WL_BODY.count);                          // body table [19][33] (+ pad)
constexpr auto PL_DOF = ldsAfter<double>(PL_BODY, WL_DOF.count);                           // dof axis[24][3], origin[24][3]
constexpr auto PL_WR = ldsAfter<double>(PL_DOF, WL_WR.count);                              // body wrench force[19][3] torque[19][3] (+ pad)
constexpr auto PL_M = ldsAfter<double>(PL_WR, WL_M.count);                                 // M [24][24]
constexpr auto PL_NLE = ldsAfter<double>(PL_M, WL_NLE.count);                              // nle[24]
constexpr auto PL_JF = ldsAfter<double>(PL_NLE, WL_JF.count);                              // feet J [12][24]
constexpr auto PL_JA = ldsAfter<double>(PL_JF, WL_JA.count);                               // arm J [6][24] (written by S4, not read)
constexpr auto PL_MISC = ldsAfter<double>(PL_JA, WL_MISC.count);                           // mi: the MI_* entries S4 writes (not read)
constexpr auto PL_B = ldsAfter<double>(PL_MISC, NVV);                                      // b = S' tau - nle [24]
constexpr auto PL_U = ldsAfter<double>(PL_B, NVV);                                         // b + Jc' F, then M^-1 of it [24]
constexpr auto PL_F = ldsAfter<double>(PL_U, PLANT_NC);                                    // right-hand side of G F = ., then F [12]
constexpr auto PL_JL = ldsAfter<double>(PL_F, WO_JL.count);                                // Jacobian columns JL [19][24][6] of S4; the solve's arrays over them
constexpr int PLANT_LDS_DOUBLES = PL_JL.end();
constexpr int PLANT_LDS_BYTES = PLANT_LDS_DOUBLES * 8;
static_assert(55 <= PL_IN.count && 55 <= PL_OUT.count, "the state records");
static_assert(3 * PLANT_LDS_BYTES <= QM_CU_LDS_BYTES, "three instances share a CU's LDS");

// ---- overlay: the solve over JL.  S4 has read JL for the last time when M is complete; the solve's arrays are dead when the next substep's S4 writes JL again.
constexpr LdsRegion<double> PO_L{PL_JL.off, NVV * LDK};                                    // L of M = L L' [24][LDK] (lower triangle; stride of ldsCholSolve)
constexpr auto PO_YT = ldsAfter<double>(PO_L, PLANT_RHS * NVV);                            // Y' = (L^-1 Jc')' [12][24], row 12: w = L^-1 b
constexpr auto PO_G = ldsAfter<double>(PO_YT, PLANT_NC * PLANT_NC);                        // G = Y'Y [12][12]
constexpr auto PO_LG = ldsAfter<double>(PO_G, PLANT_NC * LDK);                             // L of G [12][LDK]
static_assert(PO_LG.end() <= PL_JL.end(), "L, Y', G and its factor fit the Jacobian columns");

}  // namespace qmk
