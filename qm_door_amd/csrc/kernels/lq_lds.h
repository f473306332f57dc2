// lq_lds.h -- the LDS of one lq_node_kernel workgroup (one wavefront, one shooting node): every region once, in address order, the named vectors of VEC, and
// the overlays, each with the assertion that the guest fits its host and one line on when the host is dead.  The unit is `real`: the fp32 build carves floats
// with the same numbers.  lq_kernel.h takes every offset from here.  Every hand-off between aliases crosses a QM_WAVE_SYNC(); ticks are the kernel's QM_TICK sections.
//
// 12.7 KiB per node at fp64, twelve nodes per CU = THREE wavefronts per SIMD.  The kernel is latency bound (readlane chains, LDS round trips, dependent
// matrix-core accumulations): at one wavefront per SIMD it ran 1.10 ms per launch, at two 0.44 ms, at three 0.39 ms.  What keeps it this small:
//   * Pall = [Px | Pe | 0 | Pu] is stored for its 18 dense joint-velocity rows only; the 12 force rows are unit vectors / pinned
//     values and are synthesised into the matrix-core operands from registers;
//   * R' and Q never enter LDS: the operand / accumulator entries are assembled where they are needed from the constant
//     matrices (global, L1 resident) plus the few barrier terms parked in LDS;
//   * the dense rows of [A | B] never enter LDS: products (1) reads its operands straight from the AD rows (global, cache resident);
//   * W = R Pall is produced one 16-column tile at a time and never enters LDS: in the fp64 accumulator map register r of a lane
//     holds row h + 4 r, which is the row of k step r it supplies as a B operand (gpu_rt.h; the fp32 build permutes A rows to the
//     same map), so the tile feeds G = Pall^T W from the registers it was accumulated in;
//   * the zero rows of Q_v (18..31) and of Y (12..15) are synthesised into the operands, not stored.
#pragma once
#include "layout.h"
#include "real.h"
#include "lds_region.h"

namespace qmk {

constexpr int PAW = 50;                      // row stride of the dense rows of Pall (columns 0..29 Px, 30 Pe, 31 zero, 32..32+m~-1 Pu)
constexpr int CDW = 49;                      // row stride of [C | D_v] (48 used: the 30 state columns and the 18 joint-velocity columns)
constexpr int LDQ = 18, LDY = 34;            // row strides of Q_v and of Y
constexpr int XU_LD = 32, EEJ_LD = 32;       // row strides of x | u | x_next | dx and of the EE error Jacobian
static_assert(PAW == 32 + MT && CDW >= NX + 18 && LDQ >= 18 && LDY >= 32 && XU_LD >= NX && EEJ_LD >= NX, "every row holds its columns");

// ---- the carve, in address order
using LqRegion = LdsRegion<real, real>;
constexpr LqRegion LQ_X{0, 18 * LDQ};                          // X: x u x_next dx (+ fin, red), then Q_v -- see the overlays
constexpr auto LQ_PA = ldsAfter<real>(LQ_X, 18 * PAW);         // PA: [C | D_v], then Y, then rows 12..29 of Pall -- see the overlays
constexpr auto LQ_EEJ = ldsAfter<real>(LQ_PA, 6 * EEJ_LD);     // EE error Jacobian [6][EEJ_LD]                           ticks 0..9
// VEC, ticks 0..9: the named vectors (+ n: padding behind them)
constexpr auto LV_B = ldsAfter<real>(LQ_EEJ, 30);              // b: defect of the dynamics
constexpr auto LV_R = ldsAfter<real>(LV_B, 30);                // r: dt-scaled input-cost gradient
constexpr auto LV_E = ldsAfter<real>(LV_R, NCMAX);             // e: constant column of the constraint rows
constexpr auto LV_EEH = ldsAfter<real>(LV_E, 6 + 2);           // eeh: end-effector pose error
constexpr auto LV_PE = ldsAfter<real>(LV_EEH, 12);             // pe: force rows of Pe (pinned swing forces)
constexpr auto LV_FB = ldsAfter<real>(LV_PE, 36);              // fb: four 3 x 3 friction-cone Hessian blocks
constexpr auto LV_DDP = ldsAfter<real>(LV_FB, 6);              // ddp: arm joint-position barrier diagonal
constexpr auto LV_DDV = ldsAfter<real>(LV_DDP, 6 + 4);         // ddv: arm joint-velocity barrier diagonal
constexpr auto LV_Q = ldsAfter<real>(LV_DDV, 30 + 2);          // q: state-cost gradient
constexpr auto LV_COST = ldsAfter<real>(LV_Q, 30 + 2);         // cost: per-lane cost parts
constexpr LqRegion LQ_VEC{LV_B.off, LV_COST.end() - LV_B.off};
constexpr int LQ_LDS_DOUBLES = LQ_VEC.end();
static_assert(LQ_LDS_DOUBLES == 1628 && LQ_VEC.count == 84 + 64 + 32 + 32, "the carve as it was measured: 13,024 B at fp64");
static_assert(LQ_LDS_DOUBLES * sizeof(real) * 12 <= QM_CU_LDS_BYTES, "twelve nodes per CU");

// ---- guests of X
// x u x_next dx [4][XU_LD]: ticks 0..3, dead at the sync in front of the QR (tick 5).  fin[64], red[64] behind them: red in the terminal path (tick 1, beside
// x u x_next dx) and after products (1); fin in products (2)(3).
constexpr LqRegion LO_XU{LQ_X.off, 4 * XU_LD};
constexpr auto LO_FIN = ldsAfter<real>(LO_XU, 64);
constexpr auto LO_RED = ldsAfter<real>(LO_FIN, 64);
static_assert(LO_FIN.off >= LO_XU.end() && LO_RED.off >= LO_FIN.end() && LO_RED.end() <= LQ_X.end(), "x u x_next dx, fin and red lie side by side inside X");
// Q_v [18][LDQ]: published after the QR (tick 5, x u x_next dx are dead), dead at the sync after Pall is complete (tick 6).  It covers fin and red, which are used
// before (red, terminal path) and after it (red after products (1), fin in products (2)(3)) only.
constexpr LqRegion LO_QV{LQ_X.off, 18 * LDQ};
static_assert(LO_QV.end() <= LQ_X.end(), "Q_v lies inside X");

// ---- guests of PA
constexpr LqRegion LO_CD{LQ_PA.off, NCMAX * CDW};     // [C | D_v] [16][CDW]: ticks 0..5, dead at the sync in front of the QR
constexpr LqRegion LO_Y{LQ_PA.off, 12 * LDY};         // Y [12][LDY]: tick 5, published after the QR, read by -Q_v1 Y, dead at the sync in front of the Pall stores
constexpr LqRegion LO_PALL{LQ_PA.off, 18 * PAW};      // rows 12..29 of Pall [18][PAW]: tick 5 .. the end of products (2)(3)
static_assert(LO_CD.end() <= LQ_PA.end() && LO_Y.end() <= LQ_PA.end() && LO_PALL.end() <= LQ_PA.end(), "[C | D_v], Y and the Pall rows share PA");

}  // namespace qmk
