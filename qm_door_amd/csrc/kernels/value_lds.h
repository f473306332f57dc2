// value_lds.h -- the dynamic LDS of one value_function_kernel workgroup: every region once, in address order (extent = rows x row stride).  The unit is `real`.
// value_kernel.h takes every offset from here.  No overlays: every region keeps its meaning for the whole kernel.
#pragma once
#include "layout.h"
#include "real.h"
#include "lds_region.h"
#include "riccati_lds.h"   // LDS_S: S has the sweep's image (row 30 = s, row / column 31 and column 30 zero)

namespace qmk {

// Row strides (reals) = 16 mod 32 for the images the matrix-core operands are read from: the four k-rows x sixteen consecutive columns of one operand read hit distinct banks
constexpr int LDS_VY = 48, LDS_VG = 48, LDS_VC = 34;
constexpr int VALUE_G_ROWS = 20;                     // MT rows of W (and of the gains) and two zero rows: five k steps of four
constexpr int VALUE_STG = OFF_DT + 1;                // reals of a record the kernel stages: the sweep's head (OFF_TAIL) and Pe, the contact mode, the step (the mode says m~)

using ValueRegion = LdsRegion<real, real>;
constexpr ValueRegion VL_STG{0, STAGE_DOUBLES};                         // the record of the node in flight, joint rows as A~ / B~ (commitDynamics); [A~ | b~] becomes [A_cl | b_cl] in place
constexpr auto VL_GN = ldsAfter<real>(VL_STG, GAIN_DOUBLES);            // its gains [K~ | k~] (layout.h: OFF_KFB, OFF_kff)
constexpr auto VL_S = ldsAfter<real>(VL_GN, 32 * LDS_S);                // S [32][LDS_S] of node k + 1, s as row 30
constexpr auto VL_Y = ldsAfter<real>(VL_S, 32 * LDS_VY);                // Y [32][LDS_VY] = S [A_cl | b_cl] with s added to column 30
constexpr auto VL_G = ldsAfter<real>(VL_Y, VALUE_G_ROWS * LDS_VG);      // W [20][LDS_VG] = [P~ | r~] + R~ [K~ | k~], rows >= m~ zero
constexpr auto VL_C = ldsAfter<real>(VL_G, 32 * LDS_VC);                // C [32][LDS_VC] = [Q~ | q~] + A_cl^T Y + P~^T [K~ | k~] + K~^T W before the symmetrisation
constexpr auto VL_X = ldsAfter<real>(VL_C, 32);                         // the linearisation state of node k + 1
constexpr int VALUE_LDS_REALS = VL_X.end();
constexpr int VALUE_LDS_BYTES = VALUE_LDS_REALS * int(sizeof(real));    // 72,768 B = 71.1 KiB at fp64
static_assert(VALUE_LDS_REALS == 9096, "the carve as it was measured");
static_assert(2 * VALUE_LDS_BYTES <= QM_CU_LDS_BYTES, "two instances share a compute unit");
static_assert(VALUE_STG % 2 == 0 && VALUE_STG <= VL_STG.count && VL_GN.off % 2 == 0 && GAIN_DOUBLES % 2 == 0, "16-byte copies");
static_assert(MT <= VALUE_G_ROWS && VALUE_G_ROWS % 4 == 0 && LDS_VY >= 32 && LDS_VG >= 32 && LDS_VC >= 32, "whole k steps; 32 columns per image");

}  // namespace qmk
