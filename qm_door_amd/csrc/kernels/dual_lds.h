// dual_lds.h -- the dynamic LDS of one costate_kernel workgroup: every region once, in address order.  The unit is `real`.
// dual_kernel.h takes every offset from here.  No overlays: every region keeps its meaning for the whole kernel.  (dual_multiplier_kernel uses no LDS.)
#pragma once
#include "layout.h"
#include "real.h"
#include "lds_region.h"

namespace qmk {

constexpr int DUAL_STG = OFF_DT + 1;                 // reals of a record the sweep stages: the backward sweep's head (OFF_TAIL) and Pe, the contact mode (it says m~), the step
constexpr int DUAL_VEC = 32;                         // a 30- or MT-vector, padded

using DualRegion = LdsRegion<real, real>;
constexpr DualRegion DL_STG{0, STAGE_DOUBLES};                          // the record of node k, joint rows as A~ / B~ (commitDynamics)
constexpr auto DL_GN = ldsAfter<real>(DL_STG, 2 * GAIN_DOUBLES);        // the gains [K~ | k~] of node k in half k & 1; node k - 1 lands in the other half while K~ is still read
constexpr auto DL_LAM = ldsAfter<real>(DL_GN, DUAL_VEC);                // lambda_{k+1}
constexpr auto DL_DX = ldsAfter<real>(DL_LAM, DUAL_VEC);                // dx_k
constexpr auto DL_DU = ldsAfter<real>(DL_DX, DUAL_VEC);                 // du~_k = K~ dx_k + k~, rows >= m~ zero
constexpr auto DL_RHO = ldsAfter<real>(DL_DU, DUAL_VEC);                // rho_k = R~ du~ + P~ dx + r~ + B~' lambda_{k+1}: the input stationarity residual, rows >= m~ zero
constexpr int DUAL_LDS_REALS = DL_RHO.end();
constexpr int DUAL_LDS_BYTES = DUAL_LDS_REALS * int(sizeof(real));      // 36,544 B = 35.7 KiB at fp64
static_assert(DUAL_LDS_REALS == 4568, "the carve as it was measured");
static_assert(4 * DUAL_LDS_BYTES <= QM_CU_LDS_BYTES, "the LDS would let four instances share a compute unit (the register count decides: DESIGN.md section 4.10)");
static_assert(DUAL_STG % 2 == 0 && DUAL_STG <= DL_STG.count && DL_GN.off % 2 == 0 && GAIN_DOUBLES % 2 == 0, "16-byte copies");
static_assert(MT <= DUAL_VEC && NX <= DUAL_VEC, "a padded vector holds a state or a projected input");

}  // namespace qmk
