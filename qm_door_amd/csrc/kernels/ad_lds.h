// ad_lds.h -- the LDS of one ad_node_kernel workgroup (one wavefront, AD_NODES shooting nodes side by side): every region once, in address order, with the extent of
// one node and the row stride inside it, the one overlay with its assertion, and the record of a parked foot.  The unit is `real`: the fp32 build carves floats with the
// same numbers.  ad_kernel.h takes every offset and stride into LDS from here.  Every hand-off between lanes crosses a QM_WAVE_SYNC().
//
// 39.1 KiB per wavefront at fp64: four wavefronts per CU, one per SIMD -- the sweep needs the whole register file.
#pragma once
#include "layout.h"
#include "lds_region.h"
#include "sweep_dev.h"

namespace qmk {

constexpr int AD_DIRS = 21;                  // configuration directions = lanes per node
constexpr int AD_NODES = 3;                  // nodes per wavefront

constexpr int AD_XU_LD = 64, AD_XU_U = 32;                  // x | u of one node: x at 0..29, u at AD_XU_U..AD_XU_U + 29
constexpr int AD_X2_NODE = 12;                              // x + dt k1 of one node: the momentum / base-pose states
constexpr int AD_A2_LD = 16, AD_A2_NODE = 12 * AD_A2_LD;    // J2[:, 0:12] of one node [12][AD_A2_LD], columns 12..15 zero: the A operand of the chain-rule product
constexpr int AD_J_LD = 64, AD_J_NODE = 12 * AD_J_LD;       // Jacobian rows of one node [12][AD_J_LD]: column l < 60 = d/d(x, u)_l, column 60 the value (an AD row, ad_kernel.h)
constexpr int AD_PARK_LD = 64, AD_PARK_SLOTS = 15;          // a parked foot: AD_PARK_SLOTS rows of AD_PARK_LD lane-private columns (parkFoot below)
constexpr int AD_PARK_FOOT = AD_PARK_SLOTS * AD_PARK_LD;
static_assert(AD_XU_U >= NX && AD_XU_LD >= AD_XU_U + NU && AD_A2_LD >= 12 && AD_J_LD > NX + NU && AD_PARK_LD >= 64, "every row holds its columns, every lane its column");

// ---- the carve, in address order
using AdRegion = LdsRegion<real, real>;
constexpr AdRegion ADL_XU{0, AD_NODES * AD_XU_LD};                            // [3][AD_XU_LD]   x | u per node
constexpr auto ADL_X2 = ldsAfter<real>(ADL_XU, AD_NODES * AD_X2_NODE);        // [3][12]         x + dt k1
constexpr auto ADL_A2 = ldsAfter<real>(ADL_X2, AD_NODES * AD_A2_NODE);        // [3][12][AD_A2_LD] J2[:, 0:12]
constexpr auto ADL_PARK = ldsAfter<real>(ADL_A2, 4 * AD_PARK_FOOT);           // [4][15][AD_PARK_LD] the four feet of the first stage, then the Jacobian rows (below)
constexpr auto ADL_PUB = ldsAfter<real>(ADL_PARK, AD_NODES * SWEEP_PUB_NODE); // [3][119]        primal composites of the five kinematic chains of each node (sweep_dev.h: centroidalSweepOwnChain)
constexpr int AD_LDS_DOUBLES = ADL_PUB.end();
static_assert(AD_LDS_DOUBLES == 5001, "the carve as it was measured: 40,008 B at fp64");
static_assert(AD_LDS_DOUBLES * sizeof(real) * 4 <= QM_CU_LDS_BYTES, "four wavefronts per CU");

// ---- guest of PARK
// J [3][12][AD_J_LD]: J1, then J1 + J2 + dt J2[:, q_j] in place.  The host is dead at the QM_WAVE_SYNC() behind the constraint rows of the first stage: every lane has
// read its parked feet by then; the feet of the second stage are not parked.
constexpr AdRegion ADL_J{ADL_PARK.off, AD_NODES * AD_J_NODE};
static_assert(ADL_J.end() <= ADL_PARK.end(), "the Jacobian rows reuse the parking area");

// ---- a parked foot: position r relative to the base and joint-induced velocity v of one foot, waiting for the base twist the sweep delivers last.  `p` points
// at the lane's column of the foot's first row.  The store and the load walk the one list of slots below.
template <class R, class V, class F> __device__ __forceinline__ void parkedFootSlots(R& r, V& v, F&& slot) {
  slot(0, r.x.v); slot(1, r.x.d); slot(2, r.y.v); slot(3, r.y.d); slot(4, r.z.v); slot(5, r.z.d);
  slot(6, v.x.v); slot(7, v.x.d); slot(8, v.x.e); slot(9, v.y.v); slot(10, v.y.d); slot(11, v.y.e); slot(12, v.z.v); slot(13, v.z.d); slot(14, v.z.e);
  static_assert(AD_PARK_SLOTS == 14 + 1, "one row of the parked foot per slot listed above");
}
__device__ __forceinline__ void parkFoot(real* p, const Vec3<Du>& r, const Vec3<Du3>& v) {
  parkedFootSlots(r, v, [&](int k, real s) { p[k * AD_PARK_LD] = s; });
}
__device__ __forceinline__ void parkedFoot(const real* p, Vec3<Du>& r, Vec3<Du3>& v) {
  parkedFootSlots(r, v, [&](int k, real& s) { s = p[k * AD_PARK_LD]; });
}

}  // namespace qmk
