// lds_region.h -- a region of a kernel's LDS array, for the carves that declare every region once: wbc_lds.h, riccati_lds.h (dynamic LDS), lq_lds.h, ad_lds.h (one static
// array).  ls_lds.h, the fifth map, names the separate __shared__ arrays of linesearch_kernel and needs no regions.
#pragma once

namespace qmk {

// `count` elements of T, `off` units U behind the LDS base; a region starts where the one before it ends.  U is the type of the kernel's LDS array:
// double for wbc_kernel (whose int regions are declared in doubles), `real` for the kernels that are compiled once per precision.
template <class T, class U = double> struct LdsRegion {
  int off, count;
  constexpr int units() const { return int((count * sizeof(T) + sizeof(U) - 1) / sizeof(U)); }
  constexpr int end() const { return off + units(); }
};
template <class T, class P, class U> constexpr LdsRegion<T, U> ldsAfter(LdsRegion<P, U> prev, int count) { return LdsRegion<T, U>{prev.end(), count}; }

}  // namespace qmk
