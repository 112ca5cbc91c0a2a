// wx_ens_cell_common.h -- what the definition headers of the ensemble calls (wx_ens_*_cell.h), wx_diag.h and wx_rounded.h share, as
// plain C++ that a host compiler takes without the HIP headers (the tests/native/ens_*_main.cpp drivers compile the definition headers
// under AddressSanitizer and UBSan): the one __host__ __device__ macro, the bit tests of a float and a double, the first member walk's
// step that three calls word alike, and the predicate of the in-place writes. Each namespace that uses one of these names it with a
// `using` declaration, so a call site reads wxa::sum_add or wxd::f32_finite as before.
#pragma once
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define WX_HD __host__ __device__
#else
#define WX_HD
#endif

namespace wxcell {

WX_HD inline uint32_t f32_bits(float v)
{
  uint32_t u;
  memcpy(&u, &v, 4);
  return u;
}
WX_HD inline bool f32_finite(float v) { return ((f32_bits(v) >> 23) & 255u) != 255u; }
WX_HD inline bool f64_finite(double v)
{
  uint64_t u;
  memcpy(&u, &v, 8);
  return ((u >> 52) & 2047u) != 2047u;
}

// One channel of one cell, the first walk over the members (assimilation, inflation, covariance): the sum in member order, and whether
// every member's value may enter. A select, not a branch, as wx_ens_stat.h's cell_add.
WX_HD inline void sum_add(double &S, bool &ok, float x, bool air)
{
#pragma clang fp contract(off)
  ok = ok && air && f32_finite(x);
  S = S + (double)x;
}

// The in-place writes (assimilation, inflation) store a member's texel only if one of its four words changed BITS: o is what the call
// makes of v. T: anything with float members x, y, z, w.
template <class T>
WX_HD inline bool texel_changed(const T &o, const T &v)
{
  return f32_bits(o.x) != f32_bits(v.x) || f32_bits(o.y) != f32_bits(v.y) || f32_bits(o.z) != f32_bits(v.z) || f32_bits(o.w) != f32_bits(v.w);
}

} // namespace wxcell
