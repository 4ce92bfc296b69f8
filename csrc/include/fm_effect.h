// What the two tiers of the effect-size gate share: K19 (pairwise_effect.hip,
// one wave per row) and K28 (pairwise_effect_wide.hip, one workgroup per row).
// The order-preserving key of a difference d = fl32(x - y) that the
// Hodges-Lehmann selection bisects over, and the gate on (delta, shift,
// base_med) with the row's stores.  Units that include it are built with
// -ffp-contract=off: the gate's `min_shift * |base_med| + min_shift_abs` is
// defined as separately rounded fp32 operations.
#pragma once
#include "fm_common.h"

namespace fm {

// Order-preserving key of a float, +-inf included (an overflowed difference
// sorts at its end).  No NaN reaches it: both operands are finite.
__device__ __forceinline__ unsigned eff_key(float x) {
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float eff_val(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

constexpr unsigned kKeyNegInf = 0x007FFFFFu;    // keys below it decode to NaN: no difference is <= them
constexpr unsigned kKeyNegZero = 0x7FFFFFFFu;   // every d < 0 has a key <= this one

// The float t with  key(d) > T  <=>  d > t  for every difference d (never
// -0, never NaN), for T >= kKeyNegInf.  T above key(+inf) decodes to NaN and
// d > NaN is false for all d, which is the right answer there too.
__device__ __forceinline__ float eff_threshold(unsigned T) {
  // key(d) > key(-0)  <=>  d >= +0  <=>  d > the largest negative subnormal
  return eff_val(T == kKeyNegZero ? kKeyNegZero - 1u : T);
}

// The gate's verdict on a row of N pairs; bound [M] is read only when
// directional != 0.  A row with N == 0 or a NaN delta / shift passes.
__device__ __forceinline__ bool effect_passes(int N, float delta, float shift, float bmed, int64_t row,
                                              float min_effect, float min_shift, float min_shift_abs,
                                              int directional, const int* __restrict__ bound, int M) {
  bool pass = true;
  if (N > 0 && !isnan(delta) && !isnan(shift)) {
    if (min_effect > 0.f && fabsf(delta) < min_effect) pass = false;
    if (min_shift > 0.f || min_shift_abs > 0.f) {
      const float a = fabsf(shift);
      const float need_shift = min_shift * fabsf(bmed) + min_shift_abs;
      if (!(a > 0.f && a >= need_shift)) pass = false;
    }
    if (directional != 0 && bound != nullptr) {
      const int bc = bound[(int)(row % M)];
      if (bc == 1 && shift <= 0.f) pass = false;
      if (bc == 2 && shift >= 0.f) pass = false;
    }
  }
  return pass;
}

// effect [R, 4], counts [R, 2] and passed [R] of one row (one thread)
__device__ __forceinline__ void effect_store(int64_t row, float delta, float shift, float bmed, int N, int gt, int lt,
                                             bool pass, float* __restrict__ effect, int* __restrict__ counts,
                                             int8_t* __restrict__ passed) {
  float4 e;
  e.x = delta; e.y = shift; e.z = bmed; e.w = (float)N;
  *reinterpret_cast<float4*>(effect + row * 4) = e;
  counts[row * 2] = gt;
  counts[row * 2 + 1] = lt;
  passed[row] = pass ? 1 : 0;
}

}  // namespace fm
