// Band decision with a sigma per point and per side: band_decide_pp_kernel
// and band_decide_2s_kernel in one, for the models whose band is asymmetric
// about its centre and depends on the phase (K26, seasonal_quantile_robust).
// Current points are compared against [centre - thr * sigma_lo[row, i], centre
// + thr * sigma_up[row, i]]; one wave per row.  A flagged point scores its
// excess in units of its own sigma of the side it left.  The arithmetic of a
// side is band_decide_pp_kernel's with that side's sigma in the place of
// sigma[row, i]: sigma_lo == sigma_up gives that kernel's outputs, and sigmas
// that are constant along a row give band_decide_2s_kernel's.  A NaN sigma
// makes its bound NaN, which flags nothing.
//
// thr * sigma is rounded on its own (see band_decide_pp.hip): built with
// contraction limited to single expressions, and the products kept in their
// own, never one half of a fused multiply-add.
// fm-hipcc-flags: -ffp-contract=on
#include "fm_common.h"

using namespace fm;

namespace {

__device__ __forceinline__ float half_band(float th, float sd) {
#pragma clang fp contract(off)
  const float ts = th * sd;
  return ts;
}

__global__ __launch_bounds__(256) void band_decide_pp_2s_kernel(
    const float* __restrict__ cur, int64_t ld_c, int n, const float* __restrict__ center, int64_t ld_f,
    const float* __restrict__ sigma_lo, const float* __restrict__ sigma_up, int64_t ld_s, int64_t R, int M,
    const float* __restrict__ thr, const int* __restrict__ bound, const float* __restrict__ minlb,
    const int8_t* __restrict__ diff, float pair_factor, float* __restrict__ upper, float* __restrict__ lower,
    unsigned long long* __restrict__ flags, int NW, int* __restrict__ count, float* __restrict__ score) {
  const int64_t row = (int64_t)blockIdx.x * 4 + wave_id();
  if (row >= R) return;
  const int lane = lane_id();
  const int m = (int)(row % M);
  float th = thr[m];
  if (diff != nullptr && diff[row]) th *= pair_factor;
  const int bd = bound[m];
  int cnt = 0;
  float best = 0.f;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    bool f = false;
    if (i < n) {
      const float c = center[row * ld_f + i];
      const float su = sigma_up[row * ld_s + i], sl = sigma_lo[row * ld_s + i];
      const float inv_u = su > 0.f ? 1.f / su : 0.f, inv_l = sl > 0.f ? 1.f / sl : 0.f;
      const float up = c + half_band(th, su);
      float lo = c - half_band(th, sl);
      if (lo < minlb[m]) lo = minlb[m];
      upper[row * n + i] = up;
      lower[row * n + i] = lo;
      const float x = cur[row * ld_c + i];
      if (isfinite(x) && isfinite(c)) {
        const bool hi = (bd & 1) && x > up;
        const bool lw = (bd & 2) && x < lo;
        f = hi || lw;
        if (f) {
          ++cnt;
          const float z = hi ? (su > 0.f ? (x - up) * inv_u : 1e30f) : (sl > 0.f ? (lo - x) * inv_l : 1e30f);
          best = z > best ? z : best;
        }
      }
    }
    const unsigned long long bal = __ballot(f);
    if (lane == 0 && i0 / 64 < NW) flags[row * NW + i0 / 64] = bal;
  }
  cnt = wave_sum(cnt);
  best = wave_max(best);
  if (lane == 0) {
    count[row] = cnt;
    score[row] = best;
  }
}

}  // namespace

// fm_band_decide with sigma_lo [R, n] and sigma_up [R, n] (one leading
// dimension ld_s for both) instead of one sigma [R]: upper / lower [R, n]
// dense, flags [R, NW] bit-packed, count and score [R].  Row r uses table entry
// r % M; diff (int8 [R], may be null) lowers the threshold by pair_factor.
// Nothing is launched unless NW words hold n flags.
FM_API int fm_band_decide_pp_2s(const float* cur, int64_t ld_c, int n, const float* center, int64_t ld_f,
                                const float* sigma_lo, const float* sigma_up, int64_t ld_s, int64_t R, int M,
                                const float* thr, const int* bound, const float* minlb, const int8_t* diff,
                                float pair_factor, float* upper, float* lower, unsigned long long* flags, int NW,
                                int* count, float* score, hipStream_t stream) {
  if (n < 0 || M < 1 || (int64_t)NW * 64 < n || R > 4 * (int64_t)0x7FFFFFFF) return (int)hipErrorInvalidValue;
  if (R <= 0) return 0;
  hipLaunchKernelGGL(band_decide_pp_2s_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, stream, cur, ld_c, n,
                     center, ld_f, sigma_lo, sigma_up, ld_s, R, M, thr, bound, minlb, diff, pair_factor, upper, lower,
                     flags, NW, count, score);
  FM_LAUNCH_CHECK();
  return 0;
}
