// K24 quantile robust history statistics: per-row median and one sigma per
// side, each calibrated on a tail order statistic of the row, by exact
// MSB-first radix selection, one 512-thread workgroup per row.
//
// The row is read from HBM once and kept in LDS as the keys of
// fm_radix_select.h (load_row_keys), as K13 keeps it; three ranks are selected
// from the same keys: the lower middle, k_up = ceil(p (n - 1)) and k_lo =
// (n - 1) - k_up.  The keys are never rewritten (no deviations: K13's second
// half is not here).  The three ranks share the first radix pass
// (radix_select_ranks).  d_up = s[k_up] - centre and d_lo = centre - s[k_lo]
// are single order statistics, so they are exact; sigma = d / z0.  A side whose
// d is zero takes 1.2533 times the mean one-sided deviation instead, summed in
// fp64 in one more sweep, which a row runs only then (a branch uniform over the
// workgroup).  Rows longer than kRobustLdsKeys run the same passes re-reading
// global memory.  The contract is foremast_amd/ops/misc.py
// ref_quantile_robust_stats.
#include "fm_common.h"
#include "fm_quantile_row.h"   // quantile_row_stats
#include "fm_radix_select.h"

using namespace fm;

namespace {

constexpr int kQuantileThreads = 512;

static_assert(sizeof(SelectScratch<kQuantileThreads>) + 16 * sizeof(unsigned) + row_key_bytes(kRobustLdsKeys) <=
                      kLaunchLds, "the longest LDS row fits a launch");

template <int NT, bool LDS>
__global__ __launch_bounds__(NT) void quantile_robust_kernel(const float* __restrict__ hist, int64_t ld, int T,
                                                             int64_t R, double p, float iz,
                                                             float* __restrict__ out /*[R,4]*/) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_keys[];
  __shared__ SelectScratch<NT> s_sc;
  __shared__ unsigned s_sel[9];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float* prow = hist + row * ld;
  s_sc.clear_bins();
  float center, sigma_lo, sigma_up;
  int n;
  quantile_row_stats<NT, LDS>(prow, T, p, iz, s_keys, &s_sc, s_sel, center, sigma_lo, sigma_up, n);
  if (tid == 0) {
    out[row * 4 + 0] = center;
    out[row * 4 + 1] = sigma_lo;
    out[row * 4 + 2] = sigma_up;
    out[row * 4 + 3] = (float)n;
  }
}

}  // namespace

// out [R,4] fp32 = (centre, sigma_lo, sigma_up, finite count) of hist[r, :T];
// p = Phi(z0) in fp64 and inv_z0 = fp32(1 / z0) come from the host.  hist and
// ld need 4-byte alignment only.  Rows up to kRobustLdsKeys samples are
// selected in LDS, longer ones from global memory; the choice is per launch.
FM_API int fm_quantile_robust_stats(const float* hist, int64_t ld, int T, int64_t R, double p, float inv_z0,
                                    float* out, hipStream_t stream) {
  if (R <= 0) return 0;
  if (T < 0 || R > 0x7FFFFFFF || (((uintptr_t)hist) & 3) != 0 || !(p >= 0.5 && p <= 1.0) || !(inv_z0 > 0.f))
    return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)R), block(kQuantileThreads);
  if (T <= kRobustLdsKeys) {
    hipLaunchKernelGGL((quantile_robust_kernel<kQuantileThreads, true>), grid, block, row_key_bytes(T), stream, hist,
                       ld, T, R, p, inv_z0, out);
  } else {
    hipLaunchKernelGGL((quantile_robust_kernel<kQuantileThreads, false>), grid, block, 0, stream, hist, ld, T, R, p,
                       inv_z0, out);
  }
  FM_LAUNCH_CHECK();
  return 0;
}
