// K16 trend robust model: a straight line fitted to a row by Siegel's repeated
// median over the medians of its blocks, and the median / MAD band of the
// residuals about it, one 512-thread workgroup per row.
//
// The row goes into LDS and its J block medians are selected together
// (fm_radix_select.h, load_row_blocks: the front shared with K15).  Then the
// repeated median of the pair slopes of the B <= 16 block medians above the
// quorum, the inner medians one lane a block and the outer one on one lane;
// the keys rewritten in place as the keys of the residuals r_i = x_i - slope *
// (i - (T - 1)), a product and a difference each rounded to fp32 (no fused
// multiply-add: the numpy contract rounds twice); then median_sigma over the
// whole row, deviations in place as K13, whose median is the level at the last
// history sample.
//
// Block size and LDS as K15: 512 threads, up to 52 KiB of keys, 8 KiB of bins
// and 1 KiB of sort buffers, so two workgroups of a full row share a CU.  The
// contract is foremast_amd/ops/misc.py ref_trend_robust; centre, n and slope
// are exact, and sigma is where MAD > 0.
//
// Built with contraction limited to single expressions: under the library's
// -ffp-contract=fast the backend fuses the residual's product and difference
// across statements and past the pragma in detrend() (fm_repeated_median.h,
// the slope and the detrend sweep, shared with K20).
// fm-hipcc-flags: -ffp-contract=on
#include "fm_common.h"
#include "fm_repeated_median.h"

using namespace fm;

namespace {

constexpr int kTrendThreads = 512;
constexpr int kMaxBlocks = kBatchBlocks;         // foremast_amd/ops/misc.py SHIFT_MAX_BLOCKS mirrors it
static_assert(sizeof(TrendShared<kTrendThreads>) + row_key_bytes(kRobustLdsKeys) <= kLaunchLds,
              "the longest row fits a launch");

template <int NT>
__global__ __launch_bounds__(NT) void trend_robust_kernel(const float* __restrict__ hist, int64_t ld, int T, int L,
                                                          int J, int min_blocks, float* __restrict__ out /*[R,4]*/) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_keys[];
  __shared__ TrendShared<NT> s;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float* p = hist + row * ld;
  const int a = row_word(p);                                 // LDS word of key 0
  const int nq = row_quads(a, T);
  const float qnan = quiet_nan();

  // ---- the row -> keys; finite count, key range, block counts and medians
  KeyRange range;
  int n = load_row_blocks<NT>(p, T, a, L, J, s_keys, &s.sc, &s.blk, range);
  if (n == 0) {
    if (tid == 0) *reinterpret_cast<float4*>(out + row * 4) = make_float4(qnan, qnan, 0.f, 0.f);
    return;
  }

  // ---- repeated median of the pair slopes of the block medians
  int B;
  const float slope = repeated_median_slope<NT>(J, L, min_blocks, &s, B);

  // ---- the keys of the residuals in place; their finite count and key range
  RowTally res;
  detrend_keys<NT>(s_keys, nq, a, T - 1, slope, res);
  n = uniform(block_sum<NT>(res.n, s.sc.redi));
  if (n == 0) {                                              // every residual overflowed
    if (tid == 0) *reinterpret_cast<float4*>(out + row * 4) = make_float4(qnan, qnan, 0.f, slope);
    return;
  }

  // ---- median and sigma of the residuals
  float center, sigma;
  LdsRow<NT> rk{s_keys, nq};
  median_sigma(rk, (unsigned)n, block_range(res.range, &s.sc), &s.sc, center, sigma);
  if (tid == 0) *reinterpret_cast<float4*>(out + row * 4) = make_float4(center, sigma, (float)n, slope);
}

}  // namespace

// out [R,4] fp32 = (centre, sigma, finite count, slope) of hist[r, :T] under
// the trend model with J blocks of L samples (the last J * L columns) and
// min_blocks; out needs 16-byte alignment, hist and ld 4-byte alignment only.
// The row is selected in LDS: nothing is launched unless T <= kRobustLdsKeys,
// 0 <= J <= 16, J * L <= T and min_blocks >= 2.
FM_API int fm_trend_robust(const float* hist, int64_t ld, int T, int64_t R, int L, int J, int min_blocks, float* out,
                           hipStream_t stream) {
  if (T < 0 || T > kRobustLdsKeys || L < 1 || J < 0 || J > kMaxBlocks || (int64_t)J * L > T || min_blocks < 2 ||
      R > 0x7FFFFFFF || (((uintptr_t)hist) & 3) != 0 || (((uintptr_t)out) & 15) != 0)
    return (int)hipErrorInvalidValue;
  if (R <= 0) return 0;
  if (row_key_bytes(T) + sizeof(TrendShared<kTrendThreads>) > kLaunchLds) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((trend_robust_kernel<kTrendThreads>), dim3((unsigned)R), dim3(kTrendThreads), row_key_bytes(T),
                     stream, hist, ld, T, L, J, min_blocks, out);
  FM_LAUNCH_CHECK();
  return 0;
}
