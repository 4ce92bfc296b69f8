// K20 seasonal trend robust model: a straight line through the medians of the
// last J whole cycles of a row (Siegel's repeated median, as K16), and about
// that line a per-phase median profile and the MAD of the residuals (as K14),
// one 512-thread workgroup per row.
//
// The span (the last J * m columns) is read from HBM once and stays in LDS as
// the keys of fm_radix_select.h.  load_row_blocks selects the J cycle medians
// together: a block is a whole cycle, so a cycle of any shape moves every
// block median alike and does not bias the slope.  The keys are then rewritten
// in place as the keys of the residuals r_i = x_i - slope * (i - (N - 1)), a
// product and a difference each rounded to fp32; the profile of the residuals
// therefore carries the level at the last history sample plus the cycle, and
// forecast[h - 1] = profile[(h - 1) mod m] + slope * h (rounded twice too).
// From there on it is K14: per-phase register sort, circular smoothing with
// fp64 sums, deviations in place, one radix selection for the MAD.  The slope
// stage is fm_repeated_median.h's, which K16 runs too, and the per-phase
// stages are fm_seasonal_profile.h's, which K14 and K22 run: with slope 0 this
// kernel is K14 because it is the same code.
//
// LDS as K14: the profile buffer is the selection's bin array while m <= 2,048
// (load_row_blocks hands the bins back zeroed, and they are cleared after the
// last read of the profile), else it sits behind the keys; the shared struct
// is K16's.  The contract is foremast_amd/ops/misc.py
// ref_seasonal_trend_robust; n, slope and nblocks are exact, the profile is
// with k = 0, and sigma is given the profile where MAD > 0.
//
// Built with contraction limited to single expressions, as K16 (the reason is
// at the top of fm_repeated_median.h).
// fm-hipcc-flags: -ffp-contract=on
#include "fm_common.h"
#include "fm_repeated_median.h"
#include "fm_seasonal_profile.h"

using namespace fm;

namespace {

constexpr int kStThreads = 512;
// (J + 2) m <= kRobustLdsKeys: the span and a profile behind it are no longer than the longest row
static_assert(sizeof(TrendShared<kStThreads>) + row_key_bytes(kRobustLdsKeys) <= kLaunchLds,
              "the longest span and a profile behind it fit a launch");

template <int NT>
__global__ __launch_bounds__(NT) void seasonal_trend_robust_kernel(const float* __restrict__ hist, int64_t ld, int T,
                                                                   int m, int J, int k, int min_blocks, int H,
                                                                   float* __restrict__ forecast, int64_t ldf,
                                                                   float* __restrict__ stats /*[R,4]*/,
                                                                   float* __restrict__ profile /*[R,m] or null*/) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_keys[];
  __shared__ TrendShared<NT> s;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int N = J * m;                                       // span length
  const float* p = hist + row * ld + (T - N);
  const int a = row_word(p);                                 // LDS word of key 0
  const int nq = row_quads(a, N);
  unsigned* kw = reinterpret_cast<unsigned*>(s_keys);
  float* prof = reinterpret_cast<float*>(m <= kBins ? s.sc.bins : kw + 4 * nq);   // [m]: raw, then smoothed
  const float qnan = quiet_nan();

  // a row without a finite residual: NaN forecast, profile and sigma
  auto empty = [&](float slope, float nblocks) {
    for (int h = tid; h < H; h += NT) forecast[row * ldf + h] = qnan;
    if (profile != nullptr)
      for (int ph = tid; ph < m; ph += NT) profile[row * (int64_t)m + ph] = qnan;
    if (tid == 0) *reinterpret_cast<float4*>(stats + row * 4) = make_float4(qnan, 0.f, slope, nblocks);
  };

  // ---- the span -> keys; finite count, key range, cycle counts and medians
  KeyRange range;
  int n = load_row_blocks<NT>(p, N, a, m, J, s_keys, &s.sc, &s.blk, range);
  if (n == 0) {
    empty(0.f, 0.f);
    return;
  }

  // ---- repeated median of the pair slopes of the cycle medians
  int B;
  const float slope = repeated_median_slope<NT>(J, m, min_blocks, &s, B);

  // ---- the keys of the residuals in place; their finite count
  n = 0;
  auto count = [&](unsigned key) { n += key != kMissing; };
  detrend_keys<NT>(s_keys, nq, a, N - 1, slope, count);
  n = uniform(block_sum<NT>(n, s.sc.redi));                  // (barriers: residual keys visible)
  if (n == 0) {                                              // every residual overflowed
    empty(slope, (float)B);
    return;
  }

  // ---- raw profile: per-phase median of the finite residuals
  phase_values<NT>(kw + a, m, J, prof, SampleKey{});
  __syncthreads();

  // ---- smoothing in place: mean of the finite raw values within k phases, circular
  smooth_in_place<NT>(prof, m, k, [&](int ph, float v) {
    if (profile != nullptr) profile[row * (int64_t)m + ph] = v;
    return v;
  });

  // ---- forecast: the profile from phase 0 on, wrapped, plus the line from the last sample on
  write_wrapped<NT>(prof, m, H, forecast + row * ldf,
                    [&](float v, int h) { return __fadd_rn(v, __fmul_rn(slope, (float)(h + 1))); });

  // ---- deviations of the residuals about the profile: keys, fp64 sum, range
  DevTally dev;
  sweep_phase_keys<NT>(s_keys, nq, a, m, [&](unsigned key, int ph) {
    const unsigned d = dev_key(key, prof[ph]);
    dev(d);
    return d;
  });
  const double sum = uniform(block_sum<NT>(dev.sum, s.sc.redd));   // (barriers: the last read of the profile is behind)
  s.sc.clear_bins();                                         // (made visible by the barriers of mad_sigma's range)

  // ---- MAD: the padding words hold the missing key, so the span is swept as a whole row
  const LdsRow<NT> rk{s_keys, nq};
  const float sigma = mad_sigma(rk, (unsigned)n, sum, dev.range, &s.sc);
  if (tid == 0) *reinterpret_cast<float4*>(stats + row * 4) = make_float4(sigma, (float)n, slope, (float)B);
}

}  // namespace

// Per row of hist[r, :T], over its last J * m samples: the repeated-median
// slope of the J cycle medians (0 with fewer than min_blocks non-empty cycles),
// the smoothed per-phase median profile of the residuals about that line
// anchored at the last sample, forecast[r, h] = profile[h mod m] + slope *
// (h + 1) for h < H (leading dimension ldf), stats[r] = (sigma, finite count
// of the residuals, slope, non-empty cycles), and the profile [R, m] when its
// pointer is not null.  k = half width of the smoothing window.  stats needs
// 16-byte alignment, hist and ld 4-byte alignment only.  Nothing is launched
// unless 2 <= J <= 16, J * m <= T, (J + 2) * m fits the LDS budget of K13,
// 2 k + 1 <= m and min_blocks >= 2.
FM_API int fm_seasonal_trend_robust(const float* hist, int64_t ld, int T, int64_t R, int m, int J, int k,
                                    int min_blocks, int H, float* forecast, int64_t ldf, float* stats, float* profile,
                                    hipStream_t stream) {
  if (!seasonal_args_ok(hist, T, R, m, J, k, H) || min_blocks < 2 || (((uintptr_t)stats) & 15) != 0)
    return (int)hipErrorInvalidValue;
  if (R <= 0) return 0;
  const size_t lds = seasonal_lds_bytes(J, m, 0);
  if (lds + sizeof(TrendShared<kStThreads>) > kLaunchLds) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((seasonal_trend_robust_kernel<kStThreads>), dim3((unsigned)R), dim3(kStThreads), lds, stream,
                     hist, ld, T, m, J, k, min_blocks, H, forecast, ldf, stats, profile);
  FM_LAUNCH_CHECK();
  return 0;
}
