// K14 seasonal robust model: a per-phase median profile of the last J whole
// cycles of a row, smoothed over neighbouring phases, and the MAD of the
// residuals about it, one 512-thread workgroup per row.
//
// The span (the last J * m columns of the row) is read from HBM once into LDS
// as the keys of fm_radix_select.h, key i at word a + i (load_row_keys): a
// phase is a position.
//
// The stages are fm_seasonal_profile.h's, which K20 and K22 run too.  Raw
// profile: a thread takes phases p, p + 512, ...; the J keys of a phase sit m
// words apart (adjacent lanes read adjacent words), are sorted in registers
// with the missing key last, and the two middles of the finite ones are
// averaged (K13's median rule).  Smoothing: the mean of the finite raw values
// within k phases, circular, summed and divided in fp64, in the same m-word
// buffer.  Then the keys are overwritten with the bits of |x -
// profile[phase]|, summed in fp64, and one radix selection finds their middle:
// the MAD, with no re-centring.
//
// The profile buffer is the selection's bin array while m <= 2,048 (the bins
// are not in use before the selection and are cleared after the last read of
// the profile), so at the 7 x 1,440 workload a workgroup takes the LDS of a
// K13 workgroup and three of them share a CU; a longer period puts it behind
// the keys.  The contract is foremast_amd/ops/misc.py ref_seasonal_robust;
// with k = 0 the profile is exact, and sigma is exact given the profile where
// MAD > 0.
#include "fm_common.h"
#include "fm_seasonal_profile.h"

using namespace fm;

namespace {

constexpr int kSeasonalThreads = 512;
static_assert(sizeof(SelectScratch<kSeasonalThreads>) + row_key_bytes(kRobustLdsKeys) <= kLaunchLds,
              "the longest span and a profile behind it fit a launch");

template <int NT>
__global__ __launch_bounds__(NT) void seasonal_robust_kernel(const float* __restrict__ hist, int64_t ld, int T,
                                                             int m, int J, int k, int H,
                                                             float* __restrict__ forecast, int64_t ldf,
                                                             float* __restrict__ stats /*[R,2]*/,
                                                             float* __restrict__ profile /*[R,m] or null*/) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_keys[];
  __shared__ SelectScratch<NT> s_sc;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int N = J * m;                                       // span length
  const float* p = hist + row * ld + (T - N);
  const int a = row_word(p);                                 // LDS word of key 0
  const int nq = row_quads(a, N);
  unsigned* kw = reinterpret_cast<unsigned*>(s_keys);
  float* prof = reinterpret_cast<float*>(m <= kBins ? s_sc.bins : kw + 4 * nq);   // [m]: raw, then smoothed

  // ---- the span -> keys in place; finite count (the key range is not needed)
  int n = 0;
  auto count = [&](unsigned k) { n += k != kMissing; };
  load_row_keys<NT>(p, N, a, s_keys, count);
  n = uniform(block_sum<NT>(n, s_sc.redi));                  // (barriers: keys visible)
  const float qnan = quiet_nan();
  if (n == 0) {
    for (int h = tid; h < H; h += NT) forecast[row * ldf + h] = qnan;
    if (profile != nullptr)
      for (int ph = tid; ph < m; ph += NT) profile[row * (int64_t)m + ph] = qnan;
    if (tid == 0) {
      stats[row * 2 + 0] = qnan;
      stats[row * 2 + 1] = 0.f;
    }
    return;
  }

  // ---- raw profile: per-phase median of the finite samples
  phase_values<NT>(kw + a, m, J, prof, SampleKey{});
  __syncthreads();

  // ---- smoothing in place: mean of the finite raw values within k phases, circular
  smooth_in_place<NT>(prof, m, k, [&](int ph, float v) {
    if (profile != nullptr) profile[row * (int64_t)m + ph] = v;
    return v;
  });

  // ---- forecast: the profile from phase 0 on, wrapped
  write_wrapped<NT>(prof, m, H, forecast + row * ldf);

  // ---- residuals about the profile: keys, fp64 sum, range
  DevTally dev;
  sweep_phase_keys<NT>(s_keys, nq, a, m, [&](unsigned key, int ph) {
    const unsigned d = dev_key(key, prof[ph]);
    dev(d);
    return d;
  });
  const double sum = uniform(block_sum<NT>(dev.sum, s_sc.redd));   // (barriers: the last read of the profile is behind)
  s_sc.clear_bins();                                         // (made visible by the barriers of mad_sigma's range)

  // ---- MAD: the padding words hold the missing key, so the span is swept as a whole row
  const LdsRow<NT> rk{s_keys, nq};
  const float sigma = mad_sigma(rk, (unsigned)n, sum, dev.range, &s_sc);
  if (tid == 0) {
    stats[row * 2 + 0] = sigma;
    stats[row * 2 + 1] = (float)n;
  }
}

}  // namespace

// Per row of hist[r, :T]: the smoothed per-phase median profile of its last
// J * m samples (phase = position in that span mod m), forecast[r, h] =
// profile[h mod m] for h < H (leading dimension ldf), stats[r] = (sigma,
// finite count of the span), and the profile [R, m] when its pointer is not
// null.  k = half width of the smoothing window.  hist and ld need 4-byte
// alignment only.  Nothing is launched unless 2 <= J <= 16, J * m <= T,
// (J + 2) * m fits the LDS budget of K13 and 2 k + 1 <= m.
FM_API int fm_seasonal_robust(const float* hist, int64_t ld, int T, int64_t R, int m, int J, int k, int H,
                              float* forecast, int64_t ldf, float* stats, float* profile, hipStream_t stream) {
  if (!seasonal_args_ok(hist, T, R, m, J, k, H)) return (int)hipErrorInvalidValue;
  if (R <= 0) return 0;
  const size_t lds = seasonal_lds_bytes(J, m, 0);
  if (lds + sizeof(SelectScratch<kSeasonalThreads>) > kLaunchLds) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((seasonal_robust_kernel<kSeasonalThreads>), dim3((unsigned)R), dim3(kSeasonalThreads), lds, stream,
                     hist, ld, T, m, J, k, H, forecast, ldf, stats, profile);
  FM_LAUNCH_CHECK();
  return 0;
}
