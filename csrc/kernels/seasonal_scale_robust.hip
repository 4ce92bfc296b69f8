// K22 seasonal scale robust model: K14's per-phase median profile of the last
// J whole cycles of a row, and about it a sigma per phase instead of one MAD,
// one 512-thread workgroup per row.
//
// The span stays in LDS as the keys of fm_radix_select.h from the one HBM read
// to the end.  Profile, smoothing, forecast and the residual keys |x -
// profile[phase]| are K14's stages (fm_seasonal_profile.h, one text for K14,
// K20 and this kernel), and the first radix selection gives K14's sigma,
// sigma0.  Then the raw scale of a phase is
// the middle of its J residual keys by the same register sorting network
// (non-negative floats order as their bits, the missing key last); it is
// smoothed over w phases each side, circular, with fp64 sums, and floored at
// floor * sigma0 / 1.4826.  All of that is fm_seasonal_scale.h, which K26
// (seasonal_quantile_robust.hip) runs too.  The keys are rewritten once more, as the bits of
// u = r / scale[phase], and a second radix selection finds kappa = 1.4826
// middle(u): sigma[phase] = kappa * scale[phase].
//
// LDS: the profile buffer is the selection's bin array while m <= 2,048, as in
// K14.  The scale buffer is read while the keys are rewritten for a selection
// that needs the bins right after, so it sits behind the keys always, and a
// longer period puts the profile behind it: (J + 2) m <= kRobustLdsKeys
// (ops/misc.py seasonal_cycles) holds the span and both.  At 7 x 1,440 a
// workgroup takes 54,432 B against K14's 48,672 B: by bytes three still fit
// the 160 KiB of a CU, with 544 to spare, but the timings on either side of
// that edge say only two are resident (docs/PERF.md).  The contract is foremast_amd/ops/misc.py ref_seasonal_scale_robust;
// forecast, profile and sigma0 are K14's bit for bit, and given the profile the
// scale is exact up to kappa, which is exact where the middle of u is > 0.
#include "fm_common.h"
#include "fm_seasonal_scale.h"

using namespace fm;

namespace {

constexpr int kScaleThreads = 512;
static_assert(sizeof(SelectScratch<kScaleThreads>) + row_key_bytes(kRobustLdsKeys) + sizeof(uint4) <= kLaunchLds,
              "the longest span, a profile and a scale behind it fit a launch");

template <int NT>
__global__ __launch_bounds__(NT) void seasonal_scale_robust_kernel(const float* __restrict__ hist, int64_t ld, int T,
                                                                   int m, int J, int k, int w, float floor_share,
                                                                   int H, float* __restrict__ forecast,
                                                                   float* __restrict__ sigma_h, int64_t ldf,
                                                                   float* __restrict__ stats /*[R,3]*/,
                                                                   float* __restrict__ profile /*[R,m] or null*/,
                                                                   float* __restrict__ scale /*[R,m] or null*/) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_keys[];
  __shared__ SelectScratch<NT> s_sc;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float qnan = quiet_nan();

  // a row without a sigma per phase: v in every phase
  auto flat = [&](float v, float sigma0, float n) {
    for (int h = tid; h < H; h += NT) sigma_h[row * ldf + h] = v;
    if (scale != nullptr)
      for (int ph = tid; ph < m; ph += NT) scale[row * (int64_t)m + ph] = v;
    if (tid == 0) {
      stats[row * 3 + 0] = sigma0;
      stats[row * 3 + 1] = n;
      stats[row * 3 + 2] = qnan;
    }
  };

  // ---- keys, profile, forecast, residual keys |e|, sigma0, the floored scale g' (fm_seasonal_scale.h)
  const ScaleSpan sp = seasonal_scale_stages<NT, AbsResidual>(
      hist + row * ld + (T - J * m), m, J, k, w, floor_share, H, s_keys, &s_sc, forecast + row * ldf,
      profile != nullptr ? profile + row * (int64_t)m : nullptr, nullptr);
  const int n = sp.n, a = sp.a, nq = sp.nq;
  float* scl = sp.scl;                                       // [m]: floored scale, then sigma per phase
  if (n == 0) {
    for (int h = tid; h < H; h += NT) forecast[row * ldf + h] = qnan;
    if (profile != nullptr)
      for (int ph = tid; ph < m; ph += NT) profile[row * (int64_t)m + ph] = qnan;
    flat(qnan, qnan, 0.f);
    return;
  }
  const float sigma0 = sp.sigma0;
  if (sigma0 == 0.f) {                                       // a perfectly periodic span
    flat(0.f, 0.f, (float)n);
    return;
  }
  const LdsRow<NT> rk{s_keys, nq};

  // ---- the residuals in units of their phase's scale: keys, fp64 sum, range
  DevTally rel;
  sweep_phase_keys<NT>(s_keys, nq, a, m, [&](unsigned key, int ph) {
    const unsigned u = __float_as_uint(__fdiv_rn(__uint_as_float(key), scl[ph]));
    rel(u);
    return u;
  });
  const double sum_u = uniform(block_sum<NT>(rel.sum, s_sc.redd));   // (barriers: keys visible; the bins are still zero)

  // ---- kappa: sigma's rule over u
  const float kappa = mad_sigma(rk, (unsigned)n, sum_u, rel.range, &s_sc);

  // ---- sigma per phase, in place (a thread rewrites the phases it reads), and wrapped like the forecast
  for (int ph = tid; ph < m; ph += NT) {
    const float s = __fmul_rn(kappa, scl[ph]);
    scl[ph] = s;
    if (scale != nullptr) scale[row * (int64_t)m + ph] = s;
  }
  __syncthreads();
  write_wrapped<NT>(scl, m, H, sigma_h + row * ldf);
  if (tid == 0) {
    stats[row * 3 + 0] = sigma0;
    stats[row * 3 + 1] = (float)n;
    stats[row * 3 + 2] = kappa;
  }
}

}  // namespace

// Per row of hist[r, :T], over its last J * m samples (phase = position in
// that span mod m): fm_seasonal_robust's smoothed per-phase median profile and
// forecast[r, h] = profile[h mod m]; the per-phase middle of the residuals
// about the profile, smoothed over w phases each side, floored at floor *
// sigma0 / 1.4826 and scaled by kappa (1.4826 times the middle of the
// residuals over that scale): sigma_h[r, h] = scale[h mod m] for h < H
// (forecast and sigma_h share the leading dimension ldf); stats[r] = (sigma0 =
// fm_seasonal_robust's sigma, finite count of the span, kappa); the profile and
// the scale [R, m] when their pointers are not null.  k and w = half widths of
// the two smoothing windows.  hist and ld need 4-byte alignment only.  Nothing
// is launched unless 2 <= J <= 16, J * m <= T, (J + 2) * m fits the LDS budget
// of K13, 2 k + 1 <= m, 0 <= w, 2 w + 1 <= m and floor > 0.
FM_API int fm_seasonal_scale_robust(const float* hist, int64_t ld, int T, int64_t R, int m, int J, int k, int w,
                                    float floor, int H, float* forecast, float* sigma_h, int64_t ldf, float* stats,
                                    float* profile, float* scale, hipStream_t stream) {
  if (!seasonal_args_ok(hist, T, R, m, J, k, H)) return (int)hipErrorInvalidValue;
  if (w < 0 || 2 * (int64_t)w + 1 > m || !(floor > 0.f)) return (int)hipErrorInvalidValue;
  if (R <= 0) return 0;
  const size_t lds = seasonal_lds_bytes(J, m, 1);                // the scale behind the keys always
  if (lds + sizeof(SelectScratch<kScaleThreads>) > kLaunchLds) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((seasonal_scale_robust_kernel<kScaleThreads>), dim3((unsigned)R), dim3(kScaleThreads), lds,
                     stream, hist, ld, T, m, J, k, w, floor, H, forecast, sigma_h, ldf, stats, profile, scale);
  FM_LAUNCH_CHECK();
  return 0;
}
