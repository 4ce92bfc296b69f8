// K26 seasonal quantile robust model: K22's per-phase median profile and
// per-phase scale g', and about them a sigma per side, each calibrated on a
// tail order statistic of the signed residuals in units of their phase's
// scale; one 512-thread workgroup per row.
//
// The span stays in LDS as the keys of fm_radix_select.h from the one HBM read
// to the end.  Everything up to g' is fm_seasonal_scale.h, the code K22 runs:
// forecast, profile and sigma0 are K14's bit for bit and g' is K22's.  Then
// the keys are rewritten once more, as the order-preserving keys of v = e /
// g'[phase] (clamped to +-FLT_MAX, so that an overflow stays a finite key and
// not the missing one), and one radix_select_ranks call finds s[k_up] and
// s[k_lo], k_up = ceil(p (n - 1)), k_lo = (n - 1) - k_up: the two ranks share
// the first pass.  kappa_up = s[k_up] / z0 and kappa_lo = -s[k_lo] / z0 are
// single order statistics about the profile, nothing re-centred; a side whose
// order statistic is not > 0 takes 1.2533 times the mean of v on that side
// instead, summed in fp64 in one more sweep, which a row runs only then (a
// branch uniform over the workgroup).  sigma_up[phase] = kappa_up g'[phase],
// and likewise below.
//
// The sign of e: sigma0 and the raw scale are taken from |e|, v needs e.  The
// residual key is the bits of e with the sign in bit 31 (SignedResidual), and
// the selection of sigma0 and the sorting network of the raw scale mask that
// bit out as they read; the missing key is kept apart (e is never NaN).  The
// other way, a second read of the row from L2 to take x - profile again, needs
// the profile kept beyond the first selection, which takes its bins: m more
// words of LDS at m <= 2,048, beyond K22's budget.  It was not built.
//
// LDS is K22's to the byte: the span, g' behind it, the profile in the bins
// (behind g' when m > 2,048); the six words of the two ranks are the
// selection scratch's own reduction words, free while the ranks are selected.
// The contract is foremast_amd/ops/misc.py ref_seasonal_quantile_robust.  The
// division is correctly rounded and kappa * g' is a product on its own:
// fm-hipcc-flags: -ffp-contract=on
#include "fm_common.h"
#include "fm_quantile_row.h"   // SideTally
#include "fm_seasonal_scale.h"

using namespace fm;

namespace {

constexpr int kSqThreads = 512;
static_assert(sizeof(SelectScratch<kSqThreads>) + row_key_bytes(kRobustLdsKeys) + sizeof(uint4) <= kLaunchLds,
              "the longest span, a profile and a scale behind it fit a launch");
static_assert(kSqThreads / FM_WAVE >= 6, "the reduction words hold the selection state of two ranks");

template <int NT>
__global__ __launch_bounds__(NT) void seasonal_quantile_robust_kernel(
    const float* __restrict__ hist, int64_t ld, int T, int m, int J, int k, int w, float floor_share, double p,
    float iz, int H, float* __restrict__ forecast, float* __restrict__ sigma_lo_h, float* __restrict__ sigma_up_h,
    int64_t ldf, float* __restrict__ stats /*[R,4]*/, float* __restrict__ profile /*[R,m] or null*/,
    float* __restrict__ gscale /*[R,m] or null*/) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_keys[];
  __shared__ SelectScratch<NT> s_sc;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float qnan = quiet_nan();
  const float fmax = __uint_as_float(0x7F7FFFFFu);           // FLT_MAX

  // a row without a scale per phase: v in every phase, on both sides
  auto flat = [&](float v, float sigma0, float n) {
    for (int h = tid; h < H; h += NT) {
      sigma_lo_h[row * ldf + h] = v;
      sigma_up_h[row * ldf + h] = v;
    }
    if (gscale != nullptr)
      for (int ph = tid; ph < m; ph += NT) gscale[row * (int64_t)m + ph] = v;
    if (tid == 0) {
      stats[row * 4 + 0] = sigma0;
      stats[row * 4 + 1] = n;
      stats[row * 4 + 2] = qnan;
      stats[row * 4 + 3] = qnan;
    }
  };

  // ---- keys, profile, forecast, residual keys e, sigma0, the floored scale g' (fm_seasonal_scale.h)
  const ScaleSpan sp = seasonal_scale_stages<NT, SignedResidual>(
      hist + row * ld + (T - J * m), m, J, k, w, floor_share, H, s_keys, &s_sc, forecast + row * ldf,
      profile != nullptr ? profile + row * (int64_t)m : nullptr,
      gscale != nullptr ? gscale + row * (int64_t)m : nullptr);
  const int n = sp.n, a = sp.a, nq = sp.nq;
  const float* scl = sp.scl;                                 // [m]: g'
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

  // ---- the signed residuals in units of their phase's scale: order-preserving keys and their range
  KeyRange vr;
  sweep_phase_keys<NT>(s_keys, nq, a, m, [&](unsigned key, int ph) {
    float v = __fdiv_rn(__uint_as_float(key), scl[ph]);
    v = v > fmax ? fmax : (v < -fmax ? -fmax : v);
    const unsigned kv = enc_key(v);
    if (kv != kMissing) vr.add(kv);
    return kv;
  });
  const KeyRange range = block_range(vr, &s_sc);             // (barriers: keys visible; the bins are still zero)

  // ---- the two tail ranks, one first pass
  unsigned kup = (unsigned)ceil(p * (double)(n - 1));
  if (kup > (unsigned)(n - 1)) kup = (unsigned)(n - 1);
  const unsigned rank[2] = {kup, (unsigned)(n - 1) - kup};
  unsigned key[2], resid[2], cnt[2];
  const LdsRow<NT> rk{s_keys, nq};
  radix_select_ranks(rk, range, rank, (unsigned)n, &s_sc, s_sc.redu, key, resid, cnt);
  const float d_up = dec_key(key[0]), d_lo = -dec_key(key[1]);
  float kappa_up = __fmul_rn(d_up, iz), kappa_lo = __fmul_rn(d_lo, iz);
  if (uniform((int)(!(d_up > 0.f) || !(d_lo > 0.f)))) {        // (the same in every thread)
    SideTally t{0.f};                                        // (sums in redd and redi: the ranks' words are not written again)
    rk.sweep(t);
    const double su = block_sum<NT>(t.up, s_sc.redd), sl = block_sum<NT>(t.lo, s_sc.redd);
    const int nu = block_sum<NT>(t.nup, s_sc.redi), nl = block_sum<NT>(t.nlo, s_sc.redi);
    if (!(d_up > 0.f)) kappa_up = 1.2533f * (float)(su / (double)(nu > 0 ? nu : 1));
    if (!(d_lo > 0.f)) kappa_lo = 1.2533f * (float)(sl / (double)(nl > 0 ? nl : 1));
  }

  // ---- a sigma per side and phase, wrapped like the forecast
  write_wrapped<NT>(scl, m, H, sigma_lo_h + row * ldf, [=](float g, int) { return __fmul_rn(kappa_lo, g); });
  write_wrapped<NT>(scl, m, H, sigma_up_h + row * ldf, [=](float g, int) { return __fmul_rn(kappa_up, g); });
  if (tid == 0) {
    stats[row * 4 + 0] = sigma0;
    stats[row * 4 + 1] = (float)n;
    stats[row * 4 + 2] = kappa_lo;
    stats[row * 4 + 3] = kappa_up;
  }
}

}  // namespace

// Per row of hist[r, :T], over its last J * m samples (phase = position in
// that span mod m): fm_seasonal_scale_robust's forecast, profile, sigma0 and
// floored per-phase scale g' (k, w and floor as there), and about them
// sigma_lo_h[r, h] = kappa_lo g'[h mod m] and sigma_up_h[r, h] = kappa_up
// g'[h mod m] for h < H (the three [R, H] outputs share the leading dimension
// ldf), kappa from the ranks ceil(p (n - 1)) and its mirror of the signed
// residuals over g', times inv_z0; p = Phi(z0) in fp64 and inv_z0 = fp32(1 /
// z0) come from the host.  stats[r] = (sigma0, finite count of the span,
// kappa_lo, kappa_up); the profile and g' [R, m] when their pointers are not
// null.  hist and ld need 4-byte alignment only.  Nothing is launched unless
// fm_seasonal_scale_robust's conditions hold, 0.5 <= p <= 1 and inv_z0 > 0.
FM_API int fm_seasonal_quantile_robust(const float* hist, int64_t ld, int T, int64_t R, int m, int J, int k, int w,
                                       float floor, double p, float inv_z0, int H, float* forecast, float* sigma_lo_h,
                                       float* sigma_up_h, int64_t ldf, float* stats, float* profile, float* gscale,
                                       hipStream_t stream) {
  if (!seasonal_args_ok(hist, T, R, m, J, k, H)) return (int)hipErrorInvalidValue;
  if (w < 0 || 2 * (int64_t)w + 1 > m || !(floor > 0.f)) return (int)hipErrorInvalidValue;
  if (!(p >= 0.5 && p <= 1.0) || !(inv_z0 > 0.f)) return (int)hipErrorInvalidValue;
  if (R <= 0) return 0;
  const size_t lds = seasonal_lds_bytes(J, m, 1);                // g' behind the keys always
  if (lds + sizeof(SelectScratch<kSqThreads>) > kLaunchLds) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((seasonal_quantile_robust_kernel<kSqThreads>), dim3((unsigned)R), dim3(kSqThreads), lds, stream,
                     hist, ld, T, m, J, k, w, floor, p, inv_z0, H, forecast, sigma_lo_h, sigma_up_h, ldf, stats, profile,
                     gscale);
  FM_LAUNCH_CHECK();
  return 0;
}
