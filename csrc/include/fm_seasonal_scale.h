// The stages of the seasonal kernels with a scale per phase, up to the floored
// scale g', stated here only: K22 (seasonal_scale_robust.hip) and K26
// (seasonal_quantile_robust.hip), whose forecast, profile, sigma0 and g' are
// the same bit for bit because they are this code.
//
// The span becomes keys in LDS, K14's profile is made, smoothed and written
// out as the forecast (fm_seasonal_profile.h), the keys become the residuals
// about the profile, the first radix selection gives K14's sigma, sigma0, the
// raw scale of a phase is the middle of the magnitudes of its J residuals, and
// it is smoothed over w phases each side and floored at floor * sigma0 /
// 1.4826.
//
// What a residual key holds is the caller's choice.  K22 needs |e| only: the
// key is its bits, as dev_key makes it.  K26 needs the sign of e again after
// sigma0 and the raw scale were taken from |e|, so its key is the bits of e
// itself, the sign in bit 31, and every reader of a magnitude masks that bit
// out on the way (the missing key stays what it is: e is never NaN, so no
// residual has its bits).  With AbsResidual the mask is the identity and the
// code is K22's as it was.
#pragma once
#include "fm_seasonal_profile.h"

namespace fm {

// residual key of the sample with the (finite) key k about the centre c, and
// the magnitude key of a residual key
struct AbsResidual {
  static __device__ __forceinline__ unsigned key(unsigned k, float c) { return dev_key(k, c); }
  static __device__ __forceinline__ unsigned mag(unsigned k) { return k; }
};
struct SignedResidual {
  static __device__ __forceinline__ unsigned key(unsigned k, float c) { return __float_as_uint(dec_key(k) - c); }
  static __device__ __forceinline__ unsigned mag(unsigned k) { return k == kMissing ? kMissing : (k & 0x7FFFFFFFu); }
};

// LdsRow whose sweep yields the magnitudes of the residual keys
template <int NT, class Res>
struct ResidualRow {
  const uint4* k4;
  int nq;
  template <class F>
  __device__ __forceinline__ void sweep(F&& f) const {
    for (int q = threadIdx.x; q < nq; q += NT) {
      const uint4 v = k4[q];
      f(Res::mag(v.x)); f(Res::mag(v.y)); f(Res::mag(v.z)); f(Res::mag(v.w));
    }
  }
};

// Where the stages left the row: key 0 at word a of nq quads, n finite
// samples, sigma0, and the per-phase buffer behind the keys.
struct ScaleSpan {
  int a, nq, n;
  float sigma0;
  float* scl;                    // [m]: g' when n != 0 and sigma0 != 0
};

// The span p[0..J m) of one row by a workgroup of NT threads: forecast[0..H)
// and profile[0..m) (when not null) are written unless n == 0; on return with
// n != 0 and sigma0 != 0 the keys are the residual keys of Res, scl holds g'
// (also written to gscale[0..m) when not null), both visible, and the bins
// are zero.  With n == 0 or sigma0 == 0 the caller writes what is left; the
// return value is the same in every thread.
template <int NT, class Res>
__device__ __forceinline__ ScaleSpan seasonal_scale_stages(const float* __restrict__ p, int m, int J, int k, int w,
                                                           float floor_share, int H, uint4* s_keys,
                                                           SelectScratch<NT>* sc, float* __restrict__ forecast,
                                                           float* __restrict__ profile, float* __restrict__ gscale) {
  const int N = J * m;                                       // span length
  ScaleSpan sp;
  sp.a = row_word(p);                                        // LDS word of key 0
  sp.nq = row_quads(sp.a, N);
  sp.sigma0 = quiet_nan();
  const int a = sp.a, nq = sp.nq;
  unsigned* kw = reinterpret_cast<unsigned*>(s_keys);
  float* scl = reinterpret_cast<float*>(kw + 4 * nq);        // [m]: raw scale, then g'
  float* prof = m <= kBins ? reinterpret_cast<float*>(sc->bins) : scl + m;   // [m]: raw, then smoothed
  sp.scl = scl;

  // ---- the span -> keys in place; finite count (the key range is not needed)
  int n = 0;
  auto count = [&](unsigned key) { n += key != kMissing; };
  load_row_keys<NT>(p, N, a, s_keys, count);
  n = uniform(block_sum<NT>(n, sc->redi));                   // (barriers: keys visible)
  sp.n = n;
  if (n == 0) return sp;

  // ---- raw profile: per-phase median of the finite samples
  phase_values<NT>(kw + a, m, J, prof, SampleKey{});
  __syncthreads();

  // ---- smoothing in place: mean of the finite raw values within k phases, circular
  smooth_in_place<NT>(prof, m, k, [&](int ph, float v) {
    if (profile != nullptr) profile[ph] = v;
    return v;
  });

  // ---- forecast: the profile from phase 0 on, wrapped
  write_wrapped<NT>(prof, m, H, forecast);

  // ---- residuals about the profile: keys, fp64 sum and range of their magnitudes
  DevTally dev;
  sweep_phase_keys<NT>(s_keys, nq, a, m, [&](unsigned key, int ph) {
    const unsigned d = Res::key(key, prof[ph]);
    dev(Res::mag(d));
    return d;
  });
  const double sum = uniform(block_sum<NT>(dev.sum, sc->redd));    // (barriers: the last read of the profile is behind)
  sc->clear_bins();                                          // (made visible by the barriers of mad_sigma's range)

  // ---- sigma0, K14's sigma: the padding words hold the missing key, so the span is swept as a whole row
  const ResidualRow<NT, Res> rk{s_keys, nq};
  sp.sigma0 = mad_sigma(rk, (unsigned)n, sum, dev.range, sc);
  if (sp.sigma0 == 0.f) return sp;                           // a perfectly periodic span (uniform: every thread read the same middles)

  // ---- raw scale: per-phase middle of the residuals' magnitudes (non-negative floats order as their bits)
  phase_values<NT>(kw + a, m, J, scl, DeviationKey{}, [](unsigned key) { return Res::mag(key); });
  __syncthreads();

  // ---- smoothing in place over w phases each side, then the floor
  const float f = __fmul_rn(floor_share, __fdiv_rn(sp.sigma0, 1.4826f));
  smooth_in_place<NT>(scl, m, w, [&](int ph, float v) {
    const float g = v == v ? fmaxf(v, f) : f;
    if (gscale != nullptr) gscale[ph] = g;
    return g;
  });
  return sp;
}

}  // namespace fm
