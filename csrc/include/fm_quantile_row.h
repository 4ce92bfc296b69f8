// Median and one sigma per side of one history row by a workgroup (K24's row
// computation), shared by quantile_robust.hip (K24) and band_stats.hip (K25):
// the same device functions at the same thread count give the same bits in
// every kernel that calls them.
#pragma once
#include "fm_common.h"
#include "fm_radix_select.h"

namespace fm {

// One-sided deviations about the centre: what the fallback of a side sums.
struct SideTally {
  float c;
  double up = 0.0, lo = 0.0;
  int nup = 0, nlo = 0;
  __device__ __forceinline__ void operator()(unsigned k) {
    if (k != kMissing) {
      const float x = dec_key(k);
      if (x >= c) {
        up += (double)(x - c);
        ++nup;
      }
      if (x <= c) {
        lo += (double)(c - x);
        ++nlo;
      }
    }
  }
};

// (centre, sigma_lo, sigma_up) of the n >= 1 finite keys of rk, all within r;
// the same in every thread.
template <int NT, class Keys>
__device__ __forceinline__ void quantile_sigmas(const Keys& rk, unsigned n, KeyRange r, double p, float iz,
                                                SelectScratch<NT>* sc, unsigned* sel, float& center, float& sigma_lo,
                                                float& sigma_up) {
  unsigned kup = (unsigned)ceil(p * (double)(n - 1u));
  if (kup > n - 1u) kup = n - 1u;
  const unsigned rank[3] = {(n - 1u) >> 1, kup, (n - 1u) - kup};
  unsigned key[3], resid[3], cnt[3];
  radix_select_ranks(rk, r, rank, n, sc, sel, key, resid, cnt);
  center = mid_value(key[0], upper_middle(rk, key[0], n, resid[0], cnt[0], sc));
  const float d_up = dec_key(key[1]) - center, d_lo = center - dec_key(key[2]);
  sigma_up = d_up * iz;
  sigma_lo = d_lo * iz;
  if (uniform((int)(!(d_up > 0.f) || !(d_lo > 0.f)))) {        // (the same in every thread)
    SideTally t{center};
    rk.sweep(t);
    const double su = block_sum<NT>(t.up, sc->redd), sl = block_sum<NT>(t.lo, sc->redd);
    const int nu = block_sum<NT>(t.nup, sc->redi), nl = block_sum<NT>(t.nlo, sc->redi);
    if (!(d_up > 0.f)) sigma_up = 1.2533f * (float)(su / (double)(nu > 0 ? nu : 1));
    if (!(d_lo > 0.f)) sigma_lo = 1.2533f * (float)(sl / (double)(nl > 0 ? nl : 1));
  }
}

// K24's statistics of p[0..T): (centre, sigma_lo, sigma_up) and the finite
// count, NaN for a row without a finite sample.  The bins are zero on entry and
// on return; keys holds row_key_bytes(T) when LDS; sel is LDS, 9 words.  Every
// thread of the workgroup calls it, and all branches around barriers are
// workgroup-uniform.
template <int NT, bool LDS>
__device__ __forceinline__ void quantile_row_stats(const float* __restrict__ prow, int T, double p, float iz,
                                                   uint4* keys, SelectScratch<NT>* sc, unsigned* sel, float& center,
                                                   float& sigma_lo, float& sigma_up, int& n) {
  center = sigma_lo = sigma_up = quiet_nan();
  RowTally t;
  if constexpr (LDS) {
    const int a = row_word(prow);
    load_row_keys<NT>(prow, T, a, keys, t);
    n = uniform(block_sum<NT>(t.n, sc->redi));                // (barriers: keys and bins visible)
    if (n != 0) {                                             // (the same in every thread)
      LdsRow<NT> rk{keys, row_quads(a, T)};
      quantile_sigmas(rk, (unsigned)n, block_range(t.range, sc), p, iz, sc, sel, center, sigma_lo, sigma_up);
    }
  } else {
    GlobalRow<NT> rk{prow, T};
    rk.sweep(t);
    n = uniform(block_sum<NT>(t.n, sc->redi));
    if (n != 0)
      quantile_sigmas(rk, (unsigned)n, block_range(t.range, sc), p, iz, sc, sel, center, sigma_lo, sigma_up);
  }
}

}  // namespace fm
