// Median / MAD statistics of one history row by a workgroup (K13's row
// computation), shared by robust_stats.hip (K13, K18) and band_stats.hip
// (K25): the same device functions at the same thread count give the same
// bits in every kernel that calls them.
#pragma once
#include "fm_common.h"
#include "fm_radix_select.h"

namespace fm {

// (centre, sigma, finite count) of the keys rk makes of a row, tallied into t
// on the way; the same in every thread.
template <int NT, class Keys>
__device__ __forceinline__ void tallied_stats(Keys& rk, const RowTally& t, SelectScratch<NT>* sc, float& center,
                                              float& sigma, int& nfin) {
  nfin = uniform(block_sum<NT>(t.n, sc->redi));               // (barriers: keys and bins visible)
  if (nfin == 0) {                                            // (the same in every thread)
    center = sigma = quiet_nan();
    return;
  }
  median_sigma(rk, (unsigned)nfin, block_range(t.range, sc), sc, center, sigma);
}

// The statistics of p[0..T).  The bins are zero on entry and on return; keys
// holds row_key_bytes(T) when LDS.  Every thread of the workgroup calls it; all
// branches around barriers are workgroup-uniform, so it can be called for one
// row after another: the last reads of keys and scratch sit in front of a
// barrier that every thread passes before the next row's first write to them.
template <int NT, bool LDS>
__device__ __forceinline__ void robust_row_stats(const float* __restrict__ p, int T, uint4* keys,
                                                 SelectScratch<NT>* sc, float& center, float& sigma, int& nfin) {
  RowTally t;
  if constexpr (LDS) {
    const int a = row_word(p);
    load_row_keys<NT>(p, T, a, keys, t);
    LdsRow<NT> rk{keys, row_quads(a, T)};
    tallied_stats(rk, t, sc, center, sigma, nfin);
  } else {
    GlobalRow<NT> rk{p, T};
    rk.sweep(t);
    tallied_stats(rk, t, sc, center, sigma, nfin);
  }
}

}  // namespace fm
