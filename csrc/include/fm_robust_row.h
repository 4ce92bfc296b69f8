// Median / MAD statistics of one history row by a whole workgroup: the row
// computation of K13 (robust_stats.hip: one row per workgroup) and K18 (the
// cached, row-mapped form: a workgroup handles several rows in turn).
//
// The row is read once (16-B loads after a peeled head, so it needs 4-byte
// alignment only) and kept in LDS as the order-preserving keys of
// fm_radix_select.h; the median is selected, the keys are overwritten with the
// bits of |x - centre|, summed in fp64 and selected again.  Rows longer than
// kRobustLdsKeys run the same passes re-reading global memory (LDS = false).
// The contract is foremast_amd/ops/misc.py ref_robust_stats.
#pragma once
#include "fm_common.h"
#include "fm_radix_select.h"

namespace fm {

// LDS scratch of one workgroup besides the keys and the bins
template <int NT>
struct RobustScratch {
  unsigned sel[3];
  unsigned redu[NT / FM_WAVE];
  int redi[NT / FM_WAVE];
  double redd[NT / FM_WAVE];
};

// (centre, sigma, finite count) of p[0..T), the same in every thread.
// bins[kBins] is zero on entry (made visible by the barriers of the first
// reduction) and on return; keys holds (T + 3) / 4 uint4 when LDS.  Every
// thread of the workgroup calls it; all branches around barriers are
// workgroup-uniform, so it can be called for one row after another: the last
// reads of keys, bins and scratch sit in front of a barrier that every thread
// passes before the next row's first write to them.
template <int NT, bool LDS>
__device__ __forceinline__ void robust_row_stats(const float* __restrict__ p, int T, uint4* keys, unsigned* bins,
                                                 RobustScratch<NT>* sc, float& center, float& sigma, int& nfin) {
  const int tid = threadIdx.x;
  RowKeys<NT, LDS> rk{p, T, keys, (T + 3) >> 2, false, 0.f};

  // ---- the row -> keys; finite count and key range
  int n = 0;
  unsigned kmin = kMissing, kmax = 0u;
  auto track = [&](unsigned k) {
    if (k != kMissing) {
      ++n;
      kmin = k < kmin ? k : kmin;
      kmax = k > kmax ? k : kmax;
    }
  };
  if constexpr (LDS) {
    int head = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);   // elements before the 16-B boundary
    if (head > T) head = T;
    const int nb = (T - head) >> 2, edge = T - 4 * nb;                        // edge = head + tail elements, < 7
    const float4* b4 = reinterpret_cast<const float4*>(p + head);
    for (int q = tid; q < nb; q += NT) {
      const float4 x = b4[q];
      const uint4 k = make_uint4(enc_key(x.x), enc_key(x.y), enc_key(x.z), enc_key(x.w));
      track(k.x); track(k.y); track(k.z); track(k.w);
      keys[q] = k;
    }
    if (tid < 4 * (rk.nq - nb)) {                                             // head, tail, padding to whole quads
      unsigned k = kMissing;
      if (tid < edge) k = enc_key(p[tid < head ? tid : 4 * nb + tid]);
      track(k);
      reinterpret_cast<unsigned*>(keys)[4 * nb + tid] = k;
    }
  } else {
    rk.sweep(track);
  }
  n = block_sum<NT>(n, sc->redi);                                             // (barriers: keys and bins visible)
  nfin = n;
  if (n == 0) {                                                               // (the same in every thread)
    center = sigma = __uint_as_float(0x7FC00000u);
    return;
  }
  kmin = block_min_u32<NT>(kmin, sc->redu);
  kmax = ~block_min_u32<NT>(~kmax, sc->redu);

  // ---- median
  unsigned klo, kup;
  select_middles<NT, LDS>(rk, kmin, kmax, (unsigned)n, bins, sc->sel, sc->redu, klo, kup);
  center = 0.5f * dec_key(klo) + 0.5f * dec_key(kup);

  // ---- deviations: keys, fp64 sum, range
  double sum = 0.0;
  unsigned dmin = kMissing, dmax = 0u;
  auto track_dev = [&](unsigned d) {
    if (d != kMissing) {
      sum += (double)__uint_as_float(d);
      dmin = d < dmin ? d : dmin;
      dmax = d > dmax ? d : dmax;
    }
  };
  if constexpr (LDS) {
    for (int q = tid; q < rk.nq; q += NT) {
      const uint4 v = keys[q];
      const uint4 d = make_uint4(dev_key(v.x, center), dev_key(v.y, center), dev_key(v.z, center),
                                 dev_key(v.w, center));
      track_dev(d.x); track_dev(d.y); track_dev(d.z); track_dev(d.w);
      keys[q] = d;
    }
  } else {
    rk.dev = true;
    rk.c = center;
    rk.sweep(track_dev);
  }
  sum = block_sum<NT>(sum, sc->redd);
  dmin = block_min_u32<NT>(dmin, sc->redu);
  dmax = ~block_min_u32<NT>(~dmax, sc->redu);

  // ---- MAD
  unsigned dlo, dup;
  select_middles<NT, LDS>(rk, dmin, dmax, (unsigned)n, bins, sc->sel, sc->redu, dlo, dup);
  const float mad = 0.5f * __uint_as_float(dlo) + 0.5f * __uint_as_float(dup);
  sigma = mad > 0.f ? 1.4826f * mad : 1.2533f * (float)(sum / (double)n);
}

}  // namespace fm
