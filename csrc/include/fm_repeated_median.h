// Siegel's repeated-median line through the block medians of a row, and the
// sweep that takes that line out of the row's keys: what K16
// (trend_robust.hip; the blocks are any L samples) and K20
// (seasonal_trend_robust.hip; a block is a whole cycle) share behind
// load_row_blocks, stated here only.
//
// Only for a translation unit built with contraction limited to single
// expressions (its `fm-hipcc-flags: -ffp-contract=on` line): under the
// library's -ffp-contract=fast the backend fuses the residual's product and
// difference across statements and past the pragma in detrend(), and the
// numpy contracts round twice.  Do not include it from a file that builds
// under the library's default.
#pragma once
#include "fm_radix_select.h"

namespace fm {

// LDS of a kernel that fits the line: the selection's scratch, the front's
// blocks, and the scratch of the slope.
template <int NT>
struct TrendShared {
  SelectScratch<NT> sc;
  RowBlocks blk;
  int q[kBatchBlocks];                                       // block indices of the medians above the quorum
  float pair[kBatchBlocks][kBatchBlocks];                    // a block's pair slopes, sorted in place
  float si[kBatchBlocks];                                    // the inner medians
  int nb;                                                    // blocks above the quorum
  float slope;
};

// The repeated median of the pair slopes of the block medians above the
// quorum (s->blk of load_row_blocks with J blocks of L samples, visible on
// entry; the medians are compacted in place): the inner medians one lane a
// block, the outer one on one lane.  Returns the slope per sample, 0 with
// fewer than min_blocks such blocks or when it is not finite, and B = how many
// there are, both the same in every thread; its barriers are its own.
template <int NT>
__device__ __forceinline__ float repeated_median_slope(int J, int L, int min_blocks, TrendShared<NT>* s, int& B) {
  const int tid = threadIdx.x;
  float* s_b = s->blk.median;
  if (tid == 0) {                                            // the medians above the quorum, oldest first (b <= j)
    int b = 0;
    for (int j = 0; j < J; ++j)
      if (s_b[j] == s_b[j]) {
        s_b[b] = s_b[j];
        s->q[b] = j;
        ++b;
      }
    s->nb = b;
  }
  __syncthreads();
  B = s->nb;
  const bool fit = B >= min_blocks;                          // uniform over the workgroup
  if (fit && tid < B) {
    int c = 0;
    for (int j = 0; j < B; ++j)
      if (j != tid) s->pair[tid][c++] = __fdiv_rn(s_b[j] - s_b[tid], (float)((s->q[j] - s->q[tid]) * L));
    s->si[tid] = small_median(s->pair[tid], c);
  }
  __syncthreads();
  if (tid == 0) {
    float slope = fit ? small_median(s->si, B) : 0.f;
    if ((__float_as_uint(slope) & 0x7F800000u) == 0x7F800000u) slope = 0.f;   // NaN, +-inf
    s->slope = slope;
  }
  __syncthreads();
  return s->slope;
}

// x - slope * t, the product and the difference each rounded to fp32: never
// one fused multiply-add
__device__ __forceinline__ float detrend(float x, float slope, float t) {
#pragma clang fp contract(off)
  const float m = __fmul_rn(slope, t);
  return __fsub_rn(x, m);
}

// The keys in place as the keys of the residuals r_i = x_i - slope * (i -
// last), key i at word a + i (the words outside the row are missing and stay
// so); every new key, an overflowed residual's missing key too, is handed to
// track.  No barrier: reduce what track gathered (block_sum) before the keys
// are read.
template <int NT, class Track>
__device__ __forceinline__ void detrend_keys(uint4* keys, int nq, int a, int last, float slope, Track& track) {
  for (int q = threadIdx.x; q < nq; q += NT) {
    const uint4 v = keys[q];
    unsigned e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (e[j] == kMissing) continue;
      const float t = (float)(4 * q + j - a - last);
      e[j] = enc_key(detrend(dec_key(e[j]), slope, t));
      track(e[j]);
    }
    keys[q] = make_uint4(e[0], e[1], e[2], e[3]);
  }
}

}  // namespace fm
