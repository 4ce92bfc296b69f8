// K16 trend robust model: a straight line fitted to a row by Siegel's repeated
// median over the medians of its blocks, and the median / MAD band of the
// residuals about it, one 512-thread workgroup per row.
//
// The row is read from HBM once into LDS as the order-preserving keys of
// fm_radix_select.h, key i at word a + i (load_row_keys, as K15).
//
// Per row: the finite count of each of the J blocks (the last J * L samples,
// block 0 the oldest); the medians of all non-empty blocks, selected together
// in the same radix passes (select_block_middles: a block counts into its own
// 128 of the 2,048 bins, so a pass costs one sweep of the blocks whatever J
// is); the repeated median of the pair slopes of the B <= 16 block medians,
// the inner medians one lane a block and the outer one on one lane; the keys
// rewritten in place as the keys of the residuals r_i = x_i - slope * (i -
// (T - 1)), a product and a difference each rounded to fp32 (no fused
// multiply-add: the numpy contract rounds twice); then K15's span_stats over
// the whole row, whose median is the level at the last history sample.
//
// Block size and LDS as K15: 512 threads, up to 52 KiB of keys, 8 KiB of bins
// and 1 KiB of sort buffers, so two workgroups of a full row share a CU.  The
// contract is foremast_amd/ops/misc.py ref_trend_robust; centre, n and slope
// are exact, and sigma is where MAD > 0.
//
// Built with contraction limited to single expressions: under the library's
// -ffp-contract=fast the backend fuses the residual's product and difference
// across statements and past the pragma in detrend().
// fm-hipcc-flags: -ffp-contract=on
#include "fm_common.h"
#include "fm_radix_select.h"

using namespace fm;

namespace {

constexpr int kTrendThreads = 512;
constexpr int kMaxBlocks = kBatchBlocks;         // foremast_amd/ops/misc.py SHIFT_MAX_BLOCKS mirrors it

// x - slope * t, the product and the difference each rounded to fp32: never
// one fused multiply-add
__device__ __forceinline__ float detrend(float x, float slope, float t) {
#pragma clang fp contract(off)
  const float m = __fmul_rn(slope, t);
  return __fsub_rn(x, m);
}

template <int NT>
__global__ __launch_bounds__(NT) void trend_robust_kernel(const float* __restrict__ hist, int64_t ld, int T, int L,
                                                          int J, int min_blocks, float* __restrict__ out /*[R,4]*/) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_keys[];
  __shared__ __attribute__((aligned(16))) unsigned s_bins[kBins];
  __shared__ unsigned s_sel[3];
  __shared__ unsigned s_redu[NT / FM_WAVE];
  __shared__ int s_redi[NT / FM_WAVE];
  __shared__ double s_redd[NT / FM_WAVE];
  __shared__ int s_cnt[kMaxBlocks];                          // finite samples of each block
  __shared__ BlockSel s_blk;
  __shared__ float s_b[kMaxBlocks];                          // medians of the non-empty blocks, oldest first
  __shared__ int s_q[kMaxBlocks];                            // and their block indices
  __shared__ float s_pair[kMaxBlocks][kMaxBlocks];           // a block's pair slopes, sorted in place
  __shared__ float s_si[kMaxBlocks];                         // the inner medians
  __shared__ int s_nb;                                       // non-empty blocks
  __shared__ float s_slope;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float* p = hist + row * ld;
  const int a = (int)(((uintptr_t)p >> 2) & 3u);             // LDS word of key 0
  const int nq = (a + T + 3) >> 2;
  unsigned* kw = reinterpret_cast<unsigned*>(s_keys);
  const float qnan = __uint_as_float(0x7FC00000u);
  for (int i = tid; i < kBins; i += NT) s_bins[i] = 0u;
  if (tid < kMaxBlocks) s_cnt[tid] = 0;

  // ---- the row -> keys in place; finite count and key range
  int n = 0;
  unsigned kmin = kMissing, kmax = 0u;
  load_row_keys<NT>(p, T, a, s_keys, n, kmin, kmax);
  n = block_sum<NT>(n, s_redi);                              // (barriers: keys, bins and counts visible)
  if (n == 0) {
    if (tid == 0) *reinterpret_cast<float4*>(out + row * 4) = make_float4(qnan, qnan, 0.f, 0.f);
    return;
  }
  kmin = block_min_u32<NT>(kmin, s_redu);
  kmax = ~block_min_u32<NT>(~kmax, s_redu);

  // ---- finite count of each block; a block below the quorum takes no part
  const int off = T - J * L;                                 // columns in front of the blocks
  if (J > 0) count_block_keys<NT>(kw, a + off, L, J, s_cnt);
  __syncthreads();
  if (tid < kMaxBlocks) {
    const int need = L / 4 > 1 ? L / 4 : 1;
    s_blk.n[tid] = (tid < J && s_cnt[tid] >= need) ? (unsigned)s_cnt[tid] : 0u;
  }
  __syncthreads();

  // ---- all block medians in the same passes
  if (J > 0) select_block_middles<NT>(kw, a + off, L, J, kmin, kmax, s_bins, &s_blk);

  // ---- repeated median of the pair slopes: the inner medians one lane a block
  if (tid == 0) {
    int B = 0;
    for (int j = 0; j < J; ++j)
      if (s_blk.n[j] != 0u) {
        s_b[B] = 0.5f * dec_key(s_blk.lo[j]) + 0.5f * dec_key(s_blk.up[j]);
        s_q[B] = j;
        ++B;
      }
    s_nb = B;
  }
  __syncthreads();
  const int B = s_nb;
  const bool fit = B >= min_blocks;                          // uniform over the workgroup
  if (fit && tid < B) {
    int c = 0;
    for (int j = 0; j < B; ++j)
      if (j != tid) s_pair[tid][c++] = __fdiv_rn(s_b[j] - s_b[tid], (float)((s_q[j] - s_q[tid]) * L));
    s_si[tid] = small_median(s_pair[tid], c);
  }
  __syncthreads();
  if (tid == 0) {
    float slope = fit ? small_median(s_si, B) : 0.f;
    if ((__float_as_uint(slope) & 0x7F800000u) == 0x7F800000u) slope = 0.f;   // NaN, +-inf
    s_slope = slope;
  }
  __syncthreads();
  const float slope = s_slope;

  // ---- the keys of the residuals in place; their finite count and key range
  n = 0;
  kmin = kMissing;
  kmax = 0u;
  for (int q = tid; q < nq; q += NT) {
    const uint4 v = s_keys[q];
    unsigned e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (e[j] == kMissing) continue;                        // (the words outside the row are missing)
      const float t = (float)(4 * q + j - a - (T - 1));
      const unsigned k = enc_key(detrend(dec_key(e[j]), slope, t));
      e[j] = k;
      if (k != kMissing) {
        ++n;
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
      }
    }
    s_keys[q] = make_uint4(e[0], e[1], e[2], e[3]);
  }
  n = block_sum<NT>(n, s_redi);
  if (n == 0) {                                              // every residual overflowed
    if (tid == 0) *reinterpret_cast<float4*>(out + row * 4) = make_float4(qnan, qnan, 0.f, slope);
    return;
  }
  kmin = block_min_u32<NT>(kmin, s_redu);
  kmax = ~block_min_u32<NT>(~kmax, s_redu);

  // ---- median and sigma of the residuals
  float center, sigma;
  span_stats<NT>(kw, a, a + T, (unsigned)n, kmin, kmax, s_bins, s_sel, s_redu, s_redd, center, sigma);
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
  // keys: the row plus up to 3 words in front, in whole quads
  const size_t lds = (size_t)((T + 6) / 4) * sizeof(uint4);
  hipLaunchKernelGGL((trend_robust_kernel<kTrendThreads>), dim3((unsigned)R), dim3(kTrendThreads), lds, stream, hist,
                     ld, T, L, J, min_blocks, out);
  FM_LAUNCH_CHECK();
  return 0;
}
