// K15 level-shift robust model: the median / MAD band of a row, fitted on the
// history behind its latest persistent level shift, one 512-thread workgroup
// per row.
//
// The row is read from HBM once into LDS as the order-preserving keys of
// fm_radix_select.h, key i at word a + i with a = (address / 4) & 3 of the
// row's first sample (load_row_keys: a 16-B global load and its 16-B LDS
// store are aligned together whatever the row's alignment, and a block of the
// row is a run of words).  The words before and behind the row in its first
// and last quad hold the missing key.
//
// Per row: the whole-row median; the finite count of each of the J blocks
// (the last J * L samples, block 0 the oldest) and the median of every
// non-empty one, each a radix selection over a run of words (SpanKeys); the
// whole-row MAD, its deviation keys taken on the fly so that the raw keys
// stay; then one lane scans the candidates over the J block medians.  Only a
// row with a shift (a branch uniform over the workgroup) selects twice more,
// the median and MAD of its segment [start, T).  Every selection uses the
// key range of the whole row, which bounds every run of it.
//
// Block size: 512 threads as K13 and K14.  A full row is 26 quads a thread,
// and by a workgroup's LDS (up to 52 KiB of keys, 8 KiB of bins) two
// workgroups of a full row share a CU, three at 7 x 1,440 samples.  The
// contract is foremast_amd/ops/misc.py ref_shift_robust; centre, n, start and
// delta are exact, and sigma is where MAD > 0.
#include "fm_common.h"
#include "fm_radix_select.h"

using namespace fm;

namespace {

constexpr int kShiftThreads = 512;
constexpr int kMaxBlocks = 16;                   // foremast_amd/ops/misc.py SHIFT_MAX_BLOCKS mirrors it

template <int NT>
__global__ __launch_bounds__(NT) void shift_robust_kernel(const float* __restrict__ hist, int64_t ld, int T, int L,
                                                          int J, float sqrt_l, float kthr, int min_blocks,
                                                          float* __restrict__ out /*[R,6]*/) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_keys[];
  __shared__ __attribute__((aligned(16))) unsigned s_bins[kBins];
  __shared__ unsigned s_sel[3];
  __shared__ unsigned s_redu[NT / FM_WAVE];
  __shared__ int s_redi[NT / FM_WAVE];
  __shared__ double s_redd[NT / FM_WAVE];
  __shared__ int s_cnt[kMaxBlocks];                          // finite samples of each block
  __shared__ float s_b[kMaxBlocks];                          // block medians, NaN = empty
  __shared__ float s_side[kMaxBlocks];                       // the scan's sort buffer
  __shared__ int s_sb;                                       // start block of the shift, -1 = none
  __shared__ float s_delta, s_score;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float* p = hist + row * ld;
  const int a = (int)(((uintptr_t)p >> 2) & 3u);             // LDS word of key 0
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
    if (tid == 0) {
      out[row * 6 + 0] = qnan;
      out[row * 6 + 1] = qnan;
      out[row * 6 + 2] = 0.f;
      out[row * 6 + 3] = 0.f;
      out[row * 6 + 4] = 0.f;
      out[row * 6 + 5] = 0.f;
    }
    return;
  }
  kmin = block_min_u32<NT>(kmin, s_redu);
  kmax = ~block_min_u32<NT>(~kmax, s_redu);

  // ---- finite count of each block
  const int off = T - J * L;                                 // columns in front of the blocks
  if (J > 0) count_block_keys<NT>(kw, a + off, L, J, s_cnt);
  __syncthreads();

  // ---- whole-row median and sigma
  float c_all, s_all;
  span_stats<NT>(kw, a, a + T, (unsigned)n, kmin, kmax, s_bins, s_sel, s_redu, s_redd, c_all, s_all);

  // ---- block medians
  const int need = L / 4 > 1 ? L / 4 : 1;
  for (int j = 0; j < J; ++j) {
    const int c = s_cnt[j];                                  // uniform over the workgroup
    float bj = qnan;
    if (c >= need) {
      const int lo = a + off + j * L;
      const SpanKeys<NT> sk{kw, lo, lo + L, false, 0.f};
      unsigned klo, kup;
      select_middles_keys<NT>(sk, kmin, kmax, (unsigned)c, s_bins, s_sel, s_redu, klo, kup);
      bj = 0.5f * dec_key(klo) + 0.5f * dec_key(kup);
    }
    if (tid == 0) s_b[j] = bj;
  }

  // ---- candidate scan, one lane
  if (tid == 0) {
    const float se = __fdiv_rn(1.2533f * s_all, sqrt_l);
    int sb = -1;
    float delta = 0.f, score = 0.f;
    for (int j = J - min_blocks; j >= 3 && sb < 0; --j) {
      int npre = 0, npost = 0;
      for (int i = 0; i < j - 1; ++i)
        if (s_b[i] == s_b[i]) s_side[npre++] = s_b[i];
      if (npre < 2) continue;
      const float p0 = small_median(s_side, npre);
      for (int i = j; i < J; ++i)
        if (s_b[i] == s_b[i]) s_side[npost++] = s_b[i];
      if (npost < min_blocks) continue;
      const float p1 = small_median(s_side, npost);
      const float d = p1 - p0;
      float den = se;
      for (int i = 0; i < J; ++i) {
        if (i == j - 1 || !(s_b[i] == s_b[i])) continue;
        const float dv = fabsf(s_b[i] - (i < j ? p0 : p1));
        den = den > dv ? den : dv;
      }
      const float sc = den > 0.f ? __fdiv_rn(fabsf(d), den) : (d != 0.f ? __uint_as_float(0x7F800000u) : 0.f);
      if (sc > kthr) {
        const float bt = s_b[j - 1];
        sb = (bt == bt && fabsf(bt - p1) <= den) ? j - 1 : j;
        delta = d;
        score = sc;
      } else if (sc > score) {
        score = sc;
      }
    }
    s_sb = sb;
    s_delta = delta;
    s_score = score;
  }
  __syncthreads();

  // ---- the band: the whole row, or the segment behind the shift
  const int sb = s_sb;                                       // uniform over the workgroup
  float center = c_all, sigma = s_all;
  int nseg = n, start = 0;
  if (sb >= 0) {
    nseg = 0;
    for (int j = sb; j < J; ++j) nseg += s_cnt[j];
    start = T - (J - sb) * L;
    span_stats<NT>(kw, a + start, a + T, (unsigned)nseg, kmin, kmax, s_bins, s_sel, s_redu, s_redd, center, sigma);
  }
  if (tid == 0) {
    out[row * 6 + 0] = center;
    out[row * 6 + 1] = sigma;
    out[row * 6 + 2] = (float)nseg;
    out[row * 6 + 3] = (float)start;
    out[row * 6 + 4] = s_delta;
    out[row * 6 + 5] = s_score;
  }
}

}  // namespace

// out [R,6] fp32 = (centre, sigma, finite count, start, delta, score) of
// hist[r, :T] under the level-shift model with J blocks of L samples (the last
// J * L columns), threshold k and min_blocks; hist and ld need 4-byte alignment
// only.  The row is selected in LDS: nothing is launched unless T <=
// kRobustLdsKeys, 0 <= J <= 16, J * L <= T and min_blocks >= 1.
FM_API int fm_shift_robust(const float* hist, int64_t ld, int T, int64_t R, int L, int J, float k, int min_blocks,
                           float* out, hipStream_t stream) {
  if (T < 0 || T > kRobustLdsKeys || L < 1 || J < 0 || J > kMaxBlocks || (int64_t)J * L > T || min_blocks < 1 ||
      R > 0x7FFFFFFF || (((uintptr_t)hist) & 3) != 0)
    return (int)hipErrorInvalidValue;
  if (R <= 0) return 0;
  // keys: the row plus up to 3 words in front, in whole quads
  const size_t lds = (size_t)((T + 6) / 4) * sizeof(uint4);
  hipLaunchKernelGGL((shift_robust_kernel<kShiftThreads>), dim3((unsigned)R), dim3(kShiftThreads), lds, stream, hist,
                     ld, T, L, J, sqrtf((float)L), k, min_blocks, out);
  FM_LAUNCH_CHECK();
  return 0;
}
