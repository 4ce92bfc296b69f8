// K15 level-shift robust model: the median / MAD band of a row, fitted on the
// history behind its latest persistent level shift, one 512-thread workgroup
// per row.
//
// The row goes into LDS and its J block medians are selected together
// (fm_radix_select.h, load_row_blocks: the last J * L samples, block 0 the
// oldest).  Then the whole-row median and MAD, the deviation keys taken on the
// fly so that the raw keys stay (LdsSpan), and one lane scans the candidates
// over the block medians.  Only a row with a shift (a branch uniform over the
// workgroup) selects twice more, the median and MAD of its segment [start, T).
// Every selection uses the key range of the whole row, which bounds every run
// of it.
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
constexpr int kMaxBlocks = kBatchBlocks;         // foremast_amd/ops/misc.py SHIFT_MAX_BLOCKS mirrors it

template <int NT>
struct ShiftShared {
  SelectScratch<NT> sc;
  RowBlocks blk;
  float side[kMaxBlocks];                                    // the scan's sort buffer
  int sb;                                                    // start block of the shift, -1 = none
  float delta, score;
};
static_assert(sizeof(ShiftShared<kShiftThreads>) + row_key_bytes(kRobustLdsKeys) <= kLaunchLds,
              "the longest row fits a launch");

template <int NT>
__global__ __launch_bounds__(NT) void shift_robust_kernel(const float* __restrict__ hist, int64_t ld, int T, int L,
                                                          int J, float sqrt_l, float kthr, int min_blocks,
                                                          float* __restrict__ out /*[R,6]*/) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_keys[];
  __shared__ ShiftShared<NT> s;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float* p = hist + row * ld;
  const int a = row_word(p);                                 // LDS word of key 0
  const unsigned* kw = reinterpret_cast<const unsigned*>(s_keys);
  const float* s_b = s.blk.median;                           // block medians, NaN = below the quorum
  const int* s_cnt = s.blk.cnt;

  // ---- the row -> keys; finite count, key range, block counts and medians
  KeyRange range;
  const int n = load_row_blocks<NT>(p, T, a, L, J, s_keys, &s.sc, &s.blk, range);
  if (n == 0) {
    if (tid == 0) {
      out[row * 6 + 0] = quiet_nan();
      out[row * 6 + 1] = quiet_nan();
      out[row * 6 + 2] = 0.f;
      out[row * 6 + 3] = 0.f;
      out[row * 6 + 4] = 0.f;
      out[row * 6 + 5] = 0.f;
    }
    return;
  }

  // ---- whole-row median and sigma
  float c_all, s_all;
  LdsSpan<NT> whole{kw, a, a + T};
  median_sigma(whole, (unsigned)n, range, &s.sc, c_all, s_all);

  // ---- candidate scan, one lane
  if (tid == 0) {
    const float se = __fdiv_rn(1.2533f * s_all, sqrt_l);
    int sb = -1;
    float delta = 0.f, score = 0.f;
    for (int j = J - min_blocks; j >= 3 && sb < 0; --j) {
      int npre = 0, npost = 0;
      for (int i = 0; i < j - 1; ++i)
        if (s_b[i] == s_b[i]) s.side[npre++] = s_b[i];
      if (npre < 2) continue;
      const float p0 = small_median(s.side, npre);
      for (int i = j; i < J; ++i)
        if (s_b[i] == s_b[i]) s.side[npost++] = s_b[i];
      if (npost < min_blocks) continue;
      const float p1 = small_median(s.side, npost);
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
    s.sb = sb;
    s.delta = delta;
    s.score = score;
  }
  __syncthreads();

  // ---- the band: the whole row, or the segment behind the shift
  const int sb = s.sb;                                       // uniform over the workgroup
  float center = c_all, sigma = s_all;
  int nseg = n, start = 0;
  if (sb >= 0) {
    nseg = 0;
    for (int j = sb; j < J; ++j) nseg += s_cnt[j];
    start = T - (J - sb) * L;
    LdsSpan<NT> seg{kw, a + start, a + T};
    median_sigma(seg, (unsigned)nseg, range, &s.sc, center, sigma);
  }
  if (tid == 0) {
    out[row * 6 + 0] = center;
    out[row * 6 + 1] = sigma;
    out[row * 6 + 2] = (float)nseg;
    out[row * 6 + 3] = (float)start;
    out[row * 6 + 4] = s.delta;
    out[row * 6 + 5] = s.score;
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
  if (row_key_bytes(T) + sizeof(ShiftShared<kShiftThreads>) > kLaunchLds) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((shift_robust_kernel<kShiftThreads>), dim3((unsigned)R), dim3(kShiftThreads), row_key_bytes(T),
                     stream, hist, ld, T, L, J, sqrtf((float)L), k, min_blocks, out);
  FM_LAUNCH_CHECK();
  return 0;
}
