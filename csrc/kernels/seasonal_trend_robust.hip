// K20 seasonal trend robust model: a straight line through the medians of the
// last J whole cycles of a row (Siegel's repeated median, K16's stage), and
// about that line a per-phase median profile and the MAD of the residuals
// (K14's stages), one 512-thread workgroup per row.
//
// The span (the last J * m columns) is read from HBM once and stays in LDS as
// the keys of fm_radix_select.h.  load_row_blocks selects the J cycle medians
// together: a block is a whole cycle, so a cycle of any shape moves every
// block median alike and does not bias the slope.  The keys are then rewritten
// in place as the keys of the residuals r_i = x_i - slope * (i - (N - 1)), a
// product and a difference each rounded to fp32; the profile of the residuals
// therefore carries the level at the last history sample plus the cycle, and
// forecast[h - 1] = profile[(h - 1) mod m] + slope * h (rounded twice too).
// From there on it is K14: per-phase register sort, circular smoothing with
// fp64 sums, deviations in place, one radix selection for the MAD.
//
// LDS as K14: the profile buffer is the selection's bin array while m <= 2,048
// (load_row_blocks hands the bins back zeroed, and they are cleared after the
// last read of the profile), else it sits behind the keys; the shared struct
// is K16's.  The contract is foremast_amd/ops/misc.py
// ref_seasonal_trend_robust; n, slope and nblocks are exact, the profile is
// with k = 0, and sigma is given the profile where MAD > 0.
//
// Built with contraction limited to single expressions, as K16 (the reason is
// at the top of trend_robust.hip).
// fm-hipcc-flags: -ffp-contract=on
#include "fm_common.h"
#include "fm_radix_select.h"

using namespace fm;

namespace {

constexpr int kStThreads = 512;
constexpr int kMaxCycles = kBatchBlocks;         // foremast_amd/ops/misc.py SEASONAL_MAX_CYCLES mirrors it
constexpr int kMaxPeriod = kRobustLdsKeys / 4;   // (J + 2) m <= kRobustLdsKeys with J >= 2

// x - slope * t, the product and the difference each rounded to fp32: never
// one fused multiply-add
__device__ __forceinline__ float detrend(float x, float slope, float t) {
#pragma clang fp contract(off)
  const float m = __fmul_rn(slope, t);
  return __fsub_rn(x, m);
}

// compare-exchange: the smaller key first
__device__ __forceinline__ void cex(unsigned& a, unsigned& b) {
  const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

template <int NT>
struct SeasonalTrendShared {
  SelectScratch<NT> sc;
  RowBlocks blk;
  int q[kMaxCycles];                                         // cycle indices of the medians above the quorum
  float pair[kMaxCycles][kMaxCycles];                        // a cycle's pair slopes, sorted in place
  float si[kMaxCycles];                                      // the inner medians
  int nb;                                                    // cycles above the quorum
  float slope;
};
// (J + 2) m <= kRobustLdsKeys: the span and a profile behind it are no longer than the longest row
static_assert(sizeof(SeasonalTrendShared<kStThreads>) + row_key_bytes(kRobustLdsKeys) <= kLaunchLds,
              "the longest span and a profile behind it fit a launch");

template <int NT>
__global__ __launch_bounds__(NT) void seasonal_trend_robust_kernel(const float* __restrict__ hist, int64_t ld, int T,
                                                                   int m, int J, int k, int min_blocks, int H,
                                                                   float* __restrict__ forecast, int64_t ldf,
                                                                   float* __restrict__ stats /*[R,4]*/,
                                                                   float* __restrict__ profile /*[R,m] or null*/) {
  constexpr int kPhases = (kMaxPeriod + NT - 1) / NT;        // most phases a thread takes
  extern __shared__ __attribute__((aligned(16))) uint4 s_keys[];
  __shared__ SeasonalTrendShared<NT> s;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int N = J * m;                                       // span length
  const float* p = hist + row * ld + (T - N);
  const int a = row_word(p);                                 // LDS word of key 0
  const int nq = row_quads(a, N);
  unsigned* kw = reinterpret_cast<unsigned*>(s_keys);
  float* prof = reinterpret_cast<float*>(m <= kBins ? s.sc.bins : kw + 4 * nq);   // [m]: raw, then smoothed
  float* s_b = s.blk.median;                                 // cycle medians, compacted below
  const float qnan = quiet_nan();

  // a row without a finite residual: NaN forecast, profile and sigma
  auto empty = [&](float slope, float nblocks) {
    for (int h = tid; h < H; h += NT) forecast[row * ldf + h] = qnan;
    if (profile != nullptr)
      for (int ph = tid; ph < m; ph += NT) profile[row * (int64_t)m + ph] = qnan;
    if (tid == 0) *reinterpret_cast<float4*>(stats + row * 4) = make_float4(qnan, 0.f, slope, nblocks);
  };

  // ---- the span -> keys; finite count, key range, cycle counts and medians
  KeyRange range;
  int n = load_row_blocks<NT>(p, N, a, m, J, s_keys, &s.sc, &s.blk, range);
  if (n == 0) {
    empty(0.f, 0.f);
    return;
  }

  // ---- repeated median of the pair slopes: the inner medians one lane a cycle
  if (tid == 0) {                                            // the medians above the quorum, oldest first (B <= j)
    int B = 0;
    for (int j = 0; j < J; ++j)
      if (s_b[j] == s_b[j]) {
        s_b[B] = s_b[j];
        s.q[B] = j;
        ++B;
      }
    s.nb = B;
  }
  __syncthreads();
  const int B = s.nb;
  const bool fit = B >= min_blocks;                          // uniform over the workgroup
  if (fit && tid < B) {
    int c = 0;
    for (int j = 0; j < B; ++j)
      if (j != tid) s.pair[tid][c++] = __fdiv_rn(s_b[j] - s_b[tid], (float)((s.q[j] - s.q[tid]) * m));
    s.si[tid] = small_median(s.pair[tid], c);
  }
  __syncthreads();
  if (tid == 0) {
    float slope = fit ? small_median(s.si, B) : 0.f;
    if ((__float_as_uint(slope) & 0x7F800000u) == 0x7F800000u) slope = 0.f;   // NaN, +-inf
    s.slope = slope;
  }
  __syncthreads();
  const float slope = s.slope;

  // ---- the keys of the residuals in place; their finite count
  {
    int fin = 0;
    for (int q = tid; q < nq; q += NT) {
      const uint4 v = s_keys[q];
      unsigned e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (e[j] == kMissing) continue;                      // (the words outside the span are missing)
        const float t = (float)(4 * q + j - a - (N - 1));
        e[j] = enc_key(detrend(dec_key(e[j]), slope, t));
        fin += e[j] != kMissing;
      }
      s_keys[q] = make_uint4(e[0], e[1], e[2], e[3]);
    }
    n = uniform(block_sum<NT>(fin, s.sc.redi));              // (barriers: residual keys visible)
  }
  if (n == 0) {                                              // every residual overflowed
    empty(slope, (float)B);
    return;
  }

  // ---- raw profile: per-phase median of the finite residuals
  for (int ph = tid; ph < m; ph += NT) {
    unsigned c16[kMaxCycles];
    int c = 0;
#pragma unroll
    for (int j = 0; j < kMaxCycles; ++j) {
      c16[j] = j < J ? kw[a + ph + j * m] : kMissing;
      c += c16[j] != kMissing;
    }
#pragma unroll
    for (int r = 0; r < kMaxCycles; ++r) {
      if (r < J) {                                           // J rounds sort J keys; the padding is in place
#pragma unroll
        for (int i = r & 1; i + 1 < kMaxCycles; i += 2) cex(c16[i], c16[i + 1]);
      }
    }
    const int il = (c - 1) >> 1, iu = c >> 1;
    unsigned klo = kMissing, kup = kMissing;
#pragma unroll
    for (int j = 0; j < kMaxCycles; ++j) {
      klo = j == il ? c16[j] : klo;
      kup = j == iu ? c16[j] : kup;
    }
    prof[ph] = c == 0 ? qnan : 0.5f * dec_key(klo) + 0.5f * dec_key(kup);
  }
  __syncthreads();

  // ---- smoothing in place: mean of the finite raw values within k phases, circular
  {
    float sm[kPhases];
#pragma unroll
    for (int it = 0; it < kPhases; ++it) {
      const int ph = tid + it * NT;
      sm[it] = qnan;
      if (ph < m) {
        double sum = 0.0;
        int cnt = 0;
        int q = ph - k;
        if (q < 0) q += m;
        for (int d = -k; d <= k; ++d) {
          const float v = prof[q];
          if (v == v) {
            sum += (double)v;
            ++cnt;
          }
          if (++q == m) q = 0;
        }
        if (cnt != 0) sm[it] = (float)(sum / (double)cnt);
      }
    }
    __syncthreads();                                         // every raw value read
#pragma unroll
    for (int it = 0; it < kPhases; ++it) {
      const int ph = tid + it * NT;
      if (ph < m) {
        prof[ph] = sm[it];
        if (profile != nullptr) profile[row * (int64_t)m + ph] = sm[it];
      }
    }
    __syncthreads();
  }

  // ---- forecast: the profile from phase 0 on, wrapped, plus the line from the last sample on
  {
    const int stepm = NT % m;
    int ph = tid % m;
    for (int h = tid; h < H; h += NT) {
      forecast[row * ldf + h] = __fadd_rn(prof[ph], __fmul_rn(slope, (float)(h + 1)));
      ph += stepm;
      if (ph >= m) ph -= m;
    }
  }

  // ---- deviations of the residuals about the profile: keys, fp64 sum, range
  DevTally dev;
  {
    // word w holds span index w - a: its phase, carried along instead of divided out
    const int stepm = (4 * NT) % m;
    int ph0 = (4 * tid - a) % m;                             // (the padding in front of the span: a remainder below zero)
    if (ph0 < 0) ph0 += m;
    for (int q = tid; q < nq; q += NT) {
      const uint4 v = s_keys[q];
      unsigned e[4] = {v.x, v.y, v.z, v.w};
      int ph = ph0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (e[j] != kMissing) {
          e[j] = dev_key(e[j], prof[ph]);
          dev(e[j]);
        }
        if (++ph == m) ph = 0;
      }
      s_keys[q] = make_uint4(e[0], e[1], e[2], e[3]);
      ph0 += stepm;
      if (ph0 >= m) ph0 -= m;
    }
  }
  const double sum = uniform(block_sum<NT>(dev.sum, s.sc.redd));   // (barriers: the last read of the profile is behind)
  s.sc.clear_bins();                                         // (made visible by the barriers of mad_sigma's range)

  // ---- MAD: the padding words hold the missing key, so the span is swept as a whole row
  const LdsRow<NT> rk{s_keys, nq};
  const float sigma = mad_sigma(rk, (unsigned)n, sum, dev.range, &s.sc);
  if (tid == 0) *reinterpret_cast<float4*>(stats + row * 4) = make_float4(sigma, (float)n, slope, (float)B);
}

}  // namespace

// Per row of hist[r, :T], over its last J * m samples: the repeated-median
// slope of the J cycle medians (0 with fewer than min_blocks non-empty cycles),
// the smoothed per-phase median profile of the residuals about that line
// anchored at the last sample, forecast[r, h] = profile[h mod m] + slope *
// (h + 1) for h < H (leading dimension ldf), stats[r] = (sigma, finite count
// of the residuals, slope, non-empty cycles), and the profile [R, m] when its
// pointer is not null.  k = half width of the smoothing window.  stats needs
// 16-byte alignment, hist and ld 4-byte alignment only.  Nothing is launched
// unless 2 <= J <= 16, J * m <= T, (J + 2) * m fits the LDS budget of K13,
// 2 k + 1 <= m and min_blocks >= 2.
FM_API int fm_seasonal_trend_robust(const float* hist, int64_t ld, int T, int64_t R, int m, int J, int k,
                                    int min_blocks, int H, float* forecast, int64_t ldf, float* stats, float* profile,
                                    hipStream_t stream) {
  if (m < 1 || J < 2 || J > kMaxCycles || (int64_t)(J + 2) * m > kRobustLdsKeys || (int64_t)J * m > T || k < 0 ||
      2 * (int64_t)k + 1 > m || min_blocks < 2 || H < 0 || R > 0x7FFFFFFF || (((uintptr_t)hist) & 3) != 0 ||
      (((uintptr_t)stats) & 15) != 0)
    return (int)hipErrorInvalidValue;
  if (R <= 0) return 0;
  // keys: the span plus up to 3 words in front, in whole quads; behind them
  // the profile when the bin array is too short for it
  const size_t lds = row_key_bytes(J * m) + (m > kBins ? (size_t)m : 0) * sizeof(float);
  if (lds + sizeof(SeasonalTrendShared<kStThreads>) > kLaunchLds) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((seasonal_trend_robust_kernel<kStThreads>), dim3((unsigned)R), dim3(kStThreads), lds, stream,
                     hist, ld, T, m, J, k, min_blocks, H, forecast, ldf, stats, profile);
  FM_LAUNCH_CHECK();
  return 0;
}
