// K14 seasonal robust model: a per-phase median profile of the last J whole
// cycles of a row, smoothed over neighbouring phases, and the MAD of the
// residuals about it, one 512-thread workgroup per row.
//
// The span (the last J * m columns of the row) is read from HBM once into LDS
// as the keys of fm_radix_select.h, key i at word a + i (load_row_keys): a
// phase is a position.
//
// Raw profile: a thread takes phases p, p + 512, ...; the J keys of a phase
// sit m words apart (adjacent lanes read adjacent words), are sorted in
// registers by an odd-even transposition network with the missing key last,
// and the two middles of the finite ones are averaged (K13's median rule).
// Smoothing: the mean of the finite raw values within k phases, circular,
// summed and divided in fp64; a thread keeps its phases' means in registers
// until every thread has read the raw values, so one m-word buffer serves
// both.  Then the keys are overwritten with the bits of |x - profile[phase]|,
// summed in fp64, and one radix selection finds their middle: the MAD, with
// no re-centring.
//
// The profile buffer is the selection's bin array while m <= 2,048 (the bins
// are not in use before the selection and are cleared after the last read of
// the profile), so at the 7 x 1,440 workload a workgroup takes the LDS of a
// K13 workgroup and three of them share a CU; a longer period puts it behind
// the keys.  The contract is foremast_amd/ops/misc.py ref_seasonal_robust;
// with k = 0 the profile is exact, and sigma is exact given the profile where
// MAD > 0.
#include "fm_common.h"
#include "fm_radix_select.h"

using namespace fm;

namespace {

constexpr int kSeasonalThreads = 512;
constexpr int kMaxCycles = 16;                   // foremast_amd/ops/misc.py SEASONAL_MAX_CYCLES mirrors it
constexpr int kMaxPeriod = kRobustLdsKeys / 4;   // (J + 2) m <= kRobustLdsKeys with J >= 2
static_assert(sizeof(SelectScratch<kSeasonalThreads>) + row_key_bytes(kRobustLdsKeys) <= kLaunchLds,
              "the longest span and a profile behind it fit a launch");

// compare-exchange: the smaller key first
__device__ __forceinline__ void cex(unsigned& a, unsigned& b) {
  const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

template <int NT>
__global__ __launch_bounds__(NT) void seasonal_robust_kernel(const float* __restrict__ hist, int64_t ld, int T,
                                                             int m, int J, int k, int H,
                                                             float* __restrict__ forecast, int64_t ldf,
                                                             float* __restrict__ stats /*[R,2]*/,
                                                             float* __restrict__ profile /*[R,m] or null*/) {
  constexpr int kPhases = (kMaxPeriod + NT - 1) / NT;        // most phases a thread takes
  extern __shared__ __attribute__((aligned(16))) uint4 s_keys[];
  __shared__ SelectScratch<NT> s_sc;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int N = J * m;                                       // span length
  const float* p = hist + row * ld + (T - N);
  const int a = row_word(p);                                 // LDS word of key 0
  const int nq = row_quads(a, N);
  unsigned* kw = reinterpret_cast<unsigned*>(s_keys);
  float* prof = reinterpret_cast<float*>(m <= kBins ? s_sc.bins : kw + 4 * nq);   // [m]: raw, then smoothed

  // ---- the span -> keys in place; finite count (the key range is not needed)
  int n = 0;
  auto count = [&](unsigned k) { n += k != kMissing; };
  load_row_keys<NT>(p, N, a, s_keys, count);
  n = uniform(block_sum<NT>(n, s_sc.redi));                  // (barriers: keys visible)
  const float qnan = quiet_nan();
  if (n == 0) {
    for (int h = tid; h < H; h += NT) forecast[row * ldf + h] = qnan;
    if (profile != nullptr)
      for (int ph = tid; ph < m; ph += NT) profile[row * (int64_t)m + ph] = qnan;
    if (tid == 0) {
      stats[row * 2 + 0] = qnan;
      stats[row * 2 + 1] = 0.f;
    }
    return;
  }

  // ---- raw profile: per-phase median of the finite samples
  for (int ph = tid; ph < m; ph += NT) {
    unsigned s[kMaxCycles];
    int c = 0;
#pragma unroll
    for (int j = 0; j < kMaxCycles; ++j) {
      s[j] = j < J ? kw[a + ph + j * m] : kMissing;
      c += s[j] != kMissing;
    }
#pragma unroll
    for (int r = 0; r < kMaxCycles; ++r) {
      if (r < J) {                                           // J rounds sort J keys; the padding is in place
#pragma unroll
        for (int i = r & 1; i + 1 < kMaxCycles; i += 2) cex(s[i], s[i + 1]);
      }
    }
    const int il = (c - 1) >> 1, iu = c >> 1;
    unsigned klo = kMissing, kup = kMissing;
#pragma unroll
    for (int j = 0; j < kMaxCycles; ++j) {
      klo = j == il ? s[j] : klo;
      kup = j == iu ? s[j] : kup;
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

  // ---- forecast: the profile from phase 0 on, wrapped
  {
    const int stepm = NT % m;
    int ph = tid % m;
    for (int h = tid; h < H; h += NT) {
      forecast[row * ldf + h] = prof[ph];
      ph += stepm;
      if (ph >= m) ph -= m;
    }
  }

  // ---- residuals about the profile: keys, fp64 sum, range
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
  const double sum = uniform(block_sum<NT>(dev.sum, s_sc.redd));   // (barriers: the last read of the profile is behind)
  s_sc.clear_bins();                                         // (made visible by the barriers of mad_sigma's range)

  // ---- MAD: the padding words hold the missing key, so the span is swept as a whole row
  const LdsRow<NT> rk{s_keys, nq};
  const float sigma = mad_sigma(rk, (unsigned)n, sum, dev.range, &s_sc);
  if (tid == 0) {
    stats[row * 2 + 0] = sigma;
    stats[row * 2 + 1] = (float)n;
  }
}

}  // namespace

// Per row of hist[r, :T]: the smoothed per-phase median profile of its last
// J * m samples (phase = position in that span mod m), forecast[r, h] =
// profile[h mod m] for h < H (leading dimension ldf), stats[r] = (sigma,
// finite count of the span), and the profile [R, m] when its pointer is not
// null.  k = half width of the smoothing window.  hist and ld need 4-byte
// alignment only.  Nothing is launched unless 2 <= J <= 16, J * m <= T,
// (J + 2) * m fits the LDS budget of K13 and 2 k + 1 <= m.
FM_API int fm_seasonal_robust(const float* hist, int64_t ld, int T, int64_t R, int m, int J, int k, int H,
                              float* forecast, int64_t ldf, float* stats, float* profile, hipStream_t stream) {
  if (m < 1 || J < 2 || J > kMaxCycles || (int64_t)(J + 2) * m > kRobustLdsKeys || (int64_t)J * m > T || k < 0 ||
      2 * (int64_t)k + 1 > m || H < 0 || R > 0x7FFFFFFF || (((uintptr_t)hist) & 3) != 0)
    return (int)hipErrorInvalidValue;
  if (R <= 0) return 0;
  // keys: the span plus up to 3 words in front, in whole quads; behind them
  // the profile when the bin array is too short for it
  const size_t lds = row_key_bytes(J * m) + (m > kBins ? (size_t)m : 0) * sizeof(float);
  if (lds + sizeof(SelectScratch<kSeasonalThreads>) > kLaunchLds) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((seasonal_robust_kernel<kSeasonalThreads>), dim3((unsigned)R), dim3(kSeasonalThreads), lds, stream,
                     hist, ld, T, m, J, k, H, forecast, ldf, stats, profile);
  FM_LAUNCH_CHECK();
  return 0;
}
