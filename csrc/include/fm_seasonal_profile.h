// The per-phase stages of the seasonal robust kernels, stated here only: K14
// (seasonal_robust.hip), K20 (seasonal_trend_robust.hip) and K22
// (seasonal_scale_robust.hip), whose forecast, profile and sigma0 are K14's bit
// for bit because they are this code; K26 (seasonal_quantile_robust.hip) runs
// them through K22's stages (fm_seasonal_scale.h).
//
// The span of J cycles of m samples sits in LDS as the keys of
// fm_radix_select.h, key i at word a + i: a phase is a position, and its J
// keys are m words apart.  A value per phase (the profile, K22's scale) lives
// in an m-word buffer that is made raw (phase_values), smoothed in place
// (smooth_in_place), written out wrapped (write_wrapped) and read back while
// the keys are rewritten (sweep_phase_keys).  The helpers are for a whole
// workgroup of NT threads; each says which barrier it leaves to its caller.
#pragma once
#include "fm_radix_select.h"

namespace fm {

constexpr int kMaxCycles = kBatchBlocks;         // foremast_amd/ops/misc.py SEASONAL_MAX_CYCLES mirrors it
constexpr int kMaxPeriod = kRobustLdsKeys / 4;   // (J + 2) m <= kRobustLdsKeys with J >= 2

// compare-exchange: the smaller key first
__device__ __forceinline__ void cex(unsigned& a, unsigned& b) {
  const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

// The J keys col[0], col[m], ... of a phase sorted in registers by an odd-even
// transposition network, the missing key last: c = how many are finite, klo /
// kup their lower and upper middle (the missing key when c == 0).  load is
// applied to every word read (K26 masks the sign bit of its residual keys out).
template <class Load>
__device__ __forceinline__ int phase_middles(const unsigned* col, int m, int J, unsigned& klo, unsigned& kup,
                                             Load load) {
  unsigned s[kMaxCycles];
  int c = 0;
#pragma unroll
  for (int j = 0; j < kMaxCycles; ++j) {
    s[j] = j < J ? load(col[j * m]) : kMissing;
    c += s[j] != kMissing;
  }
#pragma unroll
  for (int r = 0; r < kMaxCycles; ++r) {
    if (r < J) {                                             // J rounds sort J keys; the padding is in place
#pragma unroll
      for (int i = r & 1; i + 1 < kMaxCycles; i += 2) cex(s[i], s[i + 1]);
    }
  }
  const int il = (c - 1) >> 1, iu = c >> 1;
  klo = kMissing;
  kup = kMissing;
#pragma unroll
  for (int j = 0; j < kMaxCycles; ++j) {
    klo = j == il ? s[j] : klo;
    kup = j == iu ? s[j] : kup;
  }
  return c;
}

// The two ways a key is read as a value: a sample (K14's and K20's keys), or a
// non-negative deviation whose key is its own bits (K22's second pass).
struct SampleKey {
  __device__ __forceinline__ float operator()(unsigned k) const { return dec_key(k); }
};
struct DeviationKey {
  __device__ __forceinline__ float operator()(unsigned k) const { return __uint_as_float(k); }
};

// buf[ph] = K13's median rule over the finite keys of phase ph (col0 = the
// word of key 0), NaN for a phase with none.  The keys are visible on entry;
// the caller puts a barrier between this and a read of buf.
template <int NT, class Decode, class Load>
__device__ __forceinline__ void phase_values(const unsigned* col0, int m, int J, float* buf, Decode value, Load load) {
  for (int ph = threadIdx.x; ph < m; ph += NT) {
    unsigned klo, kup;
    const int c = phase_middles(col0 + ph, m, J, klo, kup, load);
    buf[ph] = c == 0 ? quiet_nan() : 0.5f * value(klo) + 0.5f * value(kup);
  }
}
template <int NT, class Decode>
__device__ __forceinline__ void phase_values(const unsigned* col0, int m, int J, float* buf, Decode value) {
  phase_values<NT>(col0, m, J, buf, value, [](unsigned key) { return key; });
}

// buf[0..m) -> for each of this thread's phases the mean of the finite values
// within k phases, circular, summed from -k up and divided in fp64; NaN when
// none is finite.  The caller puts a barrier between this and a write of buf.
template <int NT, int NP>
__device__ __forceinline__ void smooth_phases(const float* buf, int m, int k, float (&sm)[NP]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int it = 0; it < NP; ++it) {
    const int ph = tid + it * NT;
    sm[it] = quiet_nan();
    if (ph < m) {
      double sum = 0.0;
      int cnt = 0;
      int q = ph - k;
      if (q < 0) q += m;
      for (int d = -k; d <= k; ++d) {
        const float v = buf[q];
        if (v == v) {
          sum += (double)v;
          ++cnt;
        }
        if (++q == m) q = 0;
      }
      if (cnt != 0) sm[it] = (float)(sum / (double)cnt);
    }
  }
}

// buf[ph] = f(ph, smoothed value of phase ph), in place: a thread keeps its
// phases' means in registers until every thread has read the raw values, so
// one buffer serves both.  The raw values are visible on entry (the caller's
// barrier after phase_values); the new ones are visible on return.
template <int NT, class F>
__device__ __forceinline__ void smooth_in_place(float* buf, int m, int k, F f) {
  constexpr int kPhases = (kMaxPeriod + NT - 1) / NT;        // most phases a thread takes
  const int tid = threadIdx.x;
  float sm[kPhases];
  smooth_phases<NT>(buf, m, k, sm);
  __syncthreads();                                           // every raw value read
#pragma unroll
  for (int it = 0; it < kPhases; ++it) {
    const int ph = tid + it * NT;
    if (ph < m) buf[ph] = f(ph, sm[it]);
  }
  __syncthreads();
}

// out[h] = f(buf[h mod m], h) for h < H.  buf is visible on entry.
template <int NT, class F>
__device__ __forceinline__ void write_wrapped(const float* buf, int m, int H, float* out, F f) {
  const int tid = threadIdx.x;
  const int stepm = NT % m;
  int ph = tid % m;
  for (int h = tid; h < H; h += NT) {
    out[h] = f(buf[ph], h);
    ph += stepm;
    if (ph >= m) ph -= m;
  }
}
template <int NT>
__device__ __forceinline__ void write_wrapped(const float* buf, int m, int H, float* out) {
  write_wrapped<NT>(buf, m, H, out, [](float v, int) { return v; });
}

// Every non-missing key of the nq quads becomes f(key, its phase).  Word wd
// holds span index wd - a: its phase, carried along a thread's quads instead
// of divided out.  What f reads (a per-phase buffer) is visible on entry; no
// barrier here: the caller reduces what f tallied (block_sum), which puts the
// last read of that buffer behind and makes the new keys visible.
template <int NT, class F>
__device__ __forceinline__ void sweep_phase_keys(uint4* keys, int nq, int a, int m, F f) {
  const int tid = threadIdx.x;
  const int stepm = (4 * NT) % m;
  int ph0 = (4 * tid - a) % m;                               // (the padding in front of the span: a remainder below zero)
  if (ph0 < 0) ph0 += m;
  for (int q = tid; q < nq; q += NT) {
    const uint4 v = keys[q];
    unsigned e[4] = {v.x, v.y, v.z, v.w};
    int ph = ph0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (e[j] != kMissing) e[j] = f(e[j], ph);
      if (++ph == m) ph = 0;
    }
    keys[q] = make_uint4(e[0], e[1], e[2], e[3]);
    ph0 += stepm;
    if (ph0 >= m) ph0 -= m;
  }
}

// ---------------------------------------------------------------------------
// Host side of the three entry points.

// What they all require: 2 <= J <= kMaxCycles whole cycles within the row,
// (J + 2) m within the LDS budget of K13, a smoothing window no longer than
// the period, and a row count and a row alignment the kernels can take.
inline bool seasonal_args_ok(const float* hist, int T, int64_t R, int m, int J, int k, int H) {
  return m >= 1 && J >= 2 && J <= kMaxCycles && (int64_t)(J + 2) * m <= kRobustLdsKeys && (int64_t)J * m <= T &&
         k >= 0 && 2 * (int64_t)k + 1 <= m && H >= 0 && R <= 0x7FFFFFFF && (((uintptr_t)hist) & 3) == 0;
}

// Dynamic LDS: the keys of the span plus up to 3 words in front, in whole
// quads; behind them `behind` per-phase buffers that are there always (K22's
// scale), and the profile when the bin array is too short for it.
inline size_t seasonal_lds_bytes(int J, int m, int behind) {
  return row_key_bytes(J * m) + (size_t)m * (size_t)(behind + (m > kBins ? 1 : 0)) * sizeof(float);
}

}  // namespace fm
