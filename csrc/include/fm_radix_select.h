// Exact order statistics of one row held by a workgroup: order-preserving
// uint32 keys, the loader that puts a row of them into LDS, an MSB-first radix
// selection over them, and the median / MAD / sigma routine built on it.
// What the robust kernels share is here, and stated here only: K13 and K18
// (robust_stats.hip: median and MAD of a row), K14 (seasonal_robust.hip: MAD
// of the residuals about a per-phase median profile), K15 (level_shift.hip:
// the band of the row, or of the segment behind a level shift found over the
// block medians) and K16 (trend_robust.hip: a line through the block medians,
// then median and MAD of the detrended row).  Two headers build on it:
// fm_seasonal_profile.h (the per-phase stages of K14, K20 and K22) and
// fm_repeated_median.h (the slope and detrend stages of K16 and K20).
//
// Keys: negatives have all bits flipped, non-negatives get the sign bit set.
// NaN / +-inf become the key 0xFFFFFFFF, which no finite value maps to and
// which sorts above every finite key, so ranks below the finite count n
// never see it and the keys need no compaction.  Non-negative floats (the
// deviations of phase two) are monotone as their own bits.
//
// Selection: the block's min and max key give the leading bits every finite
// key shares; below them, passes of up to 11 bits histogram the matching keys
// into 2,048 LDS bins (atomics; the lanes of a wave that share its first
// digit make one add), wave 0 scans the bins to the one holding rank k, and
// the prefix grows until all 32 bits are known.  For even n the upper middle is the same
// value when the last bin still holds rank k + 1, else the smallest key above.
#pragma once
#include "fm_common.h"

namespace fm {

constexpr int kDigitBits = 11;                 // bits settled per pass: three passes cover a key
constexpr int kBins = 1 << kDigitBits;
constexpr int kBinsPerLane = kBins / FM_WAVE;  // wave 0 scans the bins, a run of them per lane
static_assert(kBinsPerLane % 4 == 0, "a lane's bins are read as uint4");
// The longest row held in LDS: 52 KiB of keys, so that a workgroup's LDS (keys,
// 8 KiB of bins, reduction scratch) stays within the 64 KiB a launch gets
// without a raised limit.  foremast_amd/ops/misc.py ROBUST_LDS_KEYS mirrors it.
constexpr int kRobustLdsKeys = 13312;
constexpr size_t kLaunchLds = 64 * 1024;
constexpr unsigned kMissing = 0xFFFFFFFFu;

__device__ __forceinline__ unsigned enc_key(float x) {
  const unsigned b = __float_as_uint(x);
  if ((b & 0x7F800000u) == 0x7F800000u) return kMissing;   // NaN, +-inf
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float dec_key(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
// key of the deviation |x - c| of the sample with key k
__device__ __forceinline__ unsigned dev_key(unsigned k, float c) {
  return k == kMissing ? kMissing : __float_as_uint(fabsf(dec_key(k) - c));
}
// the median of a set from its lower and upper middle keys
__device__ __forceinline__ float mid_value(unsigned klo, unsigned kup) {
  return 0.5f * dec_key(klo) + 0.5f * dec_key(kup);
}
__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7FC00000u); }

// A reduction's result, the same in every lane, moved to scalar registers: the
// branches and loops it steers become scalar too.  For values the code waits
// for at once (a barrier or a branch follows), so the move hides no latency.
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ unsigned uniform(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ double uniform(double v) {
  return __hiloint2double(uniform(__double2hiint(v)), uniform(__double2loint(v)));
}

// LDS scratch of a workgroup's selections: one instance per kernel.  The bins
// are zero whenever no selection runs: the kernel clears them once, and every
// selection hands them back zeroed.
template <int NT>
struct SelectScratch {
  alignas(16) unsigned bins[kBins];
  unsigned sel[3];
  unsigned redu[NT / FM_WAVE];
  int redi[NT / FM_WAVE];
  double redd[NT / FM_WAVE];
  __device__ __forceinline__ void clear_bins() {             // no barrier
    for (int i = threadIdx.x; i < kBins; i += NT) bins[i] = 0u;
  }
};

template <int NT>
__device__ __forceinline__ unsigned block_min_u32(unsigned v, unsigned* scratch) {
  v = wave_min(v);
  if (lane_id() == 0) scratch[wave_id()] = v;
  __syncthreads();
  unsigned r = scratch[0];
#pragma unroll
  for (int w = 1; w < NT / FM_WAVE; ++w) r = r < scratch[w] ? r : scratch[w];
  __syncthreads();
  return r;
}

// The smallest and largest of a set of finite keys
struct KeyRange {
  unsigned min = kMissing, max = 0u;
  __device__ __forceinline__ void add(unsigned k) {
    min = k < min ? k : min;
    max = k > max ? k : max;
  }
};
// The threads' ranges folded over the workgroup in one round of barriers
// (redi, free between two block sums, carries the maxima)
template <int NT>
__device__ __forceinline__ KeyRange block_range(KeyRange r, SelectScratch<NT>* sc) {
  const unsigned lo = wave_min(r.min);
  if (lane_id() == 0) sc->redu[wave_id()] = lo;
  const unsigned hi = wave_max(r.max);
  if (lane_id() == 0) sc->redi[wave_id()] = (int)hi;
  __syncthreads();
  r.min = sc->redu[0];
  r.max = (unsigned)sc->redi[0];
#pragma unroll
  for (int w = 1; w < NT / FM_WAVE; ++w) {
    const unsigned a = sc->redu[w], b = (unsigned)sc->redi[w];
    r.min = a < r.min ? a : r.min;
    r.max = b > r.max ? b : r.max;
  }
  __syncthreads();
  return KeyRange{uniform(r.min), uniform(r.max)};
}

// What a thread gathers while keys are made: the finite count and the range
// (phase one), or the fp64 sum of the deviations and their range (phase two).
struct RowTally {
  int n = 0;
  KeyRange range;
  __device__ __forceinline__ void operator()(unsigned k) {
    if (k != kMissing) {
      ++n;
      range.add(k);
    }
  }
};
struct DevTally {
  double sum = 0.0;
  KeyRange range;
  __device__ __forceinline__ void operator()(unsigned d) {
    if (d != kMissing) {
      sum += (double)__uint_as_float(d);
      range.add(d);
    }
  }
};

// ---------------------------------------------------------------------------
// A row held in LDS at its global alignment: key i at word a + i with a =
// (address / 4) & 3 of the row's first sample, so that a 16-B global load and
// its 16-B LDS store are aligned together whatever the row's alignment (the
// row needs 4-byte alignment only), and a block of the row is a run of words.
// The words before and behind the row in its first and last quad hold the
// missing key, so a sweep of whole quads needs no mask.
__device__ __forceinline__ int row_word(const float* p) { return (int)(((uintptr_t)p >> 2) & 3u); }
constexpr int row_quads(int a, int T) { return (a + T + 3) >> 2; }
// dynamic LDS of a row of T keys at any alignment: up to 3 words in front, whole quads
constexpr size_t row_key_bytes(int T) { return (size_t)((T + 6) / 4) * sizeof(uint4); }

// The row p[0..T) -> keys in place, every key (the missing ones too) handed to
// track on the way.  No barrier: reduce what track gathered (block_sum)
// before the keys are read.
template <int NT, class Track>
__device__ __forceinline__ void load_row_keys(const float* p, int T, int a, uint4* keys, Track& track) {
  const int tid = threadIdx.x;
  const int nq = row_quads(a, T);
  unsigned* kw = reinterpret_cast<unsigned*>(keys);
  int head = (4 - a) & 3;                                    // samples before the 16-B boundary
  if (head > T) head = T;
  const int nb = (T - head) >> 2;
  const float4* b4 = reinterpret_cast<const float4*>(p + head);
  uint4* d4 = keys + ((a + head) >> 2);
  for (int q = tid; q < nb; q += NT) {
    const float4 x = b4[q];
    const uint4 key = make_uint4(enc_key(x.x), enc_key(x.y), enc_key(x.z), enc_key(x.w));
    track(key.x); track(key.y); track(key.z); track(key.w);
    d4[q] = key;
  }
  // every word the body leaves out lies in the first or the last quad: a
  // head / tail sample, or padding in front of / behind the row
  if (tid < (nq > 1 ? 8 : 4)) {
    const int w = tid < 4 ? tid : 4 * (nq - 1) + (tid - 4);
    const int i = w - a;
    if (i < head || i >= head + 4 * nb) {
      unsigned key = kMissing;
      if (i >= 0 && i < T) key = enc_key(p[i]);
      track(key);
      kw[w] = key;
    }
  }
}

// ---------------------------------------------------------------------------
// Key sources.  sweep(f) hands every key to f, the lanes of a wave together;
// to_deviations(c, f) turns the source into the keys of |x - c|, handing each
// to f, after which sweep yields those.

// The whole row in LDS: every quad, unmasked; the deviations replace the keys.
template <int NT>
struct LdsRow {
  uint4* k4;
  int nq;
  template <class F>
  __device__ __forceinline__ void sweep(F&& f) const {
    for (int q = threadIdx.x; q < nq; q += NT) {
      const uint4 v = k4[q];
      f(v.x); f(v.y); f(v.z); f(v.w);
    }
  }
  template <class F>
  __device__ __forceinline__ void to_deviations(float c, F&& f) {
    for (int q = threadIdx.x; q < nq; q += NT) {
      const uint4 v = k4[q];
      const uint4 d = make_uint4(dev_key(v.x, c), dev_key(v.y, c), dev_key(v.z, c), dev_key(v.w, c));
      f(d.x); f(d.y); f(d.z); f(d.w);
      k4[q] = d;
    }
  }
};

// The row in global memory (K13's rows beyond kRobustLdsKeys): encoded on the
// way, after to_deviations as deviations.
template <int NT>
struct GlobalRow {
  const float* p;
  int T;
  bool dev = false;
  float c = 0.f;
  template <class F>
  __device__ __forceinline__ void sweep(F&& f) const {
    for (int i = threadIdx.x; i < T; i += NT) {
      unsigned k = enc_key(p[i]);
      if (dev) k = dev_key(k, c);
      f(k);
    }
  }
  template <class F>
  __device__ __forceinline__ void to_deviations(float centre, F&& f) {
    dev = true;
    c = centre;
    sweep(f);
  }
};

// The words [lo, hi) of a row in LDS, any bounds (the row itself, or the
// segment behind a level shift).  The sweep reads whole quads and masks the
// words outside the run as missing, so every lane of a wave stays in it
// together.  The deviations are taken on the fly, which leaves the raw keys in
// place for a later selection.
template <int NT>
struct LdsSpan {
  const unsigned* kw;
  int lo, hi;
  bool dev = false;
  float c = 0.f;
  template <class F>
  __device__ __forceinline__ void sweep(F&& f) const {
    const uint4* k4 = reinterpret_cast<const uint4*>(kw);
    for (int q = (lo >> 2) + (int)threadIdx.x, qe = (hi + 3) >> 2; q < qe; q += NT) {
      const uint4 v = k4[q];
      const unsigned e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int w = 4 * q + j;
        unsigned k = (w >= lo && w < hi) ? e[j] : kMissing;
        if (dev) k = dev_key(k, c);
        f(k);
      }
    }
  }
  template <class F>
  __device__ __forceinline__ void to_deviations(float centre, F&& f) {
    dev = true;
    c = centre;
    sweep(f);
  }
};

// ---------------------------------------------------------------------------
// One key's count into bin d, for every lane with m set; the lanes of a wave
// call it together.  The lanes that share the first such lane's bin make one
// add (a row of ties would serialise 64 adds on one bin), the rest add singly.
// d is read only where m.
__device__ __forceinline__ void bin_add(unsigned* bins, bool m, unsigned d) {
  const unsigned long long act = __ballot(m);
  if (act == 0ull) return;
  const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)act) - 1);
  const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)d, leader);
  const bool same = m && d == d0;
  const unsigned long long grp = __ballot(same);
  if (lane_id() == leader) atomicAdd(&bins[d0], (unsigned)__popcll(grp));
  else if (m && !same) atomicAdd(&bins[d], 1u);
}

// Key of rank k (0-based) among the n finite keys of rk, all within r.
// cnt = how many keys equal it, resid = rank k inside that run.
template <int NT, class Keys>
__device__ __forceinline__ unsigned radix_select(const Keys& rk, KeyRange r, unsigned k, unsigned n,
                                                 SelectScratch<NT>* sc, unsigned& resid, unsigned& cnt) {
  unsigned* bins = sc->bins;
  int hi = r.min == r.max ? 32 : __clz(r.min ^ r.max);        // leading bits shared by every finite key
  unsigned pref = hi == 0 ? 0u : (hi == 32 ? r.min : (r.min & (~0u << (32 - hi))));
  cnt = n;
  while (hi < 32) {
    const int w = 32 - hi < kDigitBits ? 32 - hi : kDigitBits, shift = 32 - hi - w;
    const unsigned mask = hi == 0 ? 0u : (~0u << (32 - hi)), dm = (1u << w) - 1u;
    rk.sweep([&](unsigned key) { bin_add(bins, ((key ^ pref) & mask) == 0u, (key >> shift) & dm); });
    __syncthreads();
    if (wave_id() == 0) {
      const int l = lane_id();
      unsigned* mine = bins + l * kBinsPerLane;
      unsigned s = 0u;
#pragma unroll
      for (int j = 0; j < kBinsPerLane / 4; ++j) {
        const uint4 c = reinterpret_cast<const uint4*>(mine)[j];
        s += c.x + c.y + c.z + c.w;
      }
      const unsigned inc = wave_incl_sum(s), exc = inc - s;
      if (exc <= k && k < inc) {                               // one lane: the missing keys sort last
        unsigned rest = k - exc, b = 0u, cc = mine[0];
        while (rest >= cc) { rest -= cc; ++b; cc = mine[b]; }
        sc->sel[0] = pref | (((unsigned)(l * kBinsPerLane) + b) << shift);
        sc->sel[1] = rest;
        sc->sel[2] = cc;
      }
#pragma unroll
      for (int j = 0; j < kBinsPerLane / 4; ++j) reinterpret_cast<uint4*>(mine)[j] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    pref = sc->sel[0];                                       // (left in vector registers: the next sweep's
    k = sc->sel[1];                                          // first loads are issued before these arrive)
    cnt = sc->sel[2];
    hi += w;
  }
  resid = k;
  return pref;
}

// Lower and upper middle keys of the n finite keys of rk, all within r.
template <int NT, class Keys>
__device__ __forceinline__ void select_middles(const Keys& rk, KeyRange r, unsigned n, SelectScratch<NT>* sc,
                                               unsigned& lo, unsigned& up) {
  unsigned resid, cnt;
  lo = radix_select(rk, r, (n - 1u) >> 1, n, sc, resid, cnt);
  up = lo;
  if ((n & 1u) == 0u && resid + 1u >= cnt) {                   // the run of lo ends at the lower middle
    unsigned above = kMissing;
    rk.sweep([&](unsigned key) { if (key > lo && key < above) above = key; });
    up = block_min_u32<NT>(above, sc->redu);
  }
}

// sigma from the n >= 1 deviation keys that rk sweeps now, with their sum over
// the workgroup and this thread's share of their range: 1.4826 MAD, or 1.2533
// times the mean deviation where the MAD is zero.
template <int NT, class Keys>
__device__ __forceinline__ float mad_sigma(const Keys& rk, unsigned n, double sum, KeyRange mine,
                                           SelectScratch<NT>* sc) {
  unsigned dlo, dup;
  select_middles(rk, block_range(mine, sc), n, sc, dlo, dup);
  const float mad = 0.5f * __uint_as_float(dlo) + 0.5f * __uint_as_float(dup);
  return mad > 0.f ? 1.4826f * mad : 1.2533f * (float)(sum / (double)n);
}

// Median and sigma of the n >= 1 finite keys of rk, all within r.  rk is left
// as the deviations about the median.
template <int NT, class Keys>
__device__ __forceinline__ void median_sigma(Keys& rk, unsigned n, KeyRange r, SelectScratch<NT>* sc, float& center,
                                             float& sigma) {
  unsigned klo, kup;
  select_middles(rk, r, n, sc, klo, kup);
  center = mid_value(klo, kup);
  DevTally t;
  rk.to_deviations(center, t);
  sigma = mad_sigma(rk, n, uniform(block_sum<NT>(t.sum, sc->redd)), t.range, sc);
}

// ---------------------------------------------------------------------------
// Several ranks of one row (K24, quantile_robust.hip: the median and a rank in
// either tail).  All ranks share the prefix of the first pass, so its
// histogram, the pass in which every key makes an add, is built once and
// scanned once per rank; the passes below it are radix_select's, rank by rank.

// wave 0, after the bins of a pass are complete: the lane whose run of bins
// (mine; total s, exc keys in the lanes before it) holds rank k writes the
// grown prefix, the rank inside the bin and the bin's count to out[0..3)
__device__ __forceinline__ void pick_bin(const unsigned* mine, unsigned s, unsigned exc, unsigned k, unsigned pref,
                                         int shift, unsigned* out) {
  if (exc <= k && k < exc + s) {                               // one lane: the missing keys sort last
    unsigned rest = k - exc, b = 0u, cc = mine[0];
    while (rest >= cc) { rest -= cc; ++b; cc = mine[b]; }
    out[0] = pref | (((unsigned)(lane_id() * kBinsPerLane) + b) << shift);
    out[1] = rest;
    out[2] = cc;
  }
}

// Keys of the ranks rank[0..NR) (0-based, each below n) among the n finite
// keys of rk, all within r: key[j], with cnt[j] keys equal to it and resid[j]
// the rank inside that run.  sel is LDS, 3 NR words, free on entry.
template <int NT, int NR, class Keys>
__device__ __forceinline__ void radix_select_ranks(const Keys& rk, KeyRange r, const unsigned (&rank)[NR], unsigned n,
                                                   SelectScratch<NT>* sc, unsigned* sel, unsigned (&key)[NR],
                                                   unsigned (&resid)[NR], unsigned (&cnt)[NR]) {
  unsigned* bins = sc->bins;
  const int hi0 = r.min == r.max ? 32 : __clz(r.min ^ r.max);  // leading bits shared by every finite key
  const unsigned pref0 = hi0 == 0 ? 0u : (hi0 == 32 ? r.min : (r.min & (~0u << (32 - hi0))));
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    key[j] = pref0;
    resid[j] = rank[j];
    cnt[j] = n;
  }
  if (hi0 == 32) return;
  // every finite key carries pref0: the first pass counts them all, once
  const int w0 = 32 - hi0 < kDigitBits ? 32 - hi0 : kDigitBits;
  {
    const int shift = 32 - hi0 - w0;
    const unsigned dm = (1u << w0) - 1u;
    rk.sweep([&](unsigned k) { bin_add(bins, k != kMissing, (k >> shift) & dm); });
    __syncthreads();
    if (wave_id() == 0) {
      unsigned* mine = bins + lane_id() * kBinsPerLane;
      unsigned s = 0u;
#pragma unroll
      for (int i = 0; i < kBinsPerLane / 4; ++i) {
        const uint4 c = reinterpret_cast<const uint4*>(mine)[i];
        s += c.x + c.y + c.z + c.w;
      }
      const unsigned inc = wave_incl_sum(s), exc = inc - s;
#pragma unroll
      for (int j = 0; j < NR; ++j) pick_bin(mine, s, exc, rank[j], pref0, shift, sel + 3 * j);
#pragma unroll
      for (int i = 0; i < kBinsPerLane / 4; ++i) reinterpret_cast<uint4*>(mine)[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      key[j] = sel[3 * j];
      resid[j] = sel[3 * j + 1];
      cnt[j] = sel[3 * j + 2];
    }
  }
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    unsigned pref = key[j], k = resid[j], c = cnt[j];
    unsigned* out = sel + 3 * j;
    for (int hi = hi0 + w0; hi < 32;) {
      const int w = 32 - hi < kDigitBits ? 32 - hi : kDigitBits, shift = 32 - hi - w;
      const unsigned mask = ~0u << (32 - hi), dm = (1u << w) - 1u;
      rk.sweep([&](unsigned x) { bin_add(bins, ((x ^ pref) & mask) == 0u, (x >> shift) & dm); });
      __syncthreads();
      if (wave_id() == 0) {
        unsigned* mine = bins + lane_id() * kBinsPerLane;
        unsigned s = 0u;
#pragma unroll
        for (int i = 0; i < kBinsPerLane / 4; ++i) {
          const uint4 v = reinterpret_cast<const uint4*>(mine)[i];
          s += v.x + v.y + v.z + v.w;
        }
        const unsigned inc = wave_incl_sum(s);
        pick_bin(mine, s, inc - s, k, pref, shift, out);
#pragma unroll
        for (int i = 0; i < kBinsPerLane / 4; ++i) reinterpret_cast<uint4*>(mine)[i] = make_uint4(0u, 0u, 0u, 0u);
      }
      __syncthreads();
      pref = out[0];
      k = out[1];
      c = out[2];
      hi += w;
    }
    key[j] = pref;
    resid[j] = k;
    cnt[j] = c;
  }
}

// The upper middle key of n finite keys whose lower middle lo was selected
// with (resid, cnt): select_middles' second half.
template <int NT, class Keys>
__device__ __forceinline__ unsigned upper_middle(const Keys& rk, unsigned lo, unsigned n, unsigned resid, unsigned cnt,
                                                 SelectScratch<NT>* sc) {
  if ((n & 1u) != 0u || resid + 1u < cnt) return lo;           // the run of lo still holds the upper middle
  unsigned above = kMissing;
  rk.sweep([&](unsigned k) { if (k > lo && k < above) above = k; });
  return block_min_u32<NT>(above, sc->redu);
}

// ---------------------------------------------------------------------------
// The J blocks of L words that start at word lo of kw: f(key, block) for every
// word of the quads they touch, block outside [0, J) for a word in front of or
// behind them.  A thread walks its quads with the block and the position in it
// carried along; the lanes of a wave stay in a quad's four calls together.
template <int NT, class F>
__device__ __forceinline__ void sweep_blocks(const unsigned* kw, int lo, int L, int J, F f) {
  const uint4* k4 = reinterpret_cast<const uint4*>(kw);
  for (int q = (lo >> 2) + (int)threadIdx.x, qe = (lo + J * L + 3) >> 2; q < qe; q += NT) {
    const int u = 4 * q - lo;                                // position of the quad's word 0 among the blocks
    int blk, pos;
    if (u >= 0) {
      blk = u / L;
      pos = u - blk * L;
    } else {
      blk = -1;                                              // reaches block 0, position 0 after -u words
      pos = L + u;
    }
    const uint4 v = k4[q];
    const unsigned e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f(e[j], blk);
      if (++pos == L) {
        pos = 0;
        ++blk;
      }
    }
  }
}

// Finite keys of each of the J blocks -> cnt[0..J), zero on entry (atomics: a
// thread adds a run's count when the block changes).  No barrier.
template <int NT>
__device__ __forceinline__ void count_block_keys(const unsigned* kw, int lo, int L, int J, int* cnt) {
  int run = 0, at = -1;
  sweep_blocks<NT>(kw, lo, L, J, [&](unsigned key, int blk) {
    if (blk != at) {
      if (run != 0) atomicAdd(&cnt[at], run);
      run = 0;
      at = blk;
    }
    run += (blk >= 0 && blk < J && key != kMissing) ? 1 : 0;
  });
  if (run != 0) atomicAdd(&cnt[at], run);
}

// K13's median rule over v[0..c), sorted in place (one lane; c <= 16)
__device__ __forceinline__ float small_median(float* v, int c) {
  for (int i = 1; i < c; ++i) {
    const float x = v[i];
    int j = i - 1;
    while (j >= 0 && v[j] > x) {
      v[j + 1] = v[j];
      --j;
    }
    v[j + 1] = x;
  }
  return 0.5f * v[(c - 1) >> 1] + 0.5f * v[c >> 1];
}

// ---------------------------------------------------------------------------
// The middles of up to 16 blocks of a row, all selected in the same passes.
// Each block keeps its own prefix and residual rank; a pass settles
// kBatchBits of every block's prefix, block b counting into its own 128 bins
// at bins[128 b], which is exactly the kBins array of the one-row selection,
// so a pass costs one sweep of the blocks whatever J is.
constexpr int kBatchBlocks = 16;
constexpr int kBatchBits = 7;
constexpr int kBatchBins = 1 << kBatchBits;
constexpr int kBatchLanes = FM_WAVE / kBatchBlocks;          // wave 0 scans the bins, four lanes a block
constexpr int kBatchBinsPerLane = kBatchBins / kBatchLanes;
static_assert(kBatchBlocks * kBatchBins == kBins, "the blocks' bins fill the bin array");
static_assert(kBatchLanes == 4 && kBatchBinsPerLane % 4 == 0, "a block's scan is a prefix over four lanes");

struct BlockSel {
  unsigned n[kBatchBlocks];      // in: finite keys of the block, 0 = the block takes no part
  unsigned lo[kBatchBlocks];     // the prefix; out: the lower middle key
  unsigned up[kBatchBlocks];     // out: the upper middle key
  unsigned rank[kBatchBlocks];   // rank of the lower middle among the keys under the prefix
  unsigned cnt[kBatchBlocks];    // keys under the prefix
};

// Lower and upper middle keys of every block b < J with st->n[b] != 0: the J
// blocks of L words from word lo of kw (sweep_blocks), whose finite keys all
// lie within r.  st->n is set and visible on entry; bins[kBins] is zero on
// entry and on return.
template <int NT>
__device__ __forceinline__ void select_block_middles(const unsigned* kw, int lo, int L, int J, KeyRange r,
                                                     unsigned* bins, BlockSel* st) {
  const int tid = threadIdx.x;
  int hi = r.min == r.max ? 32 : __clz(r.min ^ r.max);        // leading bits shared by every finite key
  if (tid < kBatchBlocks) {
    const unsigned c = st->n[tid];
    st->lo[tid] = hi == 0 ? 0u : (hi == 32 ? r.min : (r.min & (~0u << (32 - hi))));
    st->up[tid] = kMissing;
    st->rank[tid] = c == 0u ? 0u : (c - 1u) >> 1;
    st->cnt[tid] = c;
  }
  __syncthreads();
  while (hi < 32) {
    const int w = 32 - hi < kBatchBits ? 32 - hi : kBatchBits, shift = 32 - hi - w;
    const unsigned mask = hi == 0 ? 0u : (~0u << (32 - hi)), dm = (1u << w) - 1u;
    // a thread keeps the prefix of the block it is in: it changes block once in L words
    int at = -2;
    unsigned pref = 0u;
    bool live = false;
    sweep_blocks<NT>(kw, lo, L, J, [&](unsigned key, int blk) {
      if (blk != at) {
        at = blk;
        live = blk >= 0 && blk < J && st->n[blk] != 0u;
        pref = live ? st->lo[blk] : 0u;
      }
      bin_add(bins, live && key != kMissing && ((key ^ pref) & mask) == 0u,
              ((unsigned)at << kBatchBits) | ((key >> shift) & dm));
    });
    __syncthreads();
    if (wave_id() == 0) {
      const int l = lane_id(), b = l / kBatchLanes, part = l % kBatchLanes;
      unsigned* mine = bins + l * kBatchBinsPerLane;
      unsigned s = 0u;
#pragma unroll
      for (int j = 0; j < kBatchBinsPerLane / 4; ++j) {
        const uint4 c = reinterpret_cast<const uint4*>(mine)[j];
        s += c.x + c.y + c.z + c.w;
      }
      const unsigned t1 = xor_lane<1>(s), t2 = xor_lane<2>(s + t1);
      const unsigned exc = ((part & 2) ? t2 : 0u) + ((part & 1) ? t1 : 0u);
      const unsigned k = st->rank[b], pref = st->lo[b];
      const bool live = b < J && st->n[b] != 0u;
      if (live && exc <= k && k < exc + s) {                   // one lane a block
        unsigned rest = k - exc, i = 0u, cc = mine[0];
        while (rest >= cc) { rest -= cc; ++i; cc = mine[i]; }
        st->lo[b] = pref | (((unsigned)(part * kBatchBinsPerLane) + i) << shift);
        st->rank[b] = rest;
        st->cnt[b] = cc;
      }
#pragma unroll
      for (int j = 0; j < kBatchBinsPerLane / 4; ++j) reinterpret_cast<uint4*>(mine)[j] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    hi += w;
  }
  // the upper middle of an even count: the lower one while its run still holds
  // rank + 1, else the smallest key above it, found for all blocks in one sweep
  bool any = false;
  for (int b = 0; b < J; ++b) any |= (st->n[b] & 1u) == 0u && st->n[b] != 0u && st->rank[b] + 1u >= st->cnt[b];
  if (any) {
    // a thread offers a key only below the smallest it has seen in the block it is in, and below the block's
    // minimum so far (a stale read of it only costs an atomic that changes nothing)
    int at = -2;
    unsigned low = 0u, best = 0u;
    sweep_blocks<NT>(kw, lo, L, J, [&](unsigned key, int blk) {
      if (blk != at) {
        at = blk;
        const unsigned c = blk >= 0 && blk < J ? st->n[blk] : 0u;
        const bool want = c != 0u && (c & 1u) == 0u && st->rank[blk] + 1u >= st->cnt[blk];
        low = want ? st->lo[blk] : kMissing;                 // (no key lies above the missing key)
        best = kMissing;
      }
      if (key > low && key < best) {
        best = key;
        if (key < st->up[at]) atomicMin(&st->up[at], key);
      }
    });
    __syncthreads();
  }
  if (tid < kBatchBlocks && st->up[tid] == kMissing) st->up[tid] = st->lo[tid];
  __syncthreads();
}

// ---------------------------------------------------------------------------
// The front K15 and K16 share: a row into LDS and the median of each of its
// J <= kBatchBlocks blocks of L samples (the last J * L columns, block 0 the
// oldest).
struct RowBlocks {
  int cnt[kBatchBlocks];         // finite samples of each block
  float median[kBatchBlocks];    // NaN for a block with fewer than max(L / 4, 1) of them
  BlockSel sel;
};

// Clears the bins, loads p[0..T) (load_row_keys at word a) and returns its
// finite count, the same in every thread; 0 = an empty row, and nothing else
// is done.  Otherwise range = the key range of the row, and rb->cnt[j] and
// rb->median[j] are set for j < J and visible.
template <int NT>
__device__ __forceinline__ int load_row_blocks(const float* p, int T, int a, int L, int J, uint4* keys,
                                               SelectScratch<NT>* sc, RowBlocks* rb, KeyRange& range) {
  const int tid = threadIdx.x;
  const unsigned* kw = reinterpret_cast<const unsigned*>(keys);
  sc->clear_bins();
  if (tid < kBatchBlocks) rb->cnt[tid] = 0;
  RowTally t;
  load_row_keys<NT>(p, T, a, keys, t);
  const int n = uniform(block_sum<NT>(t.n, sc->redi));       // (barriers: keys, bins and counts visible)
  if (n == 0) return 0;
  range = block_range(t.range, sc);
  const int lo = a + T - J * L;                              // word of block 0's first key
  if (J > 0) count_block_keys<NT>(kw, lo, L, J, rb->cnt);
  __syncthreads();
  if (tid < kBatchBlocks) {
    const int need = L / 4 > 1 ? L / 4 : 1;
    rb->sel.n[tid] = (tid < J && rb->cnt[tid] >= need) ? (unsigned)rb->cnt[tid] : 0u;
  }
  __syncthreads();
  if (J > 0) select_block_middles<NT>(kw, lo, L, J, range, sc->bins, &rb->sel);
  if (tid < kBatchBlocks) {
    const BlockSel& s = rb->sel;
    rb->median[tid] = s.n[tid] != 0u ? mid_value(s.lo[tid], s.up[tid]) : quiet_nan();
  }
  __syncthreads();
  return n;
}

}  // namespace fm
