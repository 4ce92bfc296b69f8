// Exact order statistics of one row held by a workgroup: order-preserving
// uint32 keys and an MSB-first radix selection over them.  Shared by K13
// (robust_stats.hip: median and MAD of a row), K14 (seasonal_robust.hip: MAD
// of the residuals about a per-phase median profile), K15 (level_shift.hip:
// medians of the blocks of a row and of the segment behind a level shift) and
// K16 (trend_robust.hip: the block medians selected together, then median and
// MAD of the detrended row).
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
// The fast path's longest row: 52 KiB of keys, so that a workgroup's LDS (keys,
// 8 KiB of bins, reduction scratch) stays under the 64 KiB a launch gets
// without a raised limit.  foremast_amd/ops/misc.py ROBUST_LDS_KEYS mirrors it.
constexpr int kRobustLdsKeys = 13312;
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

// The keys of one row: the LDS copy (LDS) or the row in global memory, encoded
// on the way (phase two: as deviations from the centre c).
template <int NT, bool LDS>
struct RowKeys {
  const float* p;
  int T;
  uint4* k4;
  int nq;
  bool dev;
  float c;
  template <class F>
  __device__ __forceinline__ void sweep(F f) const {
    if constexpr (LDS) {
      for (int q = threadIdx.x; q < nq; q += NT) {
        const uint4 v = k4[q];
        f(v.x); f(v.y); f(v.z); f(v.w);
      }
    } else {
      for (int i = threadIdx.x; i < T; i += NT) {
        unsigned k = enc_key(p[i]);
        if (dev) k = dev_key(k, c);
        f(k);
      }
    }
  }
};

// A run of keys in LDS with key i at word i: the words [lo, hi) of kw, any
// bounds (K15: the row sits at its global alignment, and a block of it or the
// segment behind a level shift starts at any word).  The sweep reads whole
// quads and masks the words outside the run as missing, so every lane of a
// wave stays in it together.  dev: the keys are taken as deviations from c
// on the fly, which leaves the raw keys in place for a later selection.
template <int NT>
struct SpanKeys {
  const unsigned* kw;
  int lo, hi;
  bool dev;
  float c;
  template <class F>
  __device__ __forceinline__ void sweep(F f) const {
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
};

// Key of rank k (0-based) among the n finite keys, all within [kmin, kmax].
// cnt = how many keys equal it, resid = rank k inside that run.  bins[kBins]
// is zero on entry and on return.  Keys is any source with a sweep(f) that
// hands every key to f, the lanes of a wave together.
template <int NT, class Keys>
__device__ __forceinline__ unsigned radix_select_keys(const Keys& rk, unsigned kmin, unsigned kmax, unsigned k,
                                                      unsigned n, unsigned* bins, unsigned* sel, unsigned& resid,
                                                      unsigned& cnt) {
  int hi = kmin == kmax ? 32 : __clz(kmin ^ kmax);            // leading bits shared by every finite key
  unsigned pref = hi == 0 ? 0u : (hi == 32 ? kmin : (kmin & (~0u << (32 - hi))));
  cnt = n;
  while (hi < 32) {
    const int w = 32 - hi < kDigitBits ? 32 - hi : kDigitBits, shift = 32 - hi - w;
    const unsigned mask = hi == 0 ? 0u : (~0u << (32 - hi)), dm = (1u << w) - 1u;
    rk.sweep([&](unsigned key) {
      const bool m = ((key ^ pref) & mask) == 0u;
      const unsigned d = (key >> shift) & dm;
      const unsigned long long act = __ballot(m);
      if (act == 0ull) return;
      // the lanes that share the first matching lane's digit make one add (a
      // row of ties would serialise 64 adds on one bin); the rest add singly
      const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)act) - 1);
      const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)d, leader);
      const bool same = m && d == d0;
      const unsigned long long grp = __ballot(same);
      if (lane_id() == leader) atomicAdd(&bins[d0], (unsigned)__popcll(grp));
      else if (m && !same) atomicAdd(&bins[d], 1u);
    });
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
        unsigned r = k - exc, b = 0u, cc = mine[0];
        while (r >= cc) { r -= cc; ++b; cc = mine[b]; }
        sel[0] = pref | (((unsigned)(l * kBinsPerLane) + b) << shift);
        sel[1] = r;
        sel[2] = cc;
      }
#pragma unroll
      for (int j = 0; j < kBinsPerLane / 4; ++j) reinterpret_cast<uint4*>(mine)[j] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    pref = sel[0];
    k = sel[1];
    cnt = sel[2];
    hi += w;
  }
  resid = k;
  return pref;
}

template <int NT, bool LDS>
__device__ __forceinline__ unsigned radix_select(const RowKeys<NT, LDS>& rk, unsigned kmin, unsigned kmax, unsigned k,
                                                 unsigned n, unsigned* bins, unsigned* sel, unsigned& resid,
                                                 unsigned& cnt) {
  return radix_select_keys<NT>(rk, kmin, kmax, k, n, bins, sel, resid, cnt);
}

// Lower and upper middle keys of the n finite keys.
template <int NT, class Keys>
__device__ __forceinline__ void select_middles_keys(const Keys& rk, unsigned kmin, unsigned kmax, unsigned n,
                                                    unsigned* bins, unsigned* sel, unsigned* redu, unsigned& lo,
                                                    unsigned& up) {
  unsigned resid, cnt;
  lo = radix_select_keys<NT>(rk, kmin, kmax, (n - 1u) >> 1, n, bins, sel, resid, cnt);
  up = lo;
  if ((n & 1u) == 0u && resid + 1u >= cnt) {                   // the run of lo ends at the lower middle
    unsigned above = kMissing;
    rk.sweep([&](unsigned key) { if (key > lo && key < above) above = key; });
    up = block_min_u32<NT>(above, redu);
  }
}
template <int NT, bool LDS>
__device__ __forceinline__ void select_middles(const RowKeys<NT, LDS>& rk, unsigned kmin, unsigned kmax, unsigned n,
                                               unsigned* bins, unsigned* sel, unsigned* redu, unsigned& lo,
                                               unsigned& up) {
  select_middles_keys<NT>(rk, kmin, kmax, n, bins, sel, redu, lo, up);
}

// ---------------------------------------------------------------------------
// A row held in LDS at its global alignment (K15, K16): key i at word a + i
// with a = (address / 4) & 3 of the row's first sample, so that a 16-B global
// load and its 16-B LDS store are aligned together whatever the row's
// alignment, and a block of the row is a run of words.  The words before and
// behind the row in its first and last quad hold the missing key.

// The row p[0..T) -> keys in place; adds this thread's finite count to n and
// folds its keys into [kmin, kmax].  No barrier: reduce n (block_sum) before
// the keys are read.
template <int NT>
__device__ __forceinline__ void load_row_keys(const float* p, int T, int a, uint4* keys, int& n, unsigned& kmin,
                                              unsigned& kmax) {
  const int tid = threadIdx.x;
  const int nq = (a + T + 3) >> 2;
  unsigned* kw = reinterpret_cast<unsigned*>(keys);
  auto track = [&](unsigned k) {
    if (k != kMissing) {
      ++n;
      kmin = k < kmin ? k : kmin;
      kmax = k > kmax ? k : kmax;
    }
  };
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

// Median and sigma (1.4826 MAD, or the mean-deviation fallback) of the n >= 1
// finite keys in words [lo, hi) of kw, all within [kmin, kmax].
template <int NT>
__device__ __forceinline__ void span_stats(const unsigned* kw, int lo, int hi, unsigned n, unsigned kmin, unsigned kmax,
                                           unsigned* bins, unsigned* sel, unsigned* redu, double* redd, float& center,
                                           float& sigma) {
  SpanKeys<NT> sk{kw, lo, hi, false, 0.f};
  unsigned klo, kup;
  select_middles_keys<NT>(sk, kmin, kmax, n, bins, sel, redu, klo, kup);
  center = 0.5f * dec_key(klo) + 0.5f * dec_key(kup);
  sk.dev = true;
  sk.c = center;
  double sum = 0.0;
  unsigned dmin = kMissing, dmax = 0u;
  sk.sweep([&](unsigned d) {
    if (d != kMissing) {
      sum += (double)__uint_as_float(d);
      dmin = d < dmin ? d : dmin;
      dmax = d > dmax ? d : dmax;
    }
  });
  sum = block_sum<NT>(sum, redd);
  dmin = block_min_u32<NT>(dmin, redu);
  dmax = ~block_min_u32<NT>(~dmax, redu);
  unsigned dlo, dup;
  select_middles_keys<NT>(sk, dmin, dmax, n, bins, sel, redu, dlo, dup);
  const float mad = 0.5f * __uint_as_float(dlo) + 0.5f * __uint_as_float(dup);
  sigma = mad > 0.f ? 1.4826f * mad : 1.2533f * (float)(sum / (double)n);
}

// ---------------------------------------------------------------------------
// The middles of up to 16 blocks of a row, all selected in the same passes
// (K16).  Each block keeps its own prefix and residual rank; a pass settles
// kBatchBits of every block's prefix, block b counting into its own 128 bins
// at bins[128 b], which is exactly the kBins array of the one-row selection.
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
// lie within [kmin, kmax].  st->n is set and visible on entry; bins[kBins] is
// zero on entry and on return.
template <int NT>
__device__ __forceinline__ void select_block_middles(const unsigned* kw, int lo, int L, int J, unsigned kmin,
                                                     unsigned kmax, unsigned* bins, BlockSel* st) {
  const int tid = threadIdx.x;
  int hi = kmin == kmax ? 32 : __clz(kmin ^ kmax);            // leading bits shared by every finite key
  if (tid < kBatchBlocks) {
    const unsigned c = st->n[tid];
    st->lo[tid] = hi == 0 ? 0u : (hi == 32 ? kmin : (kmin & (~0u << (32 - hi))));
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
      const bool m = live && key != kMissing && ((key ^ pref) & mask) == 0u;
      const unsigned d = ((unsigned)at << kBatchBits) | ((key >> shift) & dm);       // (read only where m)
      const unsigned long long act = __ballot(m);
      if (act == 0ull) return;
      // as in radix_select_keys: the lanes that share the first matching
      // lane's bin make one add, the rest add singly
      const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)act) - 1);
      const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)d, leader);
      const bool same = m && d == d0;
      const unsigned long long grp = __ballot(same);
      if (lane_id() == leader) atomicAdd(&bins[d0], (unsigned)__popcll(grp));
      else if (m && !same) atomicAdd(&bins[d], 1u);
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
        unsigned r = k - exc, i = 0u, cc = mine[0];
        while (r >= cc) { r -= cc; ++i; cc = mine[i]; }
        st->lo[b] = pref | (((unsigned)(part * kBatchBinsPerLane) + i) << shift);
        st->rank[b] = r;
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

}  // namespace fm
