// Exact order statistics of one row held by a workgroup: order-preserving
// uint32 keys and an MSB-first radix selection over them.  Shared by K13
// (robust_stats.hip: median and MAD of a row), K14 (seasonal_robust.hip: MAD
// of the residuals about a per-phase median profile) and K15 (level_shift.hip:
// medians of the blocks of a row and of the segment behind a level shift).
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

}  // namespace fm
