// The LDS sort of the 256-thread workgroup kernels that hold the two samples of
// a row as order-preserving keys: K21 (pairwise_wide.hip, the rank tests),
// K28 (pairwise_effect_wide.hip, the effect-size gate) and K29
// (pairwise_pods.hip, the per-pod test), and the counting searches and the
// workgroup sums K21 and K29 rank a sorted run with.
//
// A bitonic network whose comparators all put the smaller key at the lower
// index (the first step of a merge pairs i with i ^ (size - 1), the rest i
// with i + stride).  With every comparator pointing the same way a virtual
// tail of maximal keys never moves, so a side of any length n sorts as the
// next power of two with the comparators that touch the tail left out: no
// padding to a power of two in LDS (8191 + 1 fits like 4096 + 4096).  A side
// is padded to whole chunks of 16 keys with the missing key; sizes up to 16
// and the strides 8..1 of every later merge run in the registers of the
// thread that holds the chunk, the other steps are four comparators per
// thread on uint4.
#pragma once
#include "fm_radix_select.h"

namespace fm {

constexpr int kWideNT = 256;
constexpr int kPairwiseWideMax = 8192;      // mirrored as PAIRWISE_WIDE_MAX in foremast_amd/ops/canary.py
constexpr int kChunk = 16;                  // keys a thread sorts in registers
constexpr int kWideWords = kPairwiseWideMax + 2 * kChunk;   // both sides padded to whole chunks
constexpr int kWideWaves = kWideNT / FM_WAVE;

// One side in LDS: n16 words (a multiple of kChunk), P = the power of two the
// network is laid out for (>= n16; 0 for an empty side).
struct Side {
  unsigned* k;
  int n16;
  int P;
};

__device__ __forceinline__ int chunks_up(int n) { return (n + kChunk - 1) & ~(kChunk - 1); }
__device__ __forceinline__ int pow2_up(int n) { return n <= 0 ? 0 : (n <= 1 ? 1 : 1 << (32 - __clz(n - 1))); }

__device__ __forceinline__ void cx(unsigned& a, unsigned& b) {
  const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

// strides N/2 .. 1 of a merge over N keys in registers
template <int N>
__device__ __forceinline__ void merge_tail_regs(unsigned (&e)[N]) {
#pragma unroll
  for (int s = N >> 1; s > 0; s >>= 1)
#pragma unroll
    for (int i = 0; i < N; ++i)
      if ((i & s) == 0) cx(e[i], e[i + s]);
}
template <int N>
__device__ __forceinline__ void sort_regs(unsigned (&e)[N]) {
#pragma unroll
  for (int size = 2; size <= N; size <<= 1) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int j = i ^ (size - 1);
      if (j > i) cx(e[i], e[j]);
    }
#pragma unroll
    for (int s = size >> 2; s > 0; s >>= 1)
#pragma unroll
      for (int i = 0; i < N; ++i)
        if ((i & s) == 0) cx(e[i], e[i + s]);
  }
}

// every chunk of the side through f in registers
template <class F>
__device__ __forceinline__ void chunk_pass(Side s, F f) {
  uint4* k4 = reinterpret_cast<uint4*>(s.k);
  for (int q = threadIdx.x; q * kChunk < s.n16; q += kWideNT) {
    unsigned e[kChunk];
#pragma unroll
    for (int j = 0; j < kChunk / 4; ++j) {
      const uint4 v = k4[q * (kChunk / 4) + j];
      e[4 * j] = v.x; e[4 * j + 1] = v.y; e[4 * j + 2] = v.z; e[4 * j + 3] = v.w;
    }
    f(e);
#pragma unroll
    for (int j = 0; j < kChunk / 4; ++j)
      k4[q * (kChunk / 4) + j] = make_uint4(e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]);
  }
}

// first step of the merge of size 2^lsz >= 32: i with i ^ (size - 1).  Four
// comparators a thread: i0..i0+3 against jb+3..jb, both quads aligned.
__device__ __forceinline__ void flip_step(Side s, int lsz) {
  const int size = 1 << lsz;
  if (size > s.P) return;
  uint4* k4 = reinterpret_cast<uint4*>(s.k);
  const int half = size >> 1;
  for (int g = threadIdx.x; g < (s.P >> 3); g += kWideNT) {
    const int c = 4 * g, blk = c >> (lsz - 1), off = c & (half - 1);
    const int i0 = (blk << lsz) + off, jb = (blk << lsz) + size - 4 - off;
    if (i0 >= s.n16) break;
    if (jb >= s.n16) continue;               // the partners lie in the virtual tail
    uint4 a = k4[i0 >> 2], b = k4[jb >> 2];
    cx(a.x, b.w); cx(a.y, b.z); cx(a.z, b.y); cx(a.w, b.x);
    k4[i0 >> 2] = a;
    k4[jb >> 2] = b;
  }
}
// a later step of a merge: i with i + st, st >= kChunk
__device__ __forceinline__ void stride_step(Side s, int st) {
  uint4* k4 = reinterpret_cast<uint4*>(s.k);
  for (int g = threadIdx.x; g < (s.P >> 3); g += kWideNT) {
    const int c = 4 * g;
    const int i0 = 2 * c - (c & (st - 1)), j0 = i0 + st;
    if (i0 >= s.n16) break;
    if (j0 >= s.n16) continue;
    uint4 a = k4[i0 >> 2], b = k4[j0 >> 2];
    cx(a.x, b.x); cx(a.y, b.y); cx(a.z, b.z); cx(a.w, b.w);
    k4[i0 >> 2] = a;
    k4[j0 >> 2] = b;
  }
}

// Both sides sorted ascending in place, in the same steps (one barrier a
// step for the two).  Keys visible on entry; sorted and visible on return.
__device__ __forceinline__ void sort_sides(Side a, Side b) {
  chunk_pass(a, [](unsigned (&e)[kChunk]) { sort_regs(e); });
  chunk_pass(b, [](unsigned (&e)[kChunk]) { sort_regs(e); });
  __syncthreads();
  const int pmax = a.P > b.P ? a.P : b.P;
  for (int lsz = 5; (1 << lsz) <= pmax; ++lsz) {
    flip_step(a, lsz);
    flip_step(b, lsz);
    __syncthreads();
    for (int st = 1 << (lsz - 2); st >= kChunk; st >>= 1) {
      if ((1 << lsz) <= a.P) stride_step(a, st);
      if ((1 << lsz) <= b.P) stride_step(b, st);
      __syncthreads();
    }
    if ((1 << lsz) <= a.P) chunk_pass(a, [](unsigned (&e)[kChunk]) { merge_tail_regs(e); });
    if ((1 << lsz) <= b.P) chunk_pass(b, [](unsigned (&e)[kChunk]) { merge_tail_regs(e); });
    __syncthreads();
  }
}

// #(k[0..n) < x) and #(k[0..n) <= x) of a sorted run
__device__ __forceinline__ int count_lt(const unsigned* k, int n, unsigned x) {
  int lo = 0, len = n;
  while (len > 0) {
    const int half = len >> 1;
    const bool r = k[lo + half] < x;
    lo = r ? lo + half + 1 : lo;
    len = r ? len - half - 1 : half;
  }
  return lo;
}
__device__ __forceinline__ int count_le(const unsigned* k, int n, unsigned x) {
  int lo = 0, len = n;
  while (len > 0) {
    const int half = len >> 1;
    const bool r = k[lo + half] <= x;
    lo = r ? lo + half + 1 : lo;
    len = r ? len - half - 1 : half;
  }
  return lo;
}

// N sums over the workgroup behind one pair of barriers
template <int N, typename T>
__device__ __forceinline__ void block_sums(T (&v)[N], T (*scratch)[kWideWaves]) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const T w = wave_sum(v[j]);
    if (lane_id() == 0) scratch[j][wave_id()] = w;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < N; ++j) {
    T r = 0;
#pragma unroll
    for (int w = 0; w < kWideWaves; ++w) r += scratch[j][w];
    v[j] = r;
  }
  __syncthreads();
}

// The key a sample is sorted by: -0.0 is made +0.0 first, so it ties with 0.0
// as a float compare has it; NaN / +-inf become the missing key.
__device__ __forceinline__ unsigned sample_key(float x) { return enc_key(x == 0.f ? 0.f : x); }

}  // namespace fm
