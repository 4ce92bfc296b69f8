// Register-resident statistics of one history row (K1), shared by
// hist_stats.hip (stats_decide_kernel, hist_stats_kernel) and the history
// role of tick_front.hip, plus the host-side choice of the NV instantiation.
#pragma once
#include <type_traits>

#include "fm_common.h"

using namespace fm;

// Mean / population std / finite count of one history row, computed by a
// 256-thread block with the row held in registers (NV float4 per thread).
// Fast path for rows without missing samples (the common case): the plain
// sum is computed with packed f32 adds (v_pk_add_f32, 2 elements per
// instruction) and is finite iff every sample is; only a non-finite sum sends
// the block to the masked per-element path.  Per element that is ~0.75 VALU
// instructions instead of ~8, which leaves the CU's issue slots to the
// pairwise kernel running concurrently on the side stream.
// The row is read through a buffer resource (wave-uniform, in SGPRs) with the
// thread's 16 B as the VGPR offset and the 4-KB step as a scalar offset: no
// 64-bit VGPR address per load, and the range check returns zeros past the
// row (no clamp).  109 -> 72 VGPRs for the history kernel; the front kernel
// drops from 111 to 87 (the p-value call now bounds it): five waves per SIMD
// instead of four, i.e. one pairwise + four history workgroups per CU.
template <int NV>
__device__ __forceinline__ void block_row_stats(const float* __restrict__ hrow, int T, double* red, int* redi,
                                                float& mf, float& sd, int& n) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  typedef float nt4 __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x;
  const int nq = (T + 3) >> 2;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)hrow, (short)0, nq * 16, 0x00020000);
  nt4 q[NV];
  f2 acc = {0.f, 0.f};
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int qi = tid + j * 256;
    nt4 v = __builtin_bit_cast(nt4, __builtin_amdgcn_raw_buffer_load_b128(rs, tid * 16, j * 4096, 2 /* nt */));
    if (qi == nq - 1) {
      const int e0 = qi * 4;
      if (e0 + 1 >= T) v.y = 0.f;
      if (e0 + 2 >= T) v.z = 0.f;
      if (e0 + 3 >= T) v.w = 0.f;
    }
    q[j] = v;
    acc += v.xy;
    acc += v.zw;
  }
  const double tot = block_sum<256>((double)acc.x + (double)acc.y, red);
  if (isfinite(tot)) {
    n = T;
    mf = (float)(tot / T);
    const f2 mm = {mf, mf};
    f2 a2 = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int qi = tid + j * 256;
      if (qi < nq - 1) {
        const f2 d0 = q[j].xy - mm, d1 = q[j].zw - mm;
        a2 += d0 * d0;
        a2 += d1 * d1;
      } else if (qi == nq - 1) {
        const int e0 = qi * 4;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (e0 + c < T) { const float d = q[j][c] - mf; a2.x += d * d; }
      }
    }
    const double sst = block_sum<256>((double)a2.x + (double)a2.y, red);
    sd = (float)sqrt(sst / n);
    return;
  }
  f2 ms = {0.f, 0.f};
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int e0 = (tid + j * 256) * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float x = q[j][c];
      const bool ok = e0 + c < T && isfinite(x);
      cnt += ok ? 1 : 0;
      ms[c & 1] += ok ? x : 0.f;
    }
  }
  const double t2 = block_sum<256>((double)ms.x + (double)ms.y, red);
  n = block_sum<256>(cnt, redi);
  mf = n > 0 ? (float)(t2 / n) : 0.f;
  f2 a2 = {0.f, 0.f};
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int e0 = (tid + j * 256) * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float x = q[j][c];
      const float d = (e0 + c < T && isfinite(x)) ? x - mf : 0.f;
      a2[c & 1] += d * d;
    }
  }
  const double sst = block_sum<256>((double)a2.x + (double)a2.y, red);
  sd = n > 0 ? (float)sqrt(sst / n) : 0.f;
}

// History row of logical row `row`: identity, or a slot of the brain's
// device-resident history store (engine/resident.py) when a row map is given.
// The row index is wave-uniform, so the map read is one scalar load: it goes
// through the constant address space (no launch that reads a map writes it),
// which a kernel whose pointers arrive in a struct (tick_front.hip) cannot
// say with a `const __restrict__` parameter -- there the read was a vector
// load and a readfirstlane per row.
__device__ __forceinline__ int64_t hist_row(const int* __restrict__ rowmap, int64_t row) {
  typedef const __attribute__((address_space(4))) int* const_map;
  return rowmap != nullptr ? (int64_t)((const_map)rowmap)[row] : row;
}

// ---------------------------------------------------------------------------
// Per-row statistics cache.  A static history row is written once and then
// re-examined every tick, so its (mean, std, n) are kept per PHYSICAL row:
// cache[p * 3 ..] holds the three floats block_row_stats produced, valid[p]
// the tag of the launch that produced them (the view length T, never 0;
// 0 = invalid: whoever writes a row clears its word on the same stream).
//
// Two logical rows may map to one physical row, so a workgroup may meet an
// entry that another workgroup of the same launch is writing.  Two cases:
//   * a launch that tests validity words (hist_scan_cached) publishes each
//     word with a release store and reads it with an acquire load, both at
//     agent scope (the L2s of the XCDs are not coherent for plain accesses):
//     a reader that sees the tag also sees the three floats written before
//     it; a reader that does not computes the row itself and stores the same
//     bits (same code, same input), so two writers cannot disagree;
//   * a launch that takes every row as a miss never reads the cache, so its
//     entries need no order among themselves (publish = false: plain stores;
//     a release per row, i.e. an L2 write-back, made the streaming tick 7x
//     slower: 4.10 vs 0.546 ms at 80k rows); duplicates again store the same
//     bits.
// Across launches the kernel boundary orders everything.
// K18 (robust_stats.hip) keeps a row's (median, sigma, n) in a second cache of
// the same layout under the same protocol, both forms.
// ---------------------------------------------------------------------------
template <bool publish>
__device__ __forceinline__ void row_cache_put(float* __restrict__ cache, unsigned* __restrict__ valid, int64_t p,
                                              unsigned tag, float mf, float sd, float nf) {
  cache[p * 3 + 0] = mf;
  cache[p * 3 + 1] = sd;
  cache[p * 3 + 2] = nf;
  if (publish) __hip_atomic_store(valid + p, tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  else valid[p] = tag;
}

// One history row by a 256-thread workgroup: reduce the physical row of
// logical row `row`, write hs[row * 3 ..] and, when a cache is given, record
// the three floats in it (publish: row_cache_put's two forms above).
template <int NV, bool publish>
__device__ __forceinline__ void hist_row_emit(const float* __restrict__ hist, int64_t ld_h, int T,
                                              float* __restrict__ hs, const int* __restrict__ rowmap,
                                              float* __restrict__ cache, unsigned* __restrict__ valid, int64_t row,
                                              double* red, int* redi) {
  float mf, sd;
  int n;
  const int64_t p = hist_row(rowmap, row);
  block_row_stats<NV>(hist + p * ld_h, T, red, redi, mf, sd, n);
  if (threadIdx.x == 0) {
    hs[row * 3 + 0] = mf;
    hs[row * 3 + 1] = sd;
    hs[row * 3 + 2] = (float)n;
    if (cache != nullptr) row_cache_put<publish>(cache, valid, p, (unsigned)T, mf, sd, (float)n);
  }
}

// Hit scan of the history rows {wg, wg + nwg, wg + 2 nwg, ..} by one
// 256-thread workgroup: one row per thread, hits are copied (12 bytes) and the
// misses of each 256-row pass are compacted into an LDS list, over which the
// workgroup-wide reduction then runs.  Rows are dealt round-robin, so a run of
// consecutive invalid rows (a batch of new jobs) spreads over all workgroups.
// cache == nullptr: every row is a miss and nothing is recorded.
template <int NV>
__device__ __forceinline__ void hist_scan_cached(const float* __restrict__ hist, int64_t ld_h, int T, int64_t R,
                                                 float* __restrict__ hs, const int* __restrict__ rowmap,
                                                 float* __restrict__ cache, unsigned* __restrict__ valid, int64_t wg,
                                                 int64_t nwg, double* red, int* redi, int* s_list, int* s_cnt) {
  const int tid = threadIdx.x;
  const unsigned tag = (unsigned)T;
  const int64_t nk = wg < R ? (R - wg + nwg - 1) / nwg : 0;   // rows of this workgroup
  for (int64_t k0 = 0; k0 < nk; k0 += 256) {
    if (tid == 0) *s_cnt = 0;
    __syncthreads();
    if (k0 + tid < nk) {
      const int64_t row = wg + (k0 + tid) * nwg;
      const int64_t p = hist_row(rowmap, row);
      if (cache != nullptr && __hip_atomic_load(valid + p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == tag) {
        hs[row * 3 + 0] = cache[p * 3 + 0];
        hs[row * 3 + 1] = cache[p * 3 + 1];
        hs[row * 3 + 2] = cache[p * 3 + 2];
      } else {
        s_list[atomicAdd(s_cnt, 1)] = tid;
      }
    }
    __syncthreads();
    const int nm = *s_cnt;
    for (int i = 0; i < nm; ++i) {
      const int64_t row = wg + (k0 + __builtin_amdgcn_readfirstlane(s_list[i])) * nwg;
      hist_row_emit<NV, true>(hist, ld_h, T, hs, rowmap, cache, valid, row, red, redi);
    }
    __syncthreads();   // the list is rebuilt by the next pass
  }
}

// Host side: the block_row_stats<NV> instantiation for a history row of nq
// float4 (256 threads x NV float4 hold the row).  f is a generic lambda called
// with std::integral_constant<int, NV>; hipErrorInvalidValue past 256 x 16.
template <class F>
inline int row_stats_dispatch_nv(int nq, F&& f) {
  if (nq <= 256 * 2) f(std::integral_constant<int, 2>{});
  else if (nq <= 256 * 4) f(std::integral_constant<int, 4>{});
  else if (nq <= 256 * 8) f(std::integral_constant<int, 8>{});
  else if (nq <= 256 * 10) f(std::integral_constant<int, 10>{});
  else if (nq <= 256 * 12) f(std::integral_constant<int, 12>{});
  else if (nq <= 256 * 16) f(std::integral_constant<int, 16>{});
  else return (int)hipErrorInvalidValue;
  return 0;
}
