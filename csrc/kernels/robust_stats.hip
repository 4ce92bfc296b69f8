// K13 robust history statistics: per-row median and MAD (Hampel band) by an
// exact MSB-first radix selection, one 512-thread workgroup per row.
//
// The row is read from HBM once and kept in LDS as the keys of
// fm_radix_select.h (load_row_keys); median_sigma selects the median,
// overwrites the keys with the bits of |x - centre|, sums them in fp64 and
// selects again.  Rows longer than kRobustLdsKeys run the same passes
// re-reading global memory (no limit on T; not a fast path).  The contract is
// foremast_amd/ops/misc.py ref_robust_stats; centre and MAD are exact.
//
// K18 (fm_robust_stats_cached) is the same row computation over the rows of a
// device-resident history store: logical row r reads physical row rowmap[r],
// and the three floats are kept per physical row in a row-statistics cache
// (fm_row_stats.h: layout, tags and the release / acquire protocol), so a
// static history is selected once and costs 12 bytes per tick afterwards.
#include "fm_common.h"
#include "fm_radix_select.h"
#include "fm_robust_row.h"   // tallied_stats, robust_row_stats
#include "fm_row_stats.h"

using namespace fm;

namespace {

constexpr int kRobustThreads = 512;
// workgroups of K18's scan form when the caller names none: two per CU of a
// 256-CU part, which is what the LDS of a 7-day row lets a CU hold
constexpr int kRobustScanBlocks = 512;

// K18 holds the most static LDS of the family: the scratch and the misses of a
// scan pass (K13 has the scratch alone)
static_assert(sizeof(SelectScratch<kRobustThreads>) + (kRobustThreads + 1) * sizeof(int) +
                      row_key_bytes(kRobustLdsKeys) <= kLaunchLds, "the longest LDS row fits a launch");

template <int NT, bool LDS>
__global__ __launch_bounds__(NT) void robust_stats_kernel(const float* __restrict__ hist, int64_t ld, int T, int64_t R,
                                                          float* __restrict__ out /*[R,3]*/) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_keys[];
  __shared__ SelectScratch<NT> s_sc;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  s_sc.clear_bins();
  float center, sigma;
  int n;
  robust_row_stats<NT, LDS>(hist + row * ld, T, s_keys, &s_sc, center, sigma, n);
  if (tid == 0) {
    out[row * 3 + 0] = center;
    out[row * 3 + 1] = sigma;
    out[row * 3 + 2] = (float)n;
  }
}

// K18.  scan == 0: every logical row is computed, a workgroup per row (the
// grid may be capped: rows are then dealt round-robin), no validity word is
// read and the entries are recorded with plain stores (cache may be null:
// nothing is recorded).  scan != 0: the form of hist_scan_cached
// (fm_row_stats.h) at 512 threads: each thread tests one row's word with an
// agent-scope acquire load and copies the 12 bytes on a hit; the misses of a
// pass are compacted into an LDS list and computed one by one by the whole
// workgroup, thread 0 publishing each with the release store.
template <int NT, bool LDS>
__global__ __launch_bounds__(NT) void robust_stats_cached_kernel(const float* __restrict__ hist, int64_t ld, int T,
                                                                 int64_t R, float* __restrict__ out /*[R,3]*/,
                                                                 const int* __restrict__ rowmap,
                                                                 float* __restrict__ cache,
                                                                 unsigned* __restrict__ valid, int scan) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_keys[];
  __shared__ SelectScratch<NT> s_sc;
  __shared__ int s_list[NT];                                 // the misses of a scan pass
  __shared__ int s_cnt;
  const int tid = threadIdx.x;
  const unsigned tag = (unsigned)T;
  const int64_t wg = blockIdx.x, nwg = gridDim.x;
  // zero once: every selection hands the bins back zeroed, and a row without
  // a finite sample never touches them
  s_sc.clear_bins();
  float center, sigma;
  int n;
  if (!scan) {
    for (int64_t row = wg; row < R; row += nwg) {
      const int64_t p = hist_row(rowmap, row);
      robust_row_stats<NT, LDS>(hist + p * ld, T, s_keys, &s_sc, center, sigma, n);
      if (tid == 0) {
        out[row * 3 + 0] = center;
        out[row * 3 + 1] = sigma;
        out[row * 3 + 2] = (float)n;
        if (cache != nullptr) row_cache_put<false>(cache, valid, p, tag, center, sigma, (float)n);
      }
    }
    return;
  }
  const int64_t nk = wg < R ? (R - wg + nwg - 1) / nwg : 0;   // rows of this workgroup
  for (int64_t k0 = 0; k0 < nk; k0 += NT) {
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    if (k0 + tid < nk) {
      const int64_t row = wg + (k0 + tid) * nwg;
      const int64_t p = hist_row(rowmap, row);
      if (__hip_atomic_load(valid + p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == tag) {
        out[row * 3 + 0] = cache[p * 3 + 0];
        out[row * 3 + 1] = cache[p * 3 + 1];
        out[row * 3 + 2] = cache[p * 3 + 2];
      } else {
        s_list[atomicAdd(&s_cnt, 1)] = tid;
      }
    }
    __syncthreads();
    const int nm = s_cnt;
    for (int i = 0; i < nm; ++i) {
      const int64_t row = wg + (k0 + __builtin_amdgcn_readfirstlane(s_list[i])) * nwg;
      const int64_t p = hist_row(rowmap, row);
      robust_row_stats<NT, LDS>(hist + p * ld, T, s_keys, &s_sc, center, sigma, n);
      if (tid == 0) {
        out[row * 3 + 0] = center;
        out[row * 3 + 1] = sigma;
        out[row * 3 + 2] = (float)n;
        row_cache_put<true>(cache, valid, p, tag, center, sigma, (float)n);
      }
    }
    __syncthreads();   // the list is rebuilt by the next pass
  }
}

}  // namespace

// out [R,3] fp32 = (centre, sigma, finite count) of hist[r, :T]; hist and ld
// need 4-byte alignment only.  Rows up to kRobustLdsKeys samples are selected
// in LDS, longer ones from global memory; the choice is per launch.
FM_API int fm_robust_stats(const float* hist, int64_t ld, int T, int64_t R, float* out, hipStream_t stream) {
  if (R <= 0) return 0;
  if (T < 0 || R > 0x7FFFFFFF || (((uintptr_t)hist) & 3) != 0) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)R), block(kRobustThreads);
  if (T <= kRobustLdsKeys) {
    hipLaunchKernelGGL((robust_stats_kernel<kRobustThreads, true>), grid, block, row_key_bytes(T), stream, hist, ld, T,
                       R, out);
  } else {
    hipLaunchKernelGGL((robust_stats_kernel<kRobustThreads, false>), grid, block, 0, stream, hist, ld, T, R, out);
  }
  FM_LAUNCH_CHECK();
  return 0;
}

// K18: out [R,3] = fm_robust_stats of the rows hist[rowmap[r], :T] (identity
// without a row map), with the statistics of physical row p kept in
// cache[p,3] / valid[p] (tag = T, 0 = invalid; fm_row_stats.h).
//   expect_miss != 0 or no cache: every row is computed, one workgroup per
//     logical row (at most `blocks` when blocks > 0), entries recorded with
//     plain stores;
//   expect_miss == 0: validity words are tested, hits copy 12 bytes, misses
//     are computed and published; `blocks` workgroups (<= 0: 512).
// The hint shapes the launch only: either form gives the same out and leaves
// every mapped entry valid.  T == 0 has no tag (0 = invalid): such a launch
// computes its rows (NaN, NaN, 0) and records nothing.
FM_API int fm_robust_stats_cached(const float* hist, int64_t ld, int T, int64_t R, float* out, const int* rowmap,
                                  float* cache, unsigned* valid, int expect_miss, int blocks, hipStream_t stream) {
  if (R <= 0) return 0;
  if (T < 0 || R > 0x7FFFFFFF || (((uintptr_t)hist) & 3) != 0 || (cache != nullptr && valid == nullptr))
    return (int)hipErrorInvalidValue;
  if (T == 0) cache = nullptr;
  const int scan = (cache != nullptr && expect_miss == 0) ? 1 : 0;
  int64_t g = scan ? (blocks > 0 ? blocks : kRobustScanBlocks) : (blocks > 0 ? blocks : R);
  if (g > R) g = R;
  const dim3 grid((unsigned)g), block(kRobustThreads);
  if (T <= kRobustLdsKeys) {
    hipLaunchKernelGGL((robust_stats_cached_kernel<kRobustThreads, true>), grid, block, row_key_bytes(T), stream, hist,
                       ld, T, R, out, rowmap, cache, valid, scan);
  } else {
    hipLaunchKernelGGL((robust_stats_cached_kernel<kRobustThreads, false>), grid, block, 0, stream, hist, ld, T, R,
                       out, rowmap, cache, valid, scan);
  }
  FM_LAUNCH_CHECK();
  return 0;
}
