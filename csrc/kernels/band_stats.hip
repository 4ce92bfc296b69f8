// K25 band records of the static band models over the rows of a
// device-resident history store, kept per physical row in a row-statistics
// cache: one launcher for a per-metric mix of
//   code 0  moving_average_all          (mean, std, std, n)        K1
//   code 1  robust_moving_average_all   (median, sigma, sigma, n)  K13
//   code 2  quantile_robust             (median, sigma_lo, sigma_up, n)  K24
// Logical row r has code codes[r % M] and reads physical row rowmap[r].  A
// record is four fp32 values, read and written as one float4, and is bit for
// bit what fm_hist_stats / fm_robust_stats / fm_quantile_robust_stats give for
// the row: the same device functions (fm_row_stats.h block_row_stats,
// fm_robust_row.h, fm_quantile_row.h) at the same thread counts.  Those counts
// differ (256 threads with the row in registers for code 0, 512 with the row
// in LDS for the selections), so two kernels stand behind the launcher, each
// skipping the rows of the other by their code; the launcher leaves out a
// kernel that has no row.
//
// The cache is fm_row_stats.h's protocol with 16-byte entries.  The tag of an
// entry is ((code + 1) << 28) | T, never 0: a physical row re-used under
// another model, or read at another view length, misses.
#include "fm_common.h"
#include "fm_quantile_row.h"
#include "fm_radix_select.h"
#include "fm_robust_row.h"
#include "fm_row_stats.h"

using namespace fm;

namespace {

constexpr int kMeanThreads = 256;      // block_row_stats is written for 256
constexpr int kSelectThreads = 512;    // K13's and K24's
constexpr int kSelectScanBlocks = 512; // as K18: two workgroups per CU of a 256-CU part
constexpr int kTagShift = 28;

// the 512-thread kernel's LDS: scratch, the misses of a scan pass and their
// count, K24's selection words, the longest LDS row
static_assert(sizeof(SelectScratch<kSelectThreads>) + (kSelectThreads + 1) * sizeof(int) + 16 * sizeof(unsigned) +
                      row_key_bytes(kRobustLdsKeys) <= kLaunchLds, "the longest LDS row fits a launch");

__device__ __forceinline__ unsigned band_tag(int code, int T) { return ((unsigned)(code + 1) << kTagShift) | (unsigned)T; }

// The model code of logical row `row` (R fits an int): a scalar load where the
// row is wave-uniform.
__device__ __forceinline__ int band_code(const int* __restrict__ codes, int M, int64_t row) {
  typedef const __attribute__((address_space(4))) int* const_codes;
  return ((const_codes)codes)[(int)row % M];
}

// Logical rows are dealt in metric-major order: index j of [0, S * M), S =
// ceil(R / M), is row (j % S) * M + j / S (none when that is >= R).  Workgroups
// go round the XCDs by their index, so with rows dealt as they lie and M a
// multiple of 8 every row of one metric, hence of one code, would land on one
// XCD: each of the two kernels would compute on the XCDs of its own metrics
// only.  In this order neighbouring workgroups hold neighbouring services of
// one metric.
__device__ __forceinline__ int64_t band_row(int64_t j, int S, int M) {
  const int ji = (int)j;
  return (int64_t)(ji % S) * M + ji / S;
}

// The record of logical row `row` into out, and into the entry of physical row
// p when there is a cache (publish: row_cache_put's two forms, fm_row_stats.h).
template <bool publish>
__device__ __forceinline__ void band_put(float* __restrict__ out, float* __restrict__ cache,
                                         unsigned* __restrict__ valid, int64_t row, int64_t p, unsigned tag,
                                         float4 rec) {
  reinterpret_cast<float4*>(out)[row] = rec;
  if (cache != nullptr) {
    reinterpret_cast<float4*>(cache)[p] = rec;
    if (publish) __hip_atomic_store(valid + p, tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    else valid[p] = tag;
  }
}

// One pass of a hit scan: thread tid looks at logical row `row` (have: it has
// one).  A row of another kernel's code is skipped, a hit is one 16-byte copy,
// a miss is listed.  Barriers on both sides: the list is complete on return.
template <class Mine>
__device__ __forceinline__ void scan_pass(bool have, int64_t row, const int* __restrict__ codes, int M, int T,
                                          float* __restrict__ out, const int* __restrict__ rowmap,
                                          float* __restrict__ cache, unsigned* __restrict__ valid, int* s_list,
                                          int* s_cnt, Mine mine) {
  const int tid = threadIdx.x;
  if (tid == 0) *s_cnt = 0;
  __syncthreads();
  if (have) {
    const int code = codes[(int)row % M];
    if (mine(code)) {
      const int64_t p = hist_row(rowmap, row);
      if (__hip_atomic_load(valid + p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == band_tag(code, T))
        reinterpret_cast<float4*>(out)[row] = reinterpret_cast<const float4*>(cache)[p];
      else
        s_list[atomicAdd(s_cnt, 1)] = tid;
    }
  }
  __syncthreads();
}

// The rows of code 0: K1's statistics by a 256-thread workgroup with the row
// in registers.  scan == 0: every such row is computed, rows dealt round-robin
// over the grid, no validity word read, plain stores (cache may be null);
// scan != 0: hist_scan_cached's form.
template <int NV>
__global__ __launch_bounds__(kMeanThreads) void band_mean_kernel(const float* __restrict__ hist, int64_t ld, int T,
                                                                 int64_t R, int M, const int* __restrict__ codes,
                                                                 float* __restrict__ out /*[R,4]*/,
                                                                 const int* __restrict__ rowmap,
                                                                 float* __restrict__ cache,
                                                                 unsigned* __restrict__ valid, int scan) {
  __shared__ double red[4];
  __shared__ int redi[4];
  __shared__ int s_list[kMeanThreads];
  __shared__ int s_cnt;
  const int tid = threadIdx.x;
  const unsigned tag = band_tag(0, T);
  const int64_t wg = blockIdx.x, nwg = gridDim.x;
  float mf, sd;
  int n;
  const int S = (int)((R + M - 1) / M);
  const int64_t J = (int64_t)S * M;
  if (!scan) {
    for (int64_t j = wg; j < J; j += nwg) {
      const int64_t row = band_row(j, S, M);
      if (row >= R || band_code(codes, M, row) != 0) continue;   // (the same in every thread)
      const int64_t p = hist_row(rowmap, row);
      block_row_stats<NV>(hist + p * ld, T, red, redi, mf, sd, n);
      if (tid == 0) band_put<false>(out, cache, valid, row, p, tag, make_float4(mf, sd, sd, (float)n));
    }
    return;
  }
  const int64_t nk = wg < J ? (J - wg + nwg - 1) / nwg : 0;   // rows of this workgroup
  for (int64_t k0 = 0; k0 < nk; k0 += kMeanThreads) {
    const int64_t mine = band_row(wg + (k0 + tid) * nwg, S, M);
    scan_pass(k0 + tid < nk && mine < R, mine, codes, M, T, out, rowmap, cache, valid, s_list, &s_cnt,
              [](int code) { return code == 0; });
    const int nm = s_cnt;
    for (int i = 0; i < nm; ++i) {
      const int64_t row = band_row(wg + (k0 + __builtin_amdgcn_readfirstlane(s_list[i])) * nwg, S, M);
      const int64_t p = hist_row(rowmap, row);
      block_row_stats<NV>(hist + p * ld, T, red, redi, mf, sd, n);
      if (tid == 0) band_put<true>(out, cache, valid, row, p, tag, make_float4(mf, sd, sd, (float)n));
    }
    __syncthreads();   // the list is rebuilt by the next pass
  }
}

// The record of one row of code 1 or 2 (the same in every thread of the
// workgroup): K13's or K24's row computation.  The bins are zero on entry and
// on return.
template <int NT, bool LDS>
__device__ __forceinline__ float4 select_row(const float* __restrict__ prow, int T, int code, double pq, float iz,
                                             uint4* keys, SelectScratch<NT>* sc, unsigned* sel) {
  float center, sigma_lo, sigma_up;
  int n;
  if (code == 1) {                                            // (the same in every thread)
    robust_row_stats<NT, LDS>(prow, T, keys, sc, center, sigma_lo, n);
    sigma_up = sigma_lo;
  } else {
    quantile_row_stats<NT, LDS>(prow, T, pq, iz, keys, sc, sel, center, sigma_lo, sigma_up, n);
  }
  // K24's last reads of the keys, the selection words and the scratch need not
  // sit in front of a barrier (a row whose keys are all one value reads them
  // last); the next row's first writes come after this one
  __syncthreads();
  return make_float4(center, sigma_lo, sigma_up, (float)n);
}

// The rows of codes 1 and 2 by a 512-thread workgroup, robust_stats_cached_kernel's
// two forms.
template <int NT, bool LDS>
__global__ __launch_bounds__(NT) void band_select_kernel(const float* __restrict__ hist, int64_t ld, int T, int64_t R,
                                                         int M, const int* __restrict__ codes, double pq, float iz,
                                                         float* __restrict__ out /*[R,4]*/,
                                                         const int* __restrict__ rowmap, float* __restrict__ cache,
                                                         unsigned* __restrict__ valid, int scan) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_keys[];
  __shared__ SelectScratch<NT> s_sc;
  __shared__ unsigned s_sel[9];
  __shared__ int s_list[NT];                                 // the misses of a scan pass
  __shared__ int s_cnt;
  const int tid = threadIdx.x;
  const int64_t wg = blockIdx.x, nwg = gridDim.x;
  // zero once: every selection hands the bins back zeroed, and a row without
  // a finite sample never touches them
  s_sc.clear_bins();
  const int S = (int)((R + M - 1) / M);
  const int64_t J = (int64_t)S * M;
  if (!scan) {
    for (int64_t j = wg; j < J; j += nwg) {
      const int64_t row = band_row(j, S, M);
      if (row >= R) continue;                                 // (the same in every thread)
      const int code = band_code(codes, M, row);
      if (code == 0) continue;
      const int64_t p = hist_row(rowmap, row);
      const float4 rec = select_row<NT, LDS>(hist + p * ld, T, code, pq, iz, s_keys, &s_sc, s_sel);
      if (tid == 0) band_put<false>(out, cache, valid, row, p, band_tag(code, T), rec);
    }
    return;
  }
  const int64_t nk = wg < J ? (J - wg + nwg - 1) / nwg : 0;   // rows of this workgroup
  for (int64_t k0 = 0; k0 < nk; k0 += NT) {
    const int64_t mine = band_row(wg + (k0 + tid) * nwg, S, M);
    scan_pass(k0 + tid < nk && mine < R, mine, codes, M, T, out, rowmap, cache, valid, s_list, &s_cnt,
              [](int code) { return code != 0; });
    const int nm = s_cnt;
    for (int i = 0; i < nm; ++i) {
      const int64_t row = band_row(wg + (k0 + __builtin_amdgcn_readfirstlane(s_list[i])) * nwg, S, M);
      const int code = band_code(codes, M, row);
      const int64_t p = hist_row(rowmap, row);
      const float4 rec = select_row<NT, LDS>(hist + p * ld, T, code, pq, iz, s_keys, &s_sc, s_sel);
      if (tid == 0) band_put<true>(out, cache, valid, row, p, band_tag(code, T), rec);
    }
    __syncthreads();   // the list is rebuilt by the next pass
  }
}

}  // namespace

// K25: out [R,4] fp32 = the band record (centre, sigma_lo, sigma_up, finite
// count) of hist[rowmap[r], :T] (identity without a row map) under the model
// codes[r % M] (device, [M], each 0..2); code_mask has bit c set when some
// metric has code c (host).  p = Phi(z0) in fp64 and inv_z0 = fp32(1 / z0) are
// K24's tail parameters.  The records of physical row q are kept in
// cache[q,4] / valid[q] (16-byte aligned; tag = ((code + 1) << 28) | T).
//   expect_miss != 0 or no cache: every row is computed, one workgroup per
//     logical row (at most `blocks` when blocks > 0), entries recorded with
//     plain stores;
//   expect_miss == 0: validity words are tested, hits copy 16 bytes, misses
//     are computed and published; `blocks` workgroups per kernel (<= 0: one
//     per 256 rows for code 0, 512 for the selections).
// The hint shapes the launch only.  Within one launch a physical row is mapped
// under one code only (a row of the store belongs to one metric of one job):
// duplicates then store the same bits, as fm_row_stats.h requires.  T == 0 computes (NaN, NaN, NaN, 0) and
// records nothing.  Rows of code 0 need K1's alignment (ld % 4 == 0, hist on
// 16 bytes, T within row_stats_dispatch_nv); the others 4 bytes.
FM_API int fm_band_stats_cached(const float* hist, int64_t ld, int T, int64_t R, int M, const int* codes,
                                int code_mask, double p, float inv_z0, float* out, const int* rowmap, float* cache,
                                unsigned* valid, int expect_miss, int blocks, hipStream_t stream) {
  if (R <= 0) return 0;
  if (T < 0 || T >= (1 << kTagShift) || R > 0x7FFFFFFF - 16 || (((uintptr_t)hist) & 3) != 0 ||
      (((uintptr_t)out) & 15) != 0 || M < 1 || M > 16 || codes == nullptr || code_mask <= 0 || (code_mask & ~7) != 0 ||
      (cache != nullptr && valid == nullptr) || (((uintptr_t)cache) & 15) != 0)
    return (int)hipErrorInvalidValue;
  const int nq = (T + 3) / 4;
  if ((code_mask & 1) != 0 && ((ld & 3) != 0 || (((uintptr_t)hist) & 15) != 0 || nq > 256 * 16))
    return (int)hipErrorInvalidValue;
  if ((code_mask & 4) != 0 && (!(p >= 0.5 && p <= 1.0) || !(inv_z0 > 0.f))) return (int)hipErrorInvalidValue;
  if (T == 0) cache = nullptr;                                // (no tag: nothing is recorded)
  const int scan = (cache != nullptr && expect_miss == 0) ? 1 : 0;
  const int64_t J = (R + M - 1) / M * M;                       // the rows as the kernels deal them (band_row)
  if ((code_mask & 1) != 0) {
    int64_t g = blocks > 0 ? blocks : (scan ? (J + kMeanThreads - 1) / kMeanThreads : J);
    if (g > J) g = J;
    const dim3 grid((unsigned)g), block(kMeanThreads);
    const int rc = row_stats_dispatch_nv(nq, [&](auto nv) {
      hipLaunchKernelGGL(band_mean_kernel<decltype(nv)::value>, grid, block, 0, stream, hist, ld, T, R, M, codes, out,
                         rowmap, cache, valid, scan);
    });
    if (rc != 0) return rc;
    FM_LAUNCH_CHECK();
  }
  if ((code_mask & 6) != 0) {
    int64_t g = blocks > 0 ? blocks : (scan ? kSelectScanBlocks : J);
    if (g > J) g = J;
    const dim3 grid((unsigned)g), block(kSelectThreads);
    if (T <= kRobustLdsKeys) {
      hipLaunchKernelGGL((band_select_kernel<kSelectThreads, true>), grid, block, row_key_bytes(T), stream, hist, ld, T,
                         R, M, codes, p, inv_z0, out, rowmap, cache, valid, scan);
    } else {
      hipLaunchKernelGGL((band_select_kernel<kSelectThreads, false>), grid, block, 0, stream, hist, ld, T, R, M, codes,
                         p, inv_z0, out, rowmap, cache, valid, scan);
    }
    FM_LAUNCH_CHECK();
  }
  return 0;
}
