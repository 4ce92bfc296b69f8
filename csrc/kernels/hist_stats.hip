// History statistics as stand-alone kernels (K1, K1 + K7): mean / std /
// finite count of a history row held in registers (fm_row_stats.h), alone or
// fused with the anomaly decision on the current window.
#include "fm_row_stats.h"

// ---------------------------------------------------------------------------
// K1 + K7 fused: moving_average_all bounds over the whole history row and the
// anomaly decision on the current window, one 256-thread workgroup per row.
// The row is read once from HBM with 16-B loads and kept in registers
// (NV float4 per thread) so the two-pass mean / variance costs no re-read.
// ---------------------------------------------------------------------------
template <int NV>
__global__ __launch_bounds__(256) void stats_decide_kernel(
    const float* __restrict__ hist, int64_t ld_h, int T, const float* __restrict__ cur, int64_t ld_c, int n_cur,
    int64_t R, int M, const float* __restrict__ thr, const int* __restrict__ bound, const float* __restrict__ minlb,
    float pair_factor, const int8_t* __restrict__ diff, int min_hist, float* __restrict__ out_stats,
    unsigned long long* __restrict__ out_flags, int NW, int* __restrict__ out_count, float* __restrict__ out_score,
    int* __restrict__ out_valid) {
  __shared__ double red[4];
  __shared__ int redi[4];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  float mf, sd;
  int n;
  block_row_stats<NV>(hist + row * ld_h, T, red, redi, mf, sd, n);
  const int m = (int)(row % M);
  float th = thr[m];
  if (diff != nullptr && diff[row]) th *= pair_factor;
  const int bd = bound[m];
  const float up = mf + th * sd;
  float lo = mf - th * sd;
  const float mlb = minlb[m];
  if (lo < mlb) lo = mlb;
  const bool has_hist = n >= min_hist && n > 0;

  const float* cr = cur + row * ld_c;
  int acnt = 0, ccnt = 0;
  float best = 0.f;
  const float inv = sd > 0.f ? __builtin_amdgcn_rcpf(sd) : 0.f;   // z-score scale, 1-ulp rcp
  for (int i0 = 0; i0 < n_cur; i0 += 256) {
    const int i = i0 + tid;
    bool f = false;
    if (i < n_cur) {
      const float x = cr[i];
      if (isfinite(x)) {
        ++ccnt;
        if (has_hist) {
          const bool hi = (bd & 1) && x > up;
          const bool lw = (bd & 2) && x < lo;
          f = hi || lw;
          if (f) {
            ++acnt;
            const float e = hi ? (x - up) : (lo - x);
            const float z = sd > 0.f ? e * inv : 1e30f;
            best = z > best ? z : best;
          }
        }
      }
    }
    const unsigned long long bal = __ballot(f);
    const int w = i0 / 64 + wave_id();
    if (lane_id() == 0 && w < NW) out_flags[row * NW + w] = bal;
  }
  acnt = block_sum<256>(acnt, redi);
  ccnt = block_sum<256>(ccnt, redi);
  best = block_max<256>(best, (float*)red);
  if (tid == 0) {
    out_stats[row * 4 + 0] = mf;
    out_stats[row * 4 + 1] = sd;
    out_stats[row * 4 + 2] = up;
    out_stats[row * 4 + 3] = lo;
    out_count[row] = acnt;
    out_score[row] = best;
    out_valid[row] = (has_hist ? 1 : 0) | (ccnt > 0 ? 2 : 0);
  }
}

FM_API int fm_stats_decide(const float* hist, int64_t ld_h, int T, const float* cur, int64_t ld_c, int n_cur, int64_t R,
                           int M, const float* thr, const int* bound, const float* minlb, float pair_factor,
                           const int8_t* diff, int min_hist, float* out_stats, unsigned long long* out_flags, int NW,
                           int* out_count, float* out_score, int* out_valid, hipStream_t stream) {
  if (R <= 0) return 0;
  if ((ld_h & 3) != 0 || (((uintptr_t)hist) & 15) != 0) return (int)hipErrorInvalidValue;
  if (NW * 64 < n_cur) return (int)hipErrorInvalidValue;
  const int nq = (T + 3) / 4;
  const dim3 grid((unsigned)R), block(256);
  const int rc = row_stats_dispatch_nv(nq, [&](auto nv) {
    hipLaunchKernelGGL(stats_decide_kernel<decltype(nv)::value>, grid, block, 0, stream, hist, ld_h, T, cur, ld_c,
                       n_cur, R, M, thr, bound, minlb, pair_factor, diff, min_hist, out_stats, out_flags, NW,
                       out_count, out_score, out_valid);
  });
  if (rc != 0) return rc;
  FM_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// Split form of the same computation for the two-stream tick: hist_stats is
// the HBM-bound pass (mean, std, count per row) and runs concurrently with the
// compute-bound pairwise kernel on another stream; decide_service_kernel
// (decide.hip, reads only the small current window) applies the
// diff-dependent thresholds once both are done.
// ---------------------------------------------------------------------------
template <int NV>
__global__ __launch_bounds__(256) void hist_stats_kernel(const float* __restrict__ hist, int64_t ld_h, int T,
                                                         int64_t R, float* __restrict__ out /*[R,3]*/,
                                                         const int* __restrict__ rowmap, float* __restrict__ cache,
                                                         unsigned* __restrict__ valid) {
  __shared__ double red[4];
  __shared__ int redi[4];
  // (row-statistics cache, fm_row_stats.h: this launch tests no word)
  for (int64_t row = blockIdx.x; row < R; row += gridDim.x)
    hist_row_emit<NV, false>(hist, ld_h, T, out, rowmap, cache, valid, row, red, redi);
}

// The same with the row-statistics cache of the history tensor
// (fm_row_stats.h): a row whose validity word carries this view's tag is
// copied from the cache, any other is reduced and recorded.
template <int NV>
__global__ __launch_bounds__(256) void hist_stats_cached_kernel(const float* __restrict__ hist, int64_t ld_h, int T,
                                                                int64_t R, float* __restrict__ out /*[R,3]*/,
                                                                const int* __restrict__ rowmap,
                                                                float* __restrict__ cache,
                                                                unsigned* __restrict__ valid) {
  __shared__ double red[4];
  __shared__ int redi[4];
  __shared__ int s_list[256];
  __shared__ int s_cnt;
  hist_scan_cached<NV>(hist, ld_h, T, R, out, rowmap, cache, valid, blockIdx.x, gridDim.x, red, redi, s_list, &s_cnt);
}

// expect_miss 1 (or null cache pointers, which record nothing): every row is
// reduced and recorded without a look at its word, one workgroup per row
// (capped by max_blocks); 0: one workgroup per 256 rows, a row per thread,
// which reduces what does miss.
FM_API int fm_hist_stats_cached(const float* hist, int64_t ld_h, int T, int64_t R, float* out, int max_blocks,
                                const int* rowmap, float* cache, unsigned* valid, int expect_miss,
                                hipStream_t stream) {
  if (R <= 0) return 0;
  if ((ld_h & 3) != 0 || (((uintptr_t)hist) & 15) != 0) return (int)hipErrorInvalidValue;
  if (cache == nullptr || valid == nullptr || T <= 0) cache = nullptr, valid = nullptr;   // (tag 0 means invalid)
  const bool scan = cache != nullptr && expect_miss == 0;
  const int nq = (T + 3) / 4;
  const dim3 grid((unsigned)(scan ? (R + 255) / 256 : (max_blocks > 0 && R > max_blocks ? max_blocks : R))), block(256);
  const int rc = row_stats_dispatch_nv(nq, [&](auto nv) {
    constexpr int NV = decltype(nv)::value;
    if (scan) hipLaunchKernelGGL(hist_stats_cached_kernel<NV>, grid, block, 0, stream, hist, ld_h, T, R, out, rowmap,
                                 cache, valid);
    else hipLaunchKernelGGL(hist_stats_kernel<NV>, grid, block, 0, stream, hist, ld_h, T, R, out, rowmap, cache, valid);
  });
  if (rc != 0) return rc;
  FM_LAUNCH_CHECK();
  return 0;
}

// Invalidate the first n validity words (a writer that cannot name its rows).
FM_API int fm_hist_cache_invalidate(unsigned* valid, int64_t n, hipStream_t stream) {
  if (valid == nullptr || n <= 0) return 0;
  return (int)hipMemsetAsync(valid, 0, (size_t)n * sizeof(unsigned), stream);
}

FM_API int fm_hist_stats_capped(const float* hist, int64_t ld_h, int T, int64_t R, float* out, int max_blocks,
                                hipStream_t stream) {
  return fm_hist_stats_cached(hist, ld_h, T, R, out, max_blocks, nullptr, nullptr, nullptr, 1, stream);
}

FM_API int fm_hist_stats(const float* hist, int64_t ld_h, int T, int64_t R, float* out, hipStream_t stream) {
  return fm_hist_stats_cached(hist, ld_h, T, R, out, 0, nullptr, nullptr, nullptr, 1, stream);
}
