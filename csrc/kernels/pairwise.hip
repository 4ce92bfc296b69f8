// fm-hipcc-flags: -mllvm -pragma-unroll-threshold=1000000
// (the 1024-sample pairwise sort, K = 16: past LLVM's default pragma-unroll
// size limit the stage loops stayed rolled -- runtime register indexing
// through scratch (132 B/lane) and s_set_gpr_idx; fully unrolled: 0 scratch)
// K4 as stand-alone kernels: the pairwise rank tests (sort form and counting
// form, fm_pairwise.h) -> per-row sufficient statistics, and the p-values /
// ALL-ANY combine, one row per thread.
#include "fm_pairwise.h"

template <int K>
__global__ __launch_bounds__(256) void pairwise_count_kernel(
    const float* __restrict__ cur, int64_t ld_c, int n_cur, const float* __restrict__ base, int64_t ld_b,
    int n_base, int64_t R, double* __restrict__ suff) {
  constexpr int KW = PwIn<K>::KW;
  constexpr int PER_WAVE = 3 * 64 * K + 12;
  __shared__ __attribute__((aligned(16))) float lds[4 * PER_WAVE];
  float* my = lds + wave_id() * PER_WAVE;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave_id(); row < R; row += (int64_t)gridDim.x * 4) {
    PwIn<K> in;
    pw_load<K>(cur + row * ld_c, base + row * ld_b, n_cur, n_base, in);
    pw_compute_count<K>(in, n_cur, n_base, suff + row * kSuff, my);
  }
}

// Grid-stride over rows: launched with one wave per row, or capped to a few
// workgroups per CU so a concurrently running HBM-bound kernel keeps most of
// the wave slots (two-stream tick).
template <int K>
__global__ __launch_bounds__(256) void pairwise_kernel(
    const float* __restrict__ cur, int64_t ld_c, int n_cur, const float* __restrict__ base, int64_t ld_b,
    int n_base, int64_t R, double* __restrict__ suff) {
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave_id(); row < R; row += (int64_t)gridDim.x * 4) {
    pw_row<K>(cur + row * ld_c, base + row * ld_b, n_cur, n_base, suff + row * kSuff);
  }
}

__global__ __launch_bounds__(256) void pvalue_kernel(const double* __restrict__ suff, int64_t R, int min_mw,
                                                     int min_wil, int min_kru, float* __restrict__ pvals,
                                                     float* __restrict__ stats, int t0 = 0) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int t = blockIdx.y + t0;
  if (row >= R) return;
  double pv, sv;
  eval_test(t, suff + row * kSuff, min_mw, min_wil, min_kru, pv, sv);
  pvals[row * N_TESTS + t] = (float)pv;
  stats[row * N_TESTS + t] = (float)sv;
}

// ALL / ANY over the selected, applicable tests -> "distribution differs".
__global__ __launch_bounds__(256) void pcombine_kernel(const float* __restrict__ pvals, int64_t R, int test_mask,
                                                       int combine_any, float p_thr, int8_t* __restrict__ diff) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= R) return;
  int applicable = 0, significant = 0;
#pragma unroll
  for (int t = 0; t < N_TESTS; ++t) {
    const float p = pvals[row * N_TESTS + t];
    if (((test_mask >> t) & 1) && !isnan(p)) {
      ++applicable;
      if (p < p_thr) ++significant;
    }
  }
  diff[row] = applicable > 0 ? (int8_t)(combine_any ? (significant > 0) : (significant == applicable)) : (int8_t)0;
}

static int launch_pvalues(const double* suff, int64_t R, int test_mask, int combine_any, float p_thr, int min_mw,
                          int min_wil, int min_kru, float* pvals, float* stats, int8_t* diff, hipStream_t stream) {
  const unsigned nb = (unsigned)((R + 255) / 256);
  hipLaunchKernelGGL(pvalue_kernel, dim3(nb, N_TESTS), dim3(256), 0, stream, suff, R, min_mw, min_wil, min_kru, pvals,
                     stats, 0);
  FM_LAUNCH_CHECK();
  hipLaunchKernelGGL(pcombine_kernel, dim3(nb), dim3(256), 0, stream, pvals, R, test_mask, combine_any, p_thr, diff);
  FM_LAUNCH_CHECK();
  return 0;
}

// variant: 0 = bitonic-sort form (default), 1 = counting form.  Measured at
// 80k rows x (50 + 50): sort 140 us, counting 184 us (tools/tick_breakdown.py):
// the counting sweep issues ~n compares per owned value, more instructions
// than the log^2 network now that its exchanges are DPP / permlane.
FM_API int fm_pairwise_suff_v(const float* cur, int64_t ld_c, int n_cur, const float* base, int64_t ld_b,
                              int n_base, int64_t R, double* suff, int max_blocks, int variant, hipStream_t stream) {
  if (R <= 0) return 0;
  const int n = n_cur + n_base;
  int64_t blocks = (R + 3) / 4;
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
  const dim3 grid((unsigned)blocks), block(256);
#define FM_PW(KK)                                                                                                 \
  do {                                                                                                           \
    if (variant == 0)                                                                                            \
      hipLaunchKernelGGL(pairwise_kernel<KK>, grid, block, 0, stream, cur, ld_c, n_cur, base, ld_b, n_base, R,    \
                         suff);                                                                                  \
    else                                                                                                         \
      hipLaunchKernelGGL(pairwise_count_kernel<KK>, grid, block, 0, stream, cur, ld_c, n_cur, base, ld_b, n_base, \
                         R, suff);                                                                               \
  } while (0)
  if (n <= 64) FM_PW(1);
  else if (n <= 128) FM_PW(2);
  else if (n <= 256) FM_PW(4);
  else if (n <= 512) FM_PW(8);
  else if (n <= 1024) FM_PW(16);
  else return (int)hipErrorInvalidValue;
#undef FM_PW
  FM_LAUNCH_CHECK();
  return 0;
}

FM_API int fm_pairwise_suff(const float* cur, int64_t ld_c, int n_cur, const float* base, int64_t ld_b, int n_base,
                            int64_t R, double* suff, int max_blocks, hipStream_t stream) {
  return fm_pairwise_suff_v(cur, ld_c, n_cur, base, ld_b, n_base, R, suff, max_blocks, 0, stream);
}

FM_API int fm_pvalues(const double* suff, int64_t R, int test_mask, int combine_any, float p_thr, int min_mw,
                      int min_wil, int min_kru, float* pvals, float* stats, int8_t* diff, hipStream_t stream) {
  if (R <= 0) return 0;
  return launch_pvalues(suff, R, test_mask, combine_any, p_thr, min_mw, min_wil, min_kru, pvals, stats, diff,
                        stream);
}

FM_API int fm_pairwise_tests(const float* cur, int64_t ld_c, int n_cur, const float* base, int64_t ld_b, int n_base,
                             int64_t R, int test_mask, int combine_any, float p_thr, int min_mw, int min_wil,
                             int min_kru, float* pvals, float* stats, int8_t* diff, double* suff,
                             hipStream_t stream) {
  if (R <= 0) return 0;
  // sort form, one wave per row (no block cap)
  const int rc = fm_pairwise_suff_v(cur, ld_c, n_cur, base, ld_b, n_base, R, suff, 0, 0, stream);
  if (rc != 0) return rc;
  return launch_pvalues(suff, R, test_mask, combine_any, p_thr, min_mw, min_wil, min_kru, pvals, stats, diff,
                        stream);
}

// p-values only (the combine happens in fm_decide_services)
FM_API int fm_pvalues_only(const double* suff, int64_t R, int min_mw, int min_wil, int min_kru, float* pvals,
                           float* stats, hipStream_t stream) {
  if (R <= 0) return 0;
  hipLaunchKernelGGL(pvalue_kernel, dim3((unsigned)((R + 255) / 256), N_TESTS), dim3(256), 0, stream, suff, R,
                     min_mw, min_wil, min_kru, pvals, stats, 0);
  FM_LAUNCH_CHECK();
  return 0;
}

// Tests [t0, t1) only (per-test timing in tools/tick_breakdown.py).
FM_API int fm_pvalues_range(const double* suff, int64_t R, int t0, int t1, int min_mw, int min_wil, int min_kru,
                            float* pvals, float* stats, hipStream_t stream) {
  if (R <= 0 || t0 < 0 || t1 > N_TESTS || t1 <= t0) return 0;
  hipLaunchKernelGGL(pvalue_kernel, dim3((unsigned)((R + 255) / 256), t1 - t0), dim3(256), 0, stream, suff, R,
                     min_mw, min_wil, min_kru, pvals, stats, t0);
  FM_LAUNCH_CHECK();
  return 0;
}
