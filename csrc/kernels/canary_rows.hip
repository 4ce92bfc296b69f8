// fm-hipcc-flags: -mllvm -pragma-unroll-threshold=1000000
// (the 1024-sample pairwise sort, K = 16: past LLVM's default pragma-unroll
// size limit the stage loops stayed rolled -- runtime register indexing
// through scratch (132 B/lane) and s_set_gpr_idx; fully unrolled: 0 scratch)
#include "fm_pairwise.h"

// ---------------------------------------------------------------------------
// Fused canary row kernel: ONE wave per (service, metric) row does both the
// HBM-bound history statistics (mean / std / count over the 7-day row) and the
// compute-bound pairwise rank tests.  Order inside the wave: the small
// cur/base loads, then the whole history row (NQ float4 per lane, streamed,
// non-temporal), then the pairwise compute runs while the history is still in
// flight (vmcnt waits only for the first, small loads: in-order completion),
// then the history is reduced from registers.  The separate two-stream form
// (pairwise on a side stream || hist_stats) shares the CUs between two kernels
// whose waves compete for slots; here each wave carries both.
// ---------------------------------------------------------------------------
template <int NQ, int K>
__global__ __launch_bounds__(256) void canary_row_kernel(
    const float* __restrict__ hist, int64_t ld_h, int T, const float* __restrict__ cur, int64_t ld_c, int n_cur,
    const float* __restrict__ base, int64_t ld_b, int n_base, int64_t R, float* __restrict__ hs /*[R,3]*/,
    double* __restrict__ suff) {
  const int64_t row = (int64_t)blockIdx.x * 4 + wave_id();
  if (row >= R) return;
  const int lane = lane_id();
  const bool do_pw = n_base > 0;
  PwIn<K> in;
  // same layout choice as pw_row, so every tick mode sums the Welch moments
  // in the same order (bit-identical p-values across modes)
  const bool split = K == 2 && n_cur <= 64 && n_base <= 64;
  if (do_pw) {
    if constexpr (K == 2) {
      if (split) pw_load<K, true>(cur + row * ld_c, base + row * ld_b, n_cur, n_base, in);
      else pw_load<K>(cur + row * ld_c, base + row * ld_b, n_cur, n_base, in);
    } else {
      pw_load<K>(cur + row * ld_c, base + row * ld_b, n_cur, n_base, in);
    }
  }

  typedef float nt4 __attribute__((ext_vector_type(4)));
  const nt4* h = reinterpret_cast<const nt4*>(hist + row * ld_h);
  const int nq = (T + 3) >> 2;
  nt4 q[NQ];
  // Unpredicated loads (index clamped into the row, surplus masked by e0 < T
  // in the reduction): with exec-masked branches around them the waitcnt pass
  // could not prove how many loads are outstanding and waited for all of them
  // before the pairwise compute.
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    const int qi = lane + j * 64;
    q[j] = __builtin_nontemporal_load(h + (qi < nq ? qi : nq - 1));
  }

  if (do_pw) {
    if constexpr (K == 2) {
      if (split) pw_compute<K, true>(in, n_cur, n_base, suff + row * kSuff);
      else pw_compute<K>(in, n_cur, n_base, suff + row * kSuff);
    } else {
      pw_compute<K>(in, n_cur, n_base, suff + row * kSuff);
    }
  }

  float ls = 0.f;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    const int e0 = (lane + j * 64) * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float x = q[j][c];
      if (e0 + c < T && isfinite(x)) { ls += x; ++cnt; }
    }
  }
  const double tot = wave_sum((double)ls);
  const int n = wave_sum(cnt);
  const float mf = n > 0 ? (float)(tot / n) : 0.f;
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    const int e0 = (lane + j * 64) * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float x = q[j][c];
      if (e0 + c < T && isfinite(x)) { const float d = x - mf; ss += d * d; }
    }
  }
  const double sst = wave_sum((double)ss);
  if (lane == 0) {
    hs[row * 3 + 0] = mf;
    hs[row * 3 + 1] = n > 0 ? (float)sqrt(sst / n) : 0.f;
    hs[row * 3 + 2] = (float)n;
  }
}

FM_API int fm_canary_rows(const float* hist, int64_t ld_h, int T, const float* cur, int64_t ld_c, int n_cur,
                          const float* base, int64_t ld_b, int n_base, int64_t R, float* hs, double* suff,
                          hipStream_t stream) {
  if (R <= 0) return 0;
  if ((ld_h & 3) != 0 || (((uintptr_t)hist) & 15) != 0) return (int)hipErrorInvalidValue;
  const int nq = (T + 3) / 4;
  const int n = n_cur + (n_base > 0 ? n_base : 0);
  const dim3 grid((unsigned)((R + 3) / 4)), block(256);
#define FM_CR(NQQ, KK) hipLaunchKernelGGL((canary_row_kernel<NQQ, KK>), grid, block, 0, stream, hist, ld_h, T, cur, \
                                          ld_c, n_cur, base, ld_b, n_base, R, hs, suff)
#define FM_CR_K(NQQ)              \
  if (n <= 64) FM_CR(NQQ, 1);     \
  else if (n <= 128) FM_CR(NQQ, 2); \
  else if (n <= 256) FM_CR(NQQ, 4); \
  else return (int)hipErrorInvalidValue;
  if (nq <= 64 * 8) { FM_CR_K(8) }
  else if (nq <= 64 * 16) { FM_CR_K(16) }
  else if (nq <= 64 * 24) { FM_CR_K(24) }
  else if (nq <= 64 * 32) { FM_CR_K(32) }
  else if (nq <= 64 * 40) { FM_CR_K(40) }
  else return (int)hipErrorInvalidValue;
#undef FM_CR_K
#undef FM_CR
  FM_LAUNCH_CHECK();
  return 0;
}
