// fm-hipcc-flags: -mllvm -pragma-unroll-threshold=1000000 -ffp-contract=off
// (the unroll threshold as in pairwise.hip: the K = 16 bitonic network must
// unroll fully to stay in registers.  Contraction is off because the median's
// `0.5f * lo + 0.5f * up` is defined as two fp32 products and a sum, each
// rounded once, and the fp64 moments as plain products and sums; an fma would
// round once and break the contract with the numpy reference.)
//
// K27: Brown-Forsythe scale test of current vs baseline (Levene's test on the
// absolute deviations from each side's median), docs/BRAIN_SPEC.md 4.2.  The
// contract is foremast_amd/ops/reference.py pairwise_scale / scale_verdict.
//
// Per row, over the finite samples x_1..x_n1 and y_1..y_n2:
//   med_c, med_b   fp32 medians (middle order statistic, or 0.5f lo + 0.5f up)
//   u_i = fl32(|fl32(x_i - med_c)|), v_j likewise
//   fp64: su = sum u, sv = sum v, ubar = su / n1, vbar = sv / n2,
//         SSW = sum (u - ubar)^2 + sum (v - vbar)^2   (two passes)
// Two tiers write these seven numbers per row (`moments`), and one finishing
// pass, one row per thread so that the fp64 special function runs on full
// waves as the p-values of K4 do, turns them into W = nu SSB / SSW, p =
// student_t_2sided(sqrt(W), nu), ratio = ubar / vbar, the verdict, and the copy
// of the p-values the decision reads (0 in all six columns of a flagged row).
//
// Wave tier (each side <= 1024 columns): one wave per row, four rows per
// workgroup, as K19.  Each side is sorted in registers (bitonic_sort<K>, K by
// the wider side), the middle order statistics are read off the sorted image
// with lane reads, and the deviations and both fp64 passes come from the
// registers.  No LDS.
//
// Wide tier (pooled width <= kScaleWideMax, any split): one workgroup per row.
// Each side goes to LDS once as the order-preserving keys of
// fm_radix_select.h (load_row_keys), both middle ranks come from one
// radix_select_ranks, and the two fp64 passes sweep the keys (block_sum).
#include "fm_pairwise.h"
#include "fm_radix_select.h"

namespace {

constexpr int kScaleWaveMax = 1024;          // columns per side, wave tier (SCALE_WAVE_MAX in ops/canary.py)
constexpr int kScaleWideMax = 8192;          // pooled columns, wide tier (PAIRWISE_WIDE_MAX in ops/canary.py)
constexpr int kScaleNT = 256;
constexpr int kMoments = 8;                  // n1, n2, su, sv, SSW, med_c, med_b, (unused)

// both sides' keys at any alignment and any split: row_key_bytes(a) + row_key_bytes(b) <= this for a + b <= max
constexpr size_t kScaleKeyBytes = (size_t)((kScaleWideMax + 12) / 4) * sizeof(uint4);
static_assert(row_key_bytes(kScaleWideMax) + row_key_bytes(0) <= kScaleKeyBytes &&
                  2 * row_key_bytes(kScaleWideMax / 2) <= kScaleKeyBytes,
              "the bound holds at the extreme splits");
static_assert(sizeof(SelectScratch<kScaleNT>) + 8 * sizeof(unsigned) + kScaleKeyBytes <= kLaunchLds,
              "the widest row fits a launch");

// Entry i (wave-uniform, inside the array) of a register image v[k] at lane l = slot 64 k + l
template <int K>
__device__ __forceinline__ float image_at(const float (&v)[K], int i) {
  float r = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float t = lane_bcast(v[k], i & 63);
    r = (i >> 6) == k ? t : r;
  }
  return r;
}

// One side in registers (pads = kPad, n finite values): sorted, then its
// median, the fp64 sum of the deviations from it and their squared deviations
// from their own mean.  Wave-uniform results.
template <int K>
__device__ __forceinline__ void wave_side(float (&v)[K], int n, float& med, double& sum, double& ss) {
  int tag_unused[K];
  bitonic_sort<K, false, false>(v, tag_unused);
  med = __uint_as_float(0x7FC00000u);
  sum = 0.0;
  ss = 0.0;
  if (n == 0) return;
  med = 0.5f * image_at<K>(v, (n - 1) >> 1) + 0.5f * image_at<K>(v, n >> 1);
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (v[k] != kPad) s += (double)fabsf(v[k] - med);
  sum = wave_sum(s);
  const double mean = sum / (double)n;
  double q = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (v[k] != kPad) {
      const double d = (double)fabsf(v[k] - med) - mean;
      q += d * d;
    }
  }
  ss = wave_sum(q);
}

__device__ __forceinline__ void store_moments(double* __restrict__ m, int n1, int n2, double su, double sv, double ssw,
                                              float med_c, float med_b) {
  m[0] = n1; m[1] = n2; m[2] = su; m[3] = sv; m[4] = ssw; m[5] = med_c; m[6] = med_b; m[7] = 0.0;
}

// One side of a wide row: keys into LDS, both middle ranks selected, two sweeps.
// Every thread of the workgroup calls it; every branch around a barrier is
// workgroup-uniform; the bins are zero on entry and on return.
template <int NT>
__device__ __forceinline__ void block_side(const float* p, int T, uint4* keys, SelectScratch<NT>* sc, unsigned* sel,
                                           int& n, float& med, double& sum, double& ss) {
  n = 0;
  med = quiet_nan();
  sum = 0.0;
  ss = 0.0;
  if (T == 0) return;
  const int a = row_word(p);
  RowTally t;
  load_row_keys<NT>(p, T, a, keys, t);
  n = uniform(block_sum<NT>(t.n, sc->redi));                  // (barriers: keys and bins visible)
  if (n == 0) return;
  const LdsRow<NT> rk{keys, row_quads(a, T)};
  const unsigned rank[2] = {(unsigned)(n - 1) >> 1, (unsigned)n >> 1};
  unsigned key[2], resid[2], cnt[2];
  radix_select_ranks(rk, block_range(t.range, sc), rank, (unsigned)n, sc, sel, key, resid, cnt);
  const float m = mid_value(key[0], key[1]);
  med = m;
  double s = 0.0;
  rk.sweep([&](unsigned k) { if (k != kMissing) s += (double)fabsf(dec_key(k) - m); });
  sum = uniform(block_sum<NT>(s, sc->redd));
  const double mean = sum / (double)n;
  double q = 0.0;
  rk.sweep([&](unsigned k) {
    if (k != kMissing) {
      const double d = (double)fabsf(dec_key(k) - m) - mean;
      q += d * d;
    }
  });
  ss = block_sum<NT>(q, sc->redd);
}

}  // namespace

template <int K>
__global__ __launch_bounds__(256) void scale_wave_kernel(const float* __restrict__ cur, int64_t ld_c, int n_cur,
                                                         const float* __restrict__ base, int64_t ld_b, int n_base,
                                                         int64_t R, double* __restrict__ moments) {
  const int lane = lane_id();
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave_id(); row < R; row += (int64_t)gridDim.x * 4) {
    const float* c = cur + row * ld_c;
    const float* b = base + row * ld_b;
    float x[K], y[K];
    int n1 = 0, n2 = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = k * 64 + lane;
      const float xv = i < n_cur ? c[i] : kPad;
      const float yv = i < n_base ? b[i] : kPad;
      const bool okx = isfinite(xv), oky = isfinite(yv);
      x[k] = okx ? xv : kPad;
      y[k] = oky ? yv : kPad;
      n1 += __popcll(__ballot(okx));
      n2 += __popcll(__ballot(oky));
    }
    float med_c, med_b;
    double su, sv, qu, qv;
    wave_side<K>(x, n1, med_c, su, qu);
    wave_side<K>(y, n2, med_b, sv, qv);
    if (lane == 0) store_moments(moments + row * kMoments, n1, n2, su, sv, qu + qv, med_c, med_b);
  }
}

__global__ __launch_bounds__(kScaleNT) void scale_wide_kernel(const float* __restrict__ cur, int64_t ld_c, int n_cur,
                                                              const float* __restrict__ base, int64_t ld_b, int n_base,
                                                              int64_t R, double* __restrict__ moments) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_keys[];
  __shared__ SelectScratch<kScaleNT> s_sc;
  __shared__ unsigned s_sel[8];
  uint4* keys_c = s_keys;
  uint4* keys_b = s_keys + row_key_bytes(n_cur) / sizeof(uint4);
  s_sc.clear_bins();
  for (int64_t row = blockIdx.x; row < R; row += gridDim.x) {
    int n1, n2;
    float med_c, med_b;
    double su, sv, qu, qv;
    block_side<kScaleNT>(cur + row * ld_c, n_cur, keys_c, &s_sc, s_sel, n1, med_c, su, qu);
    block_side<kScaleNT>(base + row * ld_b, n_base, keys_b, &s_sc, s_sel, n2, med_b, sv, qv);
    if (threadIdx.x == 0) store_moments(moments + row * kMoments, n1, n2, su, sv, qu + qv, med_c, med_b);
    __syncthreads();                                          // the keys and the scratch are reused by the next row
  }
}

// One row per thread: the statistic, its p-value, the verdict and the forced p-values.
__global__ __launch_bounds__(256) void scale_finish_kernel(const double* __restrict__ moments, int64_t R,
                                                           int min_points, float p_thr, float min_ratio,
                                                           float inv_ratio, int both,
                                                           const float* __restrict__ pvals_in,
                                                           float* __restrict__ scale, int8_t* __restrict__ scale_diff,
                                                           float* __restrict__ pvals_out) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= R) return;
  const double* m = moments + row * kMoments;
  const int n1 = (int)m[0], n2 = (int)m[1];
  const double su = m[2], sv = m[3], ssw = m[4];
  const double NaN = __builtin_nan("");
  double W = NaN, p = NaN, ratio = NaN;
  const int need = min_points > 1 ? min_points : 1;
  if (n1 >= need && n2 >= need && isfinite(su) && isfinite(sv)) {
    const double d1 = n1, d2 = n2, dn = d1 + d2;
    const double ubar = su / d1, vbar = sv / d2, zbar = (su + sv) / dn;
    const double a = ubar - zbar, b = vbar - zbar;
    const double ssb = d1 * (a * a) + d2 * (b * b);
    if (!(ssw == 0.0 && ssb == 0.0)) {
      const double nu = dn - 2.0;
      W = nu * ssb / ssw;                                     // SSW == 0 < SSB: +inf
      p = isinf(W) ? 0.0 : student_t_2sided(sqrt(W), nu);
      ratio = ubar / vbar;                                    // vbar == 0 < ubar: +inf
    }
  }
  const float pf = (float)p, rf = (float)ratio;
  const bool flagged = !isnan(pf) && pf < p_thr && (rf >= min_ratio || (both != 0 && rf <= inv_ratio));
  float* s = scale + row * 6;
  s[0] = (float)W; s[1] = pf; s[2] = rf; s[3] = (float)m[5]; s[4] = (float)m[6]; s[5] = (float)(n1 + n2);
  scale_diff[row] = flagged ? 1 : 0;
  if (pvals_in != nullptr) {
#pragma unroll
    for (int t = 0; t < N_TESTS; ++t) pvals_out[row * N_TESTS + t] = flagged ? 0.f : pvals_in[row * N_TESTS + t];
  }
}

// scale [R, 6] = (W, p, ratio, med_c, med_b, N), scale_diff [R] int8,
// pvals_out [R, 6] (a copy of pvals_in with 0 in all six columns of a flagged
// row; both may be null), moments [R, 8] fp64 scratch.  inv_ratio = fl32(1 /
// min_ratio) from the host.  tier 0: the wave tier where each side holds at
// most 1024 columns, else the wide tier; tier 2: the wide tier (pooled width
// up to 8192).  cur and base need 4-byte alignment only.
FM_API int fm_pairwise_scale(const float* cur, int64_t ld_c, int n_cur, const float* base, int64_t ld_b, int n_base,
                             int64_t R, int min_points, float p_thr, float min_ratio, float inv_ratio, int both,
                             int tier, const float* pvals_in, double* moments, float* scale, int8_t* scale_diff,
                             float* pvals_out, hipStream_t stream) {
  if (R <= 0) return 0;
  if (n_cur < 0 || n_base < 0 || R > 0x7FFFFFFF || moments == nullptr || scale == nullptr || scale_diff == nullptr ||
      (pvals_in != nullptr && pvals_out == nullptr) || (tier != 0 && tier != 2) ||
      (((uintptr_t)cur | (uintptr_t)base) & 3) != 0)
    return (int)hipErrorInvalidValue;
  const int n = n_cur > n_base ? n_cur : n_base;
  if (tier == 0 && n <= kScaleWaveMax) {
    const dim3 grid((unsigned)((R + 3) / 4)), block(256);
#define FM_SCALE(KK)                                                                                                 \
  hipLaunchKernelGGL(scale_wave_kernel<KK>, grid, block, 0, stream, cur, ld_c, n_cur, base, ld_b, n_base, R, moments)
    if (n <= 64) FM_SCALE(1);
    else if (n <= 128) FM_SCALE(2);
    else if (n <= 256) FM_SCALE(4);
    else if (n <= 512) FM_SCALE(8);
    else FM_SCALE(16);
#undef FM_SCALE
  } else if ((int64_t)n_cur + n_base <= kScaleWideMax) {
    const size_t lds = row_key_bytes(n_cur) + row_key_bytes(n_base);
    hipLaunchKernelGGL(scale_wide_kernel, dim3((unsigned)R), dim3(kScaleNT), lds, stream, cur, ld_c, n_cur, base, ld_b,
                       n_base, R, moments);
  } else {
    return (int)hipErrorInvalidValue;
  }
  FM_LAUNCH_CHECK();
  hipLaunchKernelGGL(scale_finish_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, stream, moments, R,
                     min_points, p_thr, min_ratio, inv_ratio, both, pvals_in, scale, scale_diff, pvals_out);
  FM_LAUNCH_CHECK();
  return 0;
}
