// fm-hipcc-flags: -mllvm -pragma-unroll-threshold=1000000 -ffp-contract=off
// (the unroll threshold as in pairwise.hip: the K = 16 bitonic network must
// unroll fully to stay in registers.  Contraction is off because the gate's
// `min_shift * |base_med| + min_shift_abs` and the median's
// `0.5f * lo + 0.5f * up` are defined as separately rounded fp32 operations;
// an fma would round once and break the bit-for-bit contract with the numpy
// reference.)
//
// K19: effect size of current vs baseline, one wave per (service, metric) row.
//
// Over all N = n1 * n2 pairs of finite samples, d_ij = fl32(x_i - y_j):
//   gt = #{d > 0}, lt = #{d < 0}, Cliff's delta = (gt - lt) / N,
//   Hodges-Lehmann shift = median of the d_ij, base_med = median of the y_j.
// The pairs are never materialised.  fp32 round-to-nearest subtraction is
// monotone, so with the baseline sorted ascending d_ij is non-increasing in j
// for every i: the pairs of x_i with d > t are a prefix of the sorted
// baseline, its length p_i(t) found by binary search (the baseline sits in
// LDS, x_i in a register of lane i), and #{d <= t} = sum_i (n2 - p_i(t)).
// The median is selected MSB-first over the order-preserving 32-bit key of d:
// one such count per key bit, exact for every input, ties included.  Three
// things keep a count cheap:
//   * the compare runs on floats (d > t with t decoded from the trial key once
//     per step, on the scalar unit), not on keys;
//   * p_i is monotone in t, so every lane keeps the bracket [p_i(upper end),
//     p_i(lower end)] of the key interval still in play and searches only
//     inside it: after a few steps most brackets are one or two wide;
//   * the bisection stops as soon as exactly one pair is left in the interval
//     (counts at its two ends differ by one): that pair is the answer, and the
//     brackets already point at it.  Long tie runs at the median are the case
//     that runs all 32 steps.
// gt and lt are two more counts, at the keys of -0 and +0 (the first is the
// bisection's own first step).
//
// Signed zeros: inputs are canonicalised to +0 on load, so no difference is
// ever -0 (x - x = +0 under round-to-nearest) and the float order of the d is
// their key order even across a tie run of mixed zeros.  fp32 denormals are
// kept in this build (see fm_pairwise.h), so subtraction and compare tell
// subnormal differences apart exactly as the keys do.
#include "fm_pairwise.h"

namespace {

// Order-preserving key of a float, +-inf included (an overflowed difference
// sorts at its end).  No NaN reaches it: both operands are finite.
__device__ __forceinline__ unsigned eff_key(float x) {
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float eff_val(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

constexpr unsigned kKeyNegInf = 0x007FFFFFu;    // keys below it decode to NaN: no difference is <= them
constexpr unsigned kKeyNegZero = 0x7FFFFFFFu;   // every d < 0 has a key <= this one

// The float t with  key(d) > T  <=>  d > t  for every difference d (never
// -0, never NaN), for T >= kKeyNegInf.  T above key(+inf) decodes to NaN and
// d > NaN is false for all d, which is the right answer there too.
__device__ __forceinline__ float eff_threshold(unsigned T) {
  // key(d) > key(-0)  <=>  d >= +0  <=>  d > the largest negative subnormal
  return eff_val(T == kKeyNegZero ? kKeyNegZero - 1u : T);
}

// One counting step: for every current sample x[k] of this lane, the length
// p[k] of the baseline prefix with x - ys[j] > t, searched inside the lane's
// bracket [plo[k], phi[k]]; returns #{pairs with d <= t} (wave-uniform).  A
// missing x carries the empty bracket [n2, n2] and counts nothing.  The K
// searches of a lane advance together, so their LDS reads overlap.
template <int K>
__device__ __forceinline__ int count_step(const float (&x)[K], int nk, const float* __restrict__ ys, int n2, float t,
                                          const int (&plo)[K], const int (&phi)[K], int (&p)[K]) {
  int lo[K], hi[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { lo[k] = plo[k]; hi[k] = phi[k]; }
  bool more;
  do {
    more = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (k < nk) {
        const bool act = lo[k] < hi[k];
        const int mid = act ? (lo[k] + hi[k]) >> 1 : 0;        // lo <= mid < hi <= n2: inside the sorted baseline
        const bool g = (x[k] - ys[mid]) > t;
        lo[k] = act && g ? mid + 1 : lo[k];
        hi[k] = act && !g ? mid : hi[k];
        more |= lo[k] < hi[k];
      }
    }
  } while (more);
  int c = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    p[k] = lo[k];
    if (k < nk) c += n2 - lo[k];
  }
  return wave_sum_uniform(c);
}

// Smallest key among the pairs just outside the prefixes q[k] (the pair
// (x[k], ys[q[k] - 1]) is the lane's smallest d above the threshold the
// prefix belongs to); 0xFFFFFFFF if there is none.  Wave-uniform.
template <int K>
__device__ __forceinline__ unsigned min_key_at(const float (&x)[K], int nk, const float* __restrict__ ys,
                                               const int (&q)[K]) {
  unsigned m = 0xFFFFFFFFu;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (k < nk) {
      const unsigned kk = eff_key(x[k] - ys[q[k] > 0 ? q[k] - 1 : 0]);
      if (x[k] != kPad && q[k] > 0) m = kk < m ? kk : m;
    }
  }
  return ~wave_max_uniform(~m);
}

}  // namespace

template <int K>
__global__ __launch_bounds__(256) void pairwise_effect_kernel(
    const float* __restrict__ cur, int64_t ld_c, int n_cur, const float* __restrict__ base, int64_t ld_b, int n_base,
    int64_t R, float min_effect, float min_shift, float min_shift_abs, int directional,
    const int* __restrict__ bound, int M, const float* __restrict__ pvals_in, float* __restrict__ effect,
    int* __restrict__ counts, int8_t* __restrict__ passed, float* __restrict__ pvals_gated) {
  __shared__ float lds[4 * 64 * K];
  float* ys = lds + wave_id() * (64 * K);
  const int lane = lane_id();
  const int nk = (n_cur + 63) >> 6;
  const float qnan = __uint_as_float(0x7FC00000u);
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
      x[k] = okx ? (xv == 0.f ? 0.f : xv) : kPad;
      y[k] = oky ? (yv == 0.f ? 0.f : yv) : kPad;
      n1 += __popcll(__ballot(okx));
      n2 += __popcll(__ballot(oky));
    }
    int tag_unused[K];
    bitonic_sort<K, false, false>(y, tag_unused);
#pragma unroll
    for (int k = 0; k < K; ++k) ys[k * 64 + lane] = y[k];
    __builtin_amdgcn_wave_barrier();   // LDS stores of this wave visible to its own reads
    __builtin_amdgcn_s_waitcnt(0xc07f);

    const int N = n1 * n2;
    int gt = 0, lt = 0;
    float delta = qnan, shift = qnan, bmed = qnan;
    if (N > 0) {
      // brackets of the prefix lengths: plo = p at the interval's upper end
      // (fewest pairs above), phi = p at its lower end
      int plo[K], phi[K], p[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const bool ok = x[k] != kPad;
        plo[k] = ok ? 0 : n2;
        phi[k] = n2;
      }
      gt = N - count_step<K>(x, nk, ys, n2, 0.f, plo, phi, p);      // #{d <= +0}
      // lower middle: the smallest key whose "<=" count reaches rank + 1.
      // Invariant: c_lo = #{key < pre} < need <= c_hi = #{key <= pre | rest}.
      const int need = ((N - 1) >> 1) + 1;
      unsigned pre = 0;
      int c_lo = 0, c_hi = N, bit = 31;
      // (the first step always runs: it is also the count of the negatives)
      for (; bit >= 0 && (bit == 31 || c_hi - c_lo > 1); --bit) {
        const unsigned trial = pre | ((1u << bit) - 1u);
        int cnt = 0;
        if (trial >= kKeyNegInf) {
          cnt = count_step<K>(x, nk, ys, n2, eff_threshold(trial), plo, phi, p);
        } else {
#pragma unroll
          for (int k = 0; k < K; ++k) p[k] = phi[k];              // below every difference: all pairs above
        }
        if (bit == 31) lt = cnt;                                   // trial == key(-0): #{d < 0}
        const bool upper = cnt >= need;
        if (upper) c_hi = cnt; else { c_lo = cnt; pre |= 1u << bit; }
#pragma unroll
        for (int k = 0; k < K; ++k) {
          plo[k] = upper ? p[k] : plo[k];
          phi[k] = upper ? phi[k] : p[k];
        }
      }
      // all bits decided: the interval is the key itself; stopped early: the
      // one pair left in it is the smallest above its lower end
      const unsigned klo = bit < 0 ? pre : min_key_at<K>(x, nk, ys, phi);
      // #{key <= klo} == c_hi either way; the upper middle is the next pair up
      unsigned kup = klo;
      if ((N & 1) == 0 && c_hi < need + 1) kup = min_key_at<K>(x, nk, ys, plo);
      delta = __fdiv_rn((float)(gt - lt), (float)N);
      shift = 0.5f * eff_val(klo) + 0.5f * eff_val(kup);
      bmed = 0.5f * ys[(n2 - 1) >> 1] + 0.5f * ys[n2 >> 1];
    }
    __builtin_amdgcn_wave_barrier();   // the LDS slot is reused by the next row

    bool pass = true;
    if (N > 0 && !isnan(delta) && !isnan(shift)) {
      if (min_effect > 0.f && fabsf(delta) < min_effect) pass = false;
      if (min_shift > 0.f || min_shift_abs > 0.f) {
        const float a = fabsf(shift);
        const float need_shift = min_shift * fabsf(bmed) + min_shift_abs;
        if (!(a > 0.f && a >= need_shift)) pass = false;
      }
      if (directional != 0 && bound != nullptr) {
        const int bc = bound[(int)(row % M)];
        if (bc == 1 && shift <= 0.f) pass = false;
        if (bc == 2 && shift >= 0.f) pass = false;
      }
    }
    if (lane == 0) {
      float4 e;
      e.x = delta; e.y = shift; e.z = bmed; e.w = (float)N;
      *reinterpret_cast<float4*>(effect + row * 4) = e;
      counts[row * 2] = gt;
      counts[row * 2 + 1] = lt;
      passed[row] = pass ? 1 : 0;
    }
    if (pvals_in != nullptr && lane < N_TESTS)
      pvals_gated[row * N_TESTS + lane] = pass ? pvals_in[row * N_TESTS + lane] : qnan;
  }
}

// effect [R, 4] = (delta, shift, base_med, N), counts [R, 2] = (gt, lt),
// passed [R] int8, pvals_gated [R, 6] (a copy of pvals_in where the row
// passes, NaN where it does not; both may be null).  Each side holds at most
// 1024 samples.  bound [M] is read only when directional != 0.
FM_API int fm_pairwise_effect(const float* cur, int64_t ld_c, int n_cur, const float* base, int64_t ld_b, int n_base,
                              int64_t R, float min_effect, float min_shift, float min_shift_abs, int directional,
                              const int* bound, int M, const float* pvals_in, float* effect, int* counts,
                              int8_t* passed, float* pvals_gated, hipStream_t stream) {
  if (R <= 0) return 0;
  if (n_cur < 0 || n_base < 0 || M <= 0 || (pvals_in != nullptr && pvals_gated == nullptr))
    return (int)hipErrorInvalidValue;
  const int n = n_cur > n_base ? n_cur : n_base;
  const dim3 grid((unsigned)((R + 3) / 4)), block(256);
#define FM_EFF(KK)                                                                                                   \
  hipLaunchKernelGGL(pairwise_effect_kernel<KK>, grid, block, 0, stream, cur, ld_c, n_cur, base, ld_b, n_base, R,     \
                     min_effect, min_shift, min_shift_abs, directional, bound, M, pvals_in, effect, counts, passed,  \
                     pvals_gated)
  if (n <= 64) FM_EFF(1);
  else if (n <= 128) FM_EFF(2);
  else if (n <= 256) FM_EFF(4);
  else if (n <= 512) FM_EFF(8);
  else if (n <= 1024) FM_EFF(16);
  else return (int)hipErrorInvalidValue;
#undef FM_EFF
  FM_LAUNCH_CHECK();
  return 0;
}
