// K23 hold-out score: how well each of up to 8 candidate forecasts predicted
// the held-out end of a history row, and which candidate that picks, one
// 256-thread workgroup per row.
//
// The held-out samples are read from HBM once and kept in LDS at their global
// alignment, as fm_radix_select.h keeps a row's keys (the row needs 4-byte
// alignment only), a sample that is not finite as NaN.  Each candidate's
// forecast and sigma are then streamed once against them: a point counts when
// sample, forecast and sigma are finite and sigma > 0, and adds ln sigma +
// min(|x - fc| / sigma, zcap) to the thread's fp64 partial sum.  An operand
// with column stride 0 is one value per row: it is read and tested once, and
// the logarithm of such a sigma is taken once and added n times at the end.
// The candidate's score is the mean over its points, +inf without one.
// Thread 0 then picks: among the candidates that scored at least half of the
// finite samples, the first within `margin` of the smallest score.  The
// contract is foremast_amd/ops/misc.py ref_holdout_score / ref_auto_pick.
#include "fm_common.h"
#include "fm_radix_select.h"

using namespace fm;

namespace {

constexpr int kHoldoutThreads = 256;
constexpr int kHoldoutMaxCands = 8;

// One candidate: forecast and sigma, each with a row stride in floats and a
// column stride of 0 (one value per row) or 1.
struct HoldoutCand {
  const float* fc;
  int64_t ldf;
  const float* sg;
  int64_t lds;
  int cf, cs;
};
struct HoldoutCands {
  HoldoutCand c[kHoldoutMaxCands];
};

static_assert(row_key_bytes(kRobustLdsKeys) + 1024 <= kLaunchLds, "the longest held-out row fits a launch");

__device__ __forceinline__ float finite_or_nan(float x) { return isfinite(x) ? x : quiet_nan(); }

// The row p[0..L) -> LDS words a .. a + L of xs (load_row_keys' layout and
// alignment handling: 16-B loads from the boundary on, the words of the first
// and last quad that the body leaves out by one thread each, NaN in front of
// and behind the row).  Returns the thread's count of finite samples.  No
// barrier.
template <int NT>
__device__ __forceinline__ int load_row_floats(const float* p, int L, int a, float4* xs) {
  const int tid = threadIdx.x;
  const int nq = row_quads(a, L);
  float* xw = reinterpret_cast<float*>(xs);
  int head = (4 - a) & 3;
  if (head > L) head = L;
  const int nb = (L - head) >> 2;
  const float4* b4 = reinterpret_cast<const float4*>(p + head);
  float4* d4 = xs + ((a + head) >> 2);
  int n = 0;
  for (int q = tid; q < nb; q += NT) {
    float4 x = b4[q];
    x = make_float4(finite_or_nan(x.x), finite_or_nan(x.y), finite_or_nan(x.z), finite_or_nan(x.w));
    n += (x.x == x.x) + (x.y == x.y) + (x.z == x.z) + (x.w == x.w);
    d4[q] = x;
  }
  if (tid < (nq > 1 ? 8 : 4)) {
    const int w = tid < 4 ? tid : 4 * (nq - 1) + (tid - 4);
    const int i = w - a;
    if (i < head || i >= head + 4 * nb) {
      float x = quiet_nan();
      if (i >= 0 && i < L) x = finite_or_nan(p[i]);
      n += x == x;
      xw[w] = x;
    }
  }
  return n;
}

// A thread's share of one candidate's sum.  PF / PS: forecast / sigma come per
// point and are tested per point; an operand of the row was tested before.
// With a sigma of the row the sum holds the misses alone.
struct HoldoutTally {
  double sum = 0.0;
  int n = 0;
  template <bool PF, bool PS>
  __device__ __forceinline__ void point(float x, float f, float s, float zcap) {
    bool ok = x == x;                                        // (staged: a sample that is not finite is NaN)
    if constexpr (PF) ok = ok && isfinite(f);
    if constexpr (PS) ok = ok && isfinite(s) && s > 0.f;
    if (!ok) return;
    const float z = fminf(__fdiv_rn(fabsf(__fsub_rn(x, f)), s), zcap);
    if constexpr (PS) sum += (double)logf(s) + (double)z;
    else sum += (double)z;
    ++n;
  }
};

// The points of one candidate over the samples xw[a .. a + L).  Where the
// operands that have a column share their 16-B alignment they are read as
// float4 from the boundary on, the up to three points either side of the
// whole quads by one thread each; otherwise a point per thread, coalesced.
template <int NT, bool PF, bool PS>
__device__ __forceinline__ HoldoutTally holdout_points(const float* xw, int a, int L, const float* __restrict__ f,
                                                       const float* __restrict__ s, float zcap) {
  const int tid = threadIdx.x;
  HoldoutTally t;
  const float f0 = PF ? 0.f : f[0], s0 = PS ? 0.f : s[0];
  if constexpr (!PF) if (!isfinite(f0)) return t;            // (workgroup-uniform)
  if constexpr (!PS) if (!(isfinite(s0) && s0 > 0.f)) return t;
  const bool vec = (PF || PS) && (!PF || !PS || row_word(f) == row_word(s));   // workgroup-uniform
  if (!vec) {
    for (int i = tid; i < L; i += NT) t.point<PF, PS>(xw[a + i], PF ? f[i] : f0, PS ? s[i] : s0, zcap);
  } else {
    int head = (4 - row_word(PF ? f : s)) & 3;               // points before the 16-B boundary
    if (head > L) head = L;
    const int nb = (L - head) >> 2;
    const float4* f4 = reinterpret_cast<const float4*>(f + head);
    const float4* s4 = reinterpret_cast<const float4*>(s + head);
    for (int q = tid; q < nb; q += NT) {
      const float4 fv = PF ? f4[q] : make_float4(f0, f0, f0, f0);
      const float4 sv = PS ? s4[q] : make_float4(s0, s0, s0, s0);
      const float* x = xw + a + head + 4 * q;
      t.point<PF, PS>(x[0], fv.x, sv.x, zcap);
      t.point<PF, PS>(x[1], fv.y, sv.y, zcap);
      t.point<PF, PS>(x[2], fv.z, sv.z, zcap);
      t.point<PF, PS>(x[3], fv.w, sv.w, zcap);
    }
    if (tid < 8) {
      const int i = tid < 4 ? tid : head + 4 * nb + (tid - 4);
      if (tid < 4 ? i < head : i < L) t.point<PF, PS>(xw[a + i], PF ? f[i] : f0, PS ? s[i] : s0, zcap);
    }
  }
  if constexpr (!PS) t.sum += (double)t.n * (double)logf(s0);   // the row's one logarithm, once per point
  return t;
}

template <int NT>
__global__ __launch_bounds__(NT) void holdout_score_kernel(const float* __restrict__ x, int64_t ldx, int L, int64_t R,
                                                           HoldoutCands cands, int C, float zcap, float margin,
                                                           float* __restrict__ score /*[R,C]*/,
                                                           int* __restrict__ cnt /*[R,C]*/, int* __restrict__ nx /*[R]*/,
                                                           int* __restrict__ choice /*[R]*/) {
  extern __shared__ __attribute__((aligned(16))) float4 s_x[];
  __shared__ double s_redd[NT / FM_WAVE];
  __shared__ int s_redi[NT / FM_WAVE];
  __shared__ float s_score[kHoldoutMaxCands];
  __shared__ int s_n[kHoldoutMaxCands];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float* p = x + row * ldx;
  const int a = row_word(p);
  const int nfin = block_sum<NT>(load_row_floats<NT>(p, L, a, s_x), s_redi);   // (barriers: the samples are visible)
  const float* xw = reinterpret_cast<const float*>(s_x);
  for (int c = 0; c < C; ++c) {
    const HoldoutCand& cd = cands.c[c];
    const float* f = cd.fc + row * cd.ldf;
    const float* s = cd.sg + row * cd.lds;
    HoldoutTally t;
    if (L > 0) {                                             // (an operand of the row is read: it has a column)
      if (cd.cf) t = cd.cs ? holdout_points<NT, true, true>(xw, a, L, f, s, zcap)
                           : holdout_points<NT, true, false>(xw, a, L, f, s, zcap);
      else t = cd.cs ? holdout_points<NT, false, true>(xw, a, L, f, s, zcap)
                     : holdout_points<NT, false, false>(xw, a, L, f, s, zcap);
    }
    const double sum = block_sum<NT>(t.sum, s_redd);
    const int n = block_sum<NT>(t.n, s_redi);
    if (tid == 0) {
      s_score[c] = n > 0 ? (float)(sum / (double)n) : __uint_as_float(0x7F800000u);
      s_n[c] = n;
    }
  }
  if (tid == 0) {                                            // (its own LDS writes: no barrier)
    const float inf = __uint_as_float(0x7F800000u);
    float best = inf;
    for (int c = 0; c < C; ++c) {
      score[row * C + c] = s_score[c];
      cnt[row * C + c] = s_n[c];
      if (s_n[c] >= 1 && 2 * s_n[c] >= nfin && s_score[c] < best) best = s_score[c];
    }
    const float lim = __fadd_rn(best, margin);
    int pick = 0;
    for (int c = C - 1; c >= 0; --c)
      if (s_n[c] >= 1 && 2 * s_n[c] >= nfin && s_score[c] <= lim) pick = c;
    nx[row] = nfin;
    choice[row] = pick;
  }
}

}  // namespace

// x [R, L] at row stride ldx: the held-out samples, 4-byte alignment only,
// L <= kRobustLdsKeys.  cands: HOST memory, C <= 8 rows of 6 int64 = (fc
// pointer, fc row stride, fc column stride 0|1, sigma pointer, sigma row
// stride, sigma column stride 0|1), strides in floats, read before the call
// returns.  Outputs: score [R, C] fp32, n [R, C] int32, nx [R] int32, choice
// [R] int32.
FM_API int fm_holdout_score(const float* x, int64_t ldx, int L, int64_t R, const int64_t* cands, int C, float zcap,
                            float margin, float* score, int* n, int* nx, int* choice, hipStream_t stream) {
  if (R <= 0) return 0;
  if (L < 0 || L > kRobustLdsKeys || C < 1 || C > kHoldoutMaxCands || R > 0x7FFFFFFF || cands == nullptr ||
      (((uintptr_t)x) & 3) != 0)
    return (int)hipErrorInvalidValue;
  HoldoutCands hc = {};
  for (int c = 0; c < C; ++c) {
    const int64_t* v = cands + 6 * c;
    if ((v[0] & 3) != 0 || (v[3] & 3) != 0 || v[0] == 0 || v[3] == 0 || (v[2] | 1) != 1 || (v[5] | 1) != 1)
      return (int)hipErrorInvalidValue;
    hc.c[c] = HoldoutCand{reinterpret_cast<const float*>((uintptr_t)v[0]), v[1],
                          reinterpret_cast<const float*>((uintptr_t)v[3]), v[4], (int)v[2], (int)v[5]};
  }
  hipLaunchKernelGGL(holdout_score_kernel<kHoldoutThreads>, dim3((unsigned)R), dim3(kHoldoutThreads), row_key_bytes(L),
                     stream, x, ldx, L, R, hc, C, zcap, margin, score, n, nx, choice);
  FM_LAUNCH_CHECK();
  return 0;
}
