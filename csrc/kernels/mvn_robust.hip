// K17: robust joint detector (`robust_multivariate`).  K12's Mahalanobis
// decision over a group of K member rows (2 <= K <= 8), with the moments taken
// over the history columns that are not incident columns: a complete column t
// is set aside when any member has |x_jt - c_j| > reject * s_j, with (c_j, s_j)
// the member's median and MAD-sigma as K13 (fm_robust_stats) wrote them.  The
// contract is foremast_amd/ops/misc.py ref_mvn_robust (docs/BRAIN_SPEC.md §3).
//
// One 256-thread workgroup per group, template <K>, rows addressed through
// rows[G, 8] with float4 loads, nothing row-sized in registers or LDS: as K12.
//
// One centred sweep.  The shift is the member's median, known before the
// history is read, so K12's tail sweep and mean sweep are not needed.  Per
// element d_j = x_j - c_j; the column is used when every x_j is finite and no
// |d_j| exceeds lim_j; it counts as rejected when complete but not used.  The
// K + K(K+1)/2 sums of d_j and d_a d_b run in fp32 per thread and are combined
// over the block in fp64.
//
// The column set equals the oracle's bit for bit: lim_j is one fp32 product
// made once per member, d_j one fp32 subtraction, and the comparison is on
// the rounded difference.  Neither feeds an addition or takes a product, so
// the library's -ffp-contract=fast has nothing to fuse them with (the only
// fused operations are the accumulations fmaf(d_a, d_b, acc), on the already
// rounded d); the unit takes no flags of its own.
//
// Breakdown guard: when more than half of the complete columns were rejected
// (2 * rejected > complete, a block-uniform test after the first reduction),
// the robust start does not describe the bulk; the sweep runs again with the
// limits at +inf and the group reports rejected = 0, which is K12 on that
// group.  The second pass reads mostly from L2 / the infinity cache.
//
// Everything from the block totals on is K12's code (fm_mvn.h).
#include "fm_common.h"
#include "fm_mvn.h"

using namespace fm;

template <int K>
__global__ __launch_bounds__(256) void mvn_robust_kernel(const float* __restrict__ hist, int64_t ld, int T, int64_t R,
                                                         const float* __restrict__ cur, int64_t ld_c, int n,
                                                         const int* __restrict__ rows /*[G,8]*/,
                                                         const float* __restrict__ cuts /*[2,9]*/,
                                                         const unsigned char* __restrict__ lowered /*[G]*/, int min_n,
                                                         const float* __restrict__ stats /*[R,3]*/, float reject,
                                                         float* __restrict__ params /*[G,2+K+NP]*/,
                                                         float* __restrict__ dist /*[G,n]*/,
                                                         unsigned long long* __restrict__ flags, int NW,
                                                         int* __restrict__ count, int* __restrict__ valid,
                                                         int* __restrict__ rejected) {
  constexpr int NA = MvnShared<K>::NA;
  __shared__ MvnShared<K> S;
  const int64_t g = blockIdx.x;
  const int tid = threadIdx.x;

  int64_t rid[K];
  bool rows_ok = true;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    rid[j] = rows[g * 8 + j];
    rows_ok = rows_ok && rid[j] >= 0 && rid[j] < R;
  }
  // a group with a row id outside the buffer reads nothing and comes out invalid
  const int nq = rows_ok ? (T + 3) >> 2 : 0;
  const float4* rp[K];
#pragma unroll
  for (int j = 0; j < K; ++j) rp[j] = reinterpret_cast<const float4*>(hist + (rows_ok ? rid[j] : 0) * ld);

  // ---- shift and limits.  A member without a finite sample has NaN statistics: its shift is 0 (the
  // group has no complete column anyway) and its NaN limit compares false, as in the oracle.
  const bool rejecting = reject > 0.f && !isinf(reject);
  float c[K], lim[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const float med = rows_ok ? stats[rid[j] * 3] : 0.f;
    const float sg = rows_ok ? stats[rid[j] * 3 + 1] : 0.f;
    c[j] = isfinite(med) ? med : 0.f;
    lim[j] = rejecting ? __fmul_rn(reject, sg) : INFINITY;
  }

  // ---- centred sums over the columns kept: acc[0..K) = sum d_j, acc[K..) = sum d_a d_b (a <= b, row-major)
  int nrej;
  for (;;) {
    float acc[NA];
    int cnt = 0, rej = 0;
#pragma unroll
    for (int i = 0; i < NA; ++i) acc[i] = 0.f;
    for (int qi = tid; qi < nq; qi += 256) {
      float4 v[K];
#pragma unroll
      for (int j = 0; j < K; ++j) v[j] = rp[j][qi];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bool ok = qi * 4 + e < T, out = false;
        float d[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
          const float x = e == 0 ? v[j].x : e == 1 ? v[j].y : e == 2 ? v[j].z : v[j].w;
          ok = ok && isfinite(x);
          d[j] = __fsub_rn(x, c[j]);
          out = out || fabsf(d[j]) > lim[j];
        }
        const bool use = ok && !out;
#pragma unroll
        for (int j = 0; j < K; ++j) {
          d[j] = use ? d[j] : 0.f;
          acc[j] += d[j];
        }
        int idx = K;
#pragma unroll
        for (int a = 0; a < K; ++a)
#pragma unroll
          for (int b = a; b < K; ++b) { acc[idx] = fmaf(d[a], d[b], acc[idx]); ++idx; }
        cnt += use;
        rej += ok && out;
      }
    }
    block_sum_arr<NA>(acc, cnt, S.sh, S.tot);
    nrej = block_sum<256>(rej, S.redi);
    // block-uniform: S.tot and nrej are the same in every thread
    if (!(2.0 * (double)nrej > S.tot[NA] + (double)nrej)) break;
#pragma unroll
    for (int j = 0; j < K; ++j) lim[j] = INFINITY;              // the guard: nothing is rejected on the second pass
  }
  if (tid == 0) rejected[g] = nrej;

  // ---- moments ... flags: the back half shared with K12 (fm_mvn.h)
  mvn_finish<K>(S, c, rid, rows_ok, g, cur, ld_c, n, cuts, lowered, min_n, params, dist, flags, NW, count, valid);
}

// hist [R, ld], cur [R, ld_c], rows [G, 8] int32 (first K entries of each group
// used), cuts [2, 9], lowered [G] bytes, stats [R, 3] as fm_robust_stats writes
// them over the same T columns (only the member rows are read).  reject <= 0,
// NaN or +inf: nothing is rejected.
FM_API int fm_mvn_robust(const float* hist, int64_t ld, int T, int64_t R, const float* cur, int64_t ld_c, int n,
                         const int* rows, int64_t G, int K, const float* cuts, const unsigned char* lowered, int min_n,
                         const float* stats, float reject, float* params, float* dist, unsigned long long* flags,
                         int NW, int* count, int* valid, int* rejected, hipStream_t stream) {
  if (G <= 0) return 0;
  if (K < 2 || K > 8 || T <= 0 || n <= 0 || R <= 0 || (ld & 3) || ld < T || ld_c < n ||
      (((uintptr_t)hist) & 15) || NW * 64 < n || G > 0x7fffffffLL || stats == nullptr)
    return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)G);
#define FM_MVNR(KK) case KK: hipLaunchKernelGGL((mvn_robust_kernel<KK>), grid, dim3(256), 0, stream, hist, ld, T, R, \
                                                cur, ld_c, n, rows, cuts, lowered, min_n, stats, reject, params, dist, \
                                                flags, NW, count, valid, rejected); break
  switch (K) {
    FM_MVNR(2); FM_MVNR(3); FM_MVNR(4); FM_MVNR(5); FM_MVNR(6); FM_MVNR(7); FM_MVNR(8);
  }
#undef FM_MVNR
  FM_LAUNCH_CHECK();
  return 0;
}
