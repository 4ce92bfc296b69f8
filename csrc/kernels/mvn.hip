// K12: joint multivariate-normal detector ("Three or more metrics" column of
// the model table).  A group is K rows (2 <= K <= 8) of one job, right-aligned
// on the same time columns.  The history gives the mean vector and the KxK
// covariance over the columns where all K members are finite; each current
// point is scored by its Mahalanobis distance in correlation space,
//   d = || L^-1 z ||,  z_a = (x_a - mu_a) / sigma_a,  L L' = R + 1e-6 I,
// and flagged when d > cut[lowered][k], the chi-square-calibrated cut for the
// k members that are not constant over the history (docs/BRAIN_SPEC.md §3).
//
// One 256-thread workgroup per group, template <K> so that the K + K(K+1)/2
// running sums (44 at K = 8) are registers.  Rows are addressed through
// rows[G, 8] (int32 row ids, -1 padding) into hist[R, ld] / cur[R, ld_c]: no
// gathered copy of the history is made, and nothing row-sized lives in
// registers, so T is unbounded.
//
// Moments.  Both forms run the same centred sweep: per thread, fp32 sums of
// d_j = x_j - s_j and d_a * d_b against a block-wide shift s, combined over
// the block in fp64 and corrected at the end (mu = s + S/N,
// M_ab = P_ab - S_a S_b / N).  They differ in where s comes from:
//   form 0  s = the mean of all complete columns (a mean sweep, then the
//           centred sweep: the history is read twice, the second time mostly
//           from L2 / the infinity cache);
//   form 1  s = the mean of the complete columns among the last 1024 (rows
//           are right-aligned, so the tail is the populated end); when the
//           tail holds no complete column the block takes the mean sweep.
// fm_mvn's `form` argument picks one.  Form 1 is the default of ops/misc.py,
// by measurement on an MI355X at 10,000 groups x K = 8 x T = 10,080: 0.862 ms
// against 1.115 ms for form 0 and 0.493 ms for one streaming read of the same
// buffer (fm_hist_stats), with equal distances to 1e-6 (docs/PERF.md,
// profiles/mvn_bench.jsonl).
//
// The kernel is bandwidth-bound (about 5.5 FMA per loaded float at K = 8):
// plain VALU FMAs, no MFMA.
#include "fm_common.h"
#include "fm_mvn.h"

using namespace fm;

namespace {

// One float4 of every member row: sums of the complete columns.
template <int K>
__device__ __forceinline__ void mean_step(const float4* const (&rp)[K], int qi, int T, float (&sum)[K], int& cnt) {
  float4 v[K];
#pragma unroll
  for (int j = 0; j < K; ++j) v[j] = rp[j][qi];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    bool ok = qi * 4 + e < T;
    float x[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      x[j] = e == 0 ? v[j].x : e == 1 ? v[j].y : e == 2 ? v[j].z : v[j].w;
      ok = ok && isfinite(x[j]);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) sum[j] += ok ? x[j] : 0.f;
    cnt += ok;
  }
}

}  // namespace

template <int K, bool TAIL>
__global__ __launch_bounds__(256) void mvn_kernel(const float* __restrict__ hist, int64_t ld, int T, int64_t R,
                                                  const float* __restrict__ cur, int64_t ld_c, int n,
                                                  const int* __restrict__ rows /*[G,8]*/,
                                                  const float* __restrict__ cuts /*[2,9]*/,
                                                  const unsigned char* __restrict__ lowered /*[G]*/, int min_n,
                                                  float* __restrict__ params /*[G,2+K+NP]*/,
                                                  float* __restrict__ dist /*[G,n]*/,
                                                  unsigned long long* __restrict__ flags, int NW,
                                                  int* __restrict__ count, int* __restrict__ valid) {
  constexpr int NA = MvnShared<K>::NA;
  __shared__ MvnShared<K> S;
  double* const sh = S.sh;
  double* const tot = S.tot;
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

  // ---- the shift
  float s[K];
  {
    float sum[K];
    int c = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) sum[j] = 0.f;
    bool have = false;
    if (TAIL) {
      const int qi = (nq > 256 ? nq - 256 : 0) + tid;
      if (qi < nq) mean_step<K>(rp, qi, T, sum, c);
      block_sum_arr<K>(sum, c, sh, tot);
      have = tot[K] > 0.0;
    }
    if (!have) {
#pragma unroll
      for (int j = 0; j < K; ++j) sum[j] = 0.f;
      c = 0;
      for (int qi = tid; qi < nq; qi += 256) mean_step<K>(rp, qi, T, sum, c);
      block_sum_arr<K>(sum, c, sh, tot);
    }
    const double c0 = tot[K];
#pragma unroll
    for (int j = 0; j < K; ++j) s[j] = c0 > 0.0 ? (float)(tot[j] / c0) : 0.f;
  }

  // ---- centred sums: acc[0..K) = sum d_j, acc[K..) = sum d_a d_b (a <= b, row-major)
  float acc[NA];
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < NA; ++i) acc[i] = 0.f;
  for (int qi = tid; qi < nq; qi += 256) {
    float4 v[K];
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = rp[j][qi];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bool ok = qi * 4 + e < T;
      float d[K];
#pragma unroll
      for (int j = 0; j < K; ++j) {
        d[j] = e == 0 ? v[j].x : e == 1 ? v[j].y : e == 2 ? v[j].z : v[j].w;
        ok = ok && isfinite(d[j]);
      }
#pragma unroll
      for (int j = 0; j < K; ++j) {
        d[j] = ok ? d[j] - s[j] : 0.f;
        acc[j] += d[j];
      }
      int idx = K;
#pragma unroll
      for (int a = 0; a < K; ++a)
#pragma unroll
        for (int b = a; b < K; ++b) { acc[idx] = fmaf(d[a], d[b], acc[idx]); ++idx; }
      cnt += ok;
    }
  }
  block_sum_arr<NA>(acc, cnt, sh, tot);

  // ---- moments ... flags: the back half shared with K17 (fm_mvn.h)
  mvn_finish<K>(S, s, rid, rows_ok, g, cur, ld_c, n, cuts, lowered, min_n, params, dist, flags, NW, count, valid);
}

template <int K>
static void mvn_launch(int form, dim3 grid, hipStream_t stream, const float* hist, int64_t ld, int T, int64_t R,
                       const float* cur, int64_t ld_c, int n, const int* rows, const float* cuts,
                       const unsigned char* lowered, int min_n, float* params, float* dist,
                       unsigned long long* flags, int NW, int* count, int* valid) {
  if (form == 1)
    hipLaunchKernelGGL((mvn_kernel<K, true>), grid, dim3(256), 0, stream, hist, ld, T, R, cur, ld_c, n, rows, cuts,
                       lowered, min_n, params, dist, flags, NW, count, valid);
  else
    hipLaunchKernelGGL((mvn_kernel<K, false>), grid, dim3(256), 0, stream, hist, ld, T, R, cur, ld_c, n, rows, cuts,
                       lowered, min_n, params, dist, flags, NW, count, valid);
}

// hist [R, ld], cur [R, ld_c], rows [G, 8] int32 (first K entries of each group
// used), cuts [2, 9], lowered [G] bytes.  form: 0 = mean sweep + centred
// sweep, 1 = tail shift + centred sweep.
FM_API int fm_mvn(const float* hist, int64_t ld, int T, int64_t R, const float* cur, int64_t ld_c, int n,
                  const int* rows, int64_t G, int K, const float* cuts, const unsigned char* lowered, int min_n,
                  int form, float* params, float* dist, unsigned long long* flags, int NW, int* count, int* valid,
                  hipStream_t stream) {
  if (G <= 0) return 0;
  if (K < 2 || K > 8 || T <= 0 || n <= 0 || R <= 0 || (ld & 3) || ld < T || ld_c < n ||
      (((uintptr_t)hist) & 15) || NW * 64 < n || G > 0x7fffffffLL || (form != 0 && form != 1))
    return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)G);
#define FM_MVN(KK) case KK: mvn_launch<KK>(form, grid, stream, hist, ld, T, R, cur, ld_c, n, rows, cuts, lowered, \
                                           min_n, params, dist, flags, NW, count, valid); break
  switch (K) {
    FM_MVN(2); FM_MVN(3); FM_MVN(4); FM_MVN(5); FM_MVN(6); FM_MVN(7); FM_MVN(8);
  }
#undef FM_MVN
  FM_LAUNCH_CHECK();
  return 0;
}
