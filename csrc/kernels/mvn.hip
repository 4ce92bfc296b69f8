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

using namespace fm;

namespace {

constexpr double MVN_RIDGE = 1e-6;

// acc[0..NA) and cnt summed over the 256 threads in fp64 -> tot[0..NA], the
// count last.  sh holds 4 * (NA + 1) doubles.
template <int NA>
__device__ __forceinline__ void block_sum_arr(const float (&acc)[NA], int cnt, double* sh, double* tot) {
  const int w = wave_id();
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const double v = wave_sum((double)acc[i]);
    if (lane_id() == 0) sh[w * (NA + 1) + i] = v;
  }
  const int c = wave_sum(cnt);
  if (lane_id() == 0) sh[w * (NA + 1) + NA] = (double)c;
  __syncthreads();
  const int t = threadIdx.x;
  if (t <= NA) tot[t] = (sh[t] + sh[(NA + 1) + t]) + (sh[2 * (NA + 1) + t] + sh[3 * (NA + 1) + t]);
  __syncthreads();
}

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
  constexpr int NP = K * (K + 1) / 2, NA = K + NP;
  __shared__ double sh[4 * (NA + 1)];
  __shared__ double tot[NA + 1];
  __shared__ double s_mu[K], s_isd[K], s_C[K * K], s_L[K * K];
  __shared__ float s_cut;
  __shared__ int s_ok;
  __shared__ int redi[4];
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

  // ---- moments, degeneracy, correlation + ridge, Cholesky (fp64, one thread, through LDS)
  if (tid == 0) {
    const double N = tot[NA];
    const int Ni = (int)N;
    const int need = min_n > K + 2 ? min_n : K + 2;
    const bool okg = Ni >= need;
    const double inv_n = N > 0.0 ? 1.0 / N : 0.0, den = N > 1.0 ? N - 1.0 : 1.0;
    float* pr = params + g * (2 + NA);
    int k = 0;
    int idx = K;
#pragma unroll
    for (int a = 0; a < K; ++a) {
      const double mu = (double)s[a] + tot[a] * inv_n;
      s_mu[a] = mu;
      pr[2 + a] = (float)mu;
#pragma unroll
      for (int b = a; b < K; ++b) {
        const double c = (tot[idx] - tot[a] * tot[b] * inv_n) / den;
        s_C[a * K + b] = c;
        s_C[b * K + a] = c;
        pr[2 + idx] = (float)c;
        ++idx;
      }
      const double caa = s_C[a * K + a];
      const bool live = caa > 1e-12 * mu * mu + 1e-30;
      s_isd[a] = live ? 1.0 / sqrt(caa) : 0.0;
      k += live;
    }
    pr[0] = (float)Ni;
    pr[1] = (float)k;
    // a constant member keeps a unit diagonal and zero couplings: it adds
    // nothing to the distance, which equals the one over the live members alone
#pragma unroll 1
    for (int a = 0; a < K; ++a) {
#pragma unroll 1
      for (int b = 0; b <= a; ++b) {
        double v = a == b ? 1.0 + MVN_RIDGE : s_C[a * K + b] * s_isd[a] * s_isd[b];
#pragma unroll 1
        for (int c = 0; c < b; ++c) v -= s_L[a * K + c] * s_L[b * K + c];
        s_L[a * K + b] = a == b ? sqrt(v > 1e-12 ? v : 1e-12) : v / s_L[b * K + b];
      }
    }
    s_cut = cuts[(lowered[g] ? 9 : 0) + k];
    s_ok = okg ? 1 : 0;
  }
  __syncthreads();

  // ---- current points, one per thread
  const bool okg = s_ok != 0;
  const float cut = s_cut;
  int nflag = 0, npres = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + tid;
    bool f = false;
    if (i < n) {
      float d = NAN;
      if (rows_ok) {
        bool present = true, moved = false;
        double y[K];
#pragma unroll
        for (int a = 0; a < K; ++a) {
          const float x = cur[rid[a] * ld_c + i];
          present = present && isfinite(x);
          const double mu = s_mu[a], isd = s_isd[a], dx = (double)x - mu;
          moved = moved || (isd == 0.0 && fabs(dx) > 1e-6 * fabs(mu) + 1e-12);
          double z = dx * isd;
#pragma unroll
          for (int b = 0; b < a; ++b) z -= s_L[a * K + b] * y[b];
          y[a] = z / s_L[a * K + a];
        }
        npres += present;
        if (present && okg) {
          double q = 0.0;
#pragma unroll
          for (int a = 0; a < K; ++a) q += y[a] * y[a];
          d = moved ? INFINITY : (float)sqrt(q);
          f = d > cut;
          nflag += f;
        }
      }
      dist[g * n + i] = d;
    }
    const unsigned long long bal = __ballot(f);
    const int w = i0 / 64 + wave_id();
    if (lane_id() == 0 && w < NW) flags[g * NW + w] = bal;
  }
  nflag = block_sum<256>(nflag, redi);
  npres = block_sum<256>(npres, redi);
  if (tid == 0) {
    count[g] = nflag;
    valid[g] = (okg ? 1 : 0) | (npres > 0 ? 2 : 0);
  }
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
