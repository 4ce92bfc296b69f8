// Device code shared by the joint Mahalanobis detectors: K12 (mvn.hip) and
// K17 (mvn_robust.hip).  Both run one 256-thread workgroup per group of K
// member rows and differ only in which history columns their centred sweep
// sums; everything from the block totals on is the same code:
//   block_sum_arr  per-thread fp32 sums and a count -> block totals in fp64
//   MvnShared      the LDS a group's decision lives in
//   mvn_finish     moments, live test, correlation + ridge + Cholesky (fp64,
//                  one thread), the scoring loop over the current points,
//                  flags by ballot, count and valid
#pragma once
#include "fm_common.h"

namespace fm {

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

template <int K>
struct MvnShared {
  static constexpr int NP = K * (K + 1) / 2, NA = K + NP;
  double sh[4 * (NA + 1)];
  double tot[NA + 1];
  double mu[K], isd[K], C[K * K], L[K * K];
  float cut;
  int ok;
  int redi[4];
};

// From the block totals S.tot (sums of d_j = x_j - s_j, of d_a d_b for a <= b
// row-major, and the column count N) to the group's outputs: mu = s + S / N,
// M_ab = P_ab - S_a S_b / N.  Called by every thread of the block.
template <int K>
__device__ __forceinline__ void mvn_finish(MvnShared<K>& S, const float (&s)[K], const int64_t (&rid)[K], bool rows_ok,
                                           int64_t g, const float* __restrict__ cur, int64_t ld_c, int n,
                                           const float* __restrict__ cuts /*[2,9]*/,
                                           const unsigned char* __restrict__ lowered /*[G]*/, int min_n,
                                           float* __restrict__ params /*[G,2+K+NP]*/, float* __restrict__ dist /*[G,n]*/,
                                           unsigned long long* __restrict__ flags, int NW, int* __restrict__ count,
                                           int* __restrict__ valid) {
  constexpr int NA = MvnShared<K>::NA;
  const int tid = threadIdx.x;
  const double* tot = S.tot;

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
      S.mu[a] = mu;
      pr[2 + a] = (float)mu;
#pragma unroll
      for (int b = a; b < K; ++b) {
        // one column has no spread: exactly 0, where a shift that is not the column itself (K17's
        // median) would leave the rounding of the fp32 products
        const double c = Ni > 1 ? (tot[idx] - tot[a] * tot[b] * inv_n) / den : 0.0;
        S.C[a * K + b] = c;
        S.C[b * K + a] = c;
        pr[2 + idx] = (float)c;
        ++idx;
      }
      const double caa = S.C[a * K + a];
      const bool live = caa > 1e-12 * mu * mu + 1e-30;
      S.isd[a] = live ? 1.0 / sqrt(caa) : 0.0;
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
        double v = a == b ? 1.0 + MVN_RIDGE : S.C[a * K + b] * S.isd[a] * S.isd[b];
#pragma unroll 1
        for (int c = 0; c < b; ++c) v -= S.L[a * K + c] * S.L[b * K + c];
        S.L[a * K + b] = a == b ? sqrt(v > 1e-12 ? v : 1e-12) : v / S.L[b * K + b];
      }
    }
    S.cut = cuts[(lowered[g] ? 9 : 0) + k];
    S.ok = okg ? 1 : 0;
  }
  __syncthreads();

  // ---- current points, one per thread
  const bool okg = S.ok != 0;
  const float cut = S.cut;
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
          const double mu = S.mu[a], isd = S.isd[a], dx = (double)x - mu;
          moved = moved || (isd == 0.0 && fabs(dx) > 1e-6 * fabs(mu) + 1e-12);
          double z = dx * isd;
#pragma unroll
          for (int b = 0; b < a; ++b) z -= S.L[a * K + b] * y[b];
          y[a] = z / S.L[a * K + a];
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
  nflag = block_sum<256>(nflag, S.redi);
  npres = block_sum<256>(npres, S.redi);
  if (tid == 0) {
    count[g] = nflag;
    valid[g] = (okg ? 1 : 0) | (npres > 0 ? 2 : 0);
  }
}

}  // namespace fm
