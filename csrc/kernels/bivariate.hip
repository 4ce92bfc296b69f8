// K5: bivariate normal detector ("Two Metrics" column of the model table,
// docs/guides/design.md:74-79).  For a metric pair (a, b) of one service the
// history gives the mean vector and 2x2 covariance; each current point pair is
// scored by its Mahalanobis distance d = sqrt(dx' S^-1 dx) and flagged when
// d > threshold (threshold in sigma units, like the univariate models).
// A history pair counts when both members are finite; fewer than two pairs
// give d = NaN and no flag.  S is the covariance with a relative ridge on its
// diagonal (below); ops/misc.py ref_bivariate is the contract.  T <= 16384.
//
// One 256-thread workgroup per pair; both history rows are read once with
// 16-B loads and kept in registers for the two-pass moments.
#include "fm_common.h"

using namespace fm;

// ops/misc.py BIVARIATE_RIDGE
constexpr double kBivariateRidge = 1e-6;

template <int NV>
__global__ __launch_bounds__(256) void bivariate_kernel(const float* __restrict__ ha, const float* __restrict__ hb,
                                                        int64_t ld_h, int T, const float* __restrict__ ca,
                                                        const float* __restrict__ cb, int64_t ld_c, int n,
                                                        int64_t P, const float* __restrict__ thr,
                                                        float* __restrict__ params /*[P,5]*/,
                                                        float* __restrict__ dist /*[P,n]*/,
                                                        unsigned long long* __restrict__ flags, int NW,
                                                        int* __restrict__ count) {
  __shared__ double red[4];
  __shared__ int redi[4];
  const int64_t p = blockIdx.x;
  const int tid = threadIdx.x;
  const float4* ra = reinterpret_cast<const float4*>(ha + p * ld_h);
  const float4* rb = reinterpret_cast<const float4*>(hb + p * ld_h);
  const int nq = (T + 3) >> 2;
  float4 qa[NV], qb[NV];
  double sa = 0, sb = 0;
  int c = 0;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int qi = tid + j * 256;
    float4 a = make_float4(NAN, NAN, NAN, NAN), b = a;
    if (qi < nq) {
      a = ra[qi]; b = rb[qi];
      const int e0 = qi * 4;
      if (e0 + 1 >= T) { a.y = NAN; b.y = NAN; }
      if (e0 + 2 >= T) { a.z = NAN; b.z = NAN; }
      if (e0 + 3 >= T) { a.w = NAN; b.w = NAN; }
    }
    // a pair counts only when both coordinates are present
    if (!(isfinite(a.x) && isfinite(b.x))) { a.x = NAN; b.x = NAN; }
    if (!(isfinite(a.y) && isfinite(b.y))) { a.y = NAN; b.y = NAN; }
    if (!(isfinite(a.z) && isfinite(b.z))) { a.z = NAN; b.z = NAN; }
    if (!(isfinite(a.w) && isfinite(b.w))) { a.w = NAN; b.w = NAN; }
    qa[j] = a; qb[j] = b;
    if (isfinite(a.x)) { sa += a.x; sb += b.x; ++c; }
    if (isfinite(a.y)) { sa += a.y; sb += b.y; ++c; }
    if (isfinite(a.z)) { sa += a.z; sb += b.z; ++c; }
    if (isfinite(a.w)) { sa += a.w; sb += b.w; ++c; }
  }
  sa = block_sum<256>(sa, red);
  sb = block_sum<256>(sb, red);
  c = block_sum<256>(c, redi);
  const float ma = c > 0 ? (float)(sa / c) : 0.f, mb = c > 0 ? (float)(sb / c) : 0.f;
  // fp32 deviations (the rows stay fp32 in registers), their products summed in
  // fp64: the determinant below cancels to 1e-6 of its terms for a dependent
  // pair, where fp32 sums (1e-7) would leave it mostly noise.
  double vaa = 0, vbb = 0, vab = 0;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const float av[4] = {qa[j].x, qa[j].y, qa[j].z, qa[j].w};
    const float bv[4] = {qb[j].x, qb[j].y, qb[j].z, qb[j].w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (isfinite(av[e])) {
        const float fa = av[e] - ma, fb = bv[e] - mb;
        const double da = fa, db = fb;
        vaa += da * da; vbb += db * db; vab += da * db;
      }
    }
  }
  const double saa = block_sum<256>(vaa, red), sbb = block_sum<256>(vbb, red), sab = block_sum<256>(vab, red);
  const double den = c > 1 ? (double)(c - 1) : 1.0;
  const double Caa = saa / den, Cbb = sbb / den, Cab = sab / den;
  // S = C with its diagonal scaled by 1 + ridge (the ridge K12 puts on the
  // correlation matrix, MVN_RIDGE): positive definite for any C, independent of
  // the members' units; the 1e-30 keeps a constant member finite.  The inverse
  // and the quadratic form are fp64: for a dependent pair the three terms cancel
  // to 1e-6 of their size, which fp32 (6e-8) turned into distances of 0 .. 16
  // for points 0 .. 5 sigma along the line.
  const double Saa = Caa * (1.0 + kBivariateRidge) + 1e-30, Sbb = Cbb * (1.0 + kBivariateRidge) + 1e-30;
  const double det = Saa * Sbb - Cab * Cab;
  const float th = thr[0];
  int cnt = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + tid;
    bool f = false;
    if (i < n) {
      const float xa = ca[p * ld_c + i], xb = cb[p * ld_c + i];
      float d = NAN;
      if (isfinite(xa) && isfinite(xb) && c > 1) {
        const double da = (double)xa - ma, db = (double)xb - mb;
        const double q = (da * da * Sbb - 2.0 * da * db * Cab + db * db * Saa) / det;
        d = (float)sqrt(fmax(q, 0.0));
        f = d > th;
        cnt += f;
      }
      dist[p * n + i] = d;
    }
    const unsigned long long bal = __ballot(f);
    const int w = i0 / 64 + wave_id();
    if (lane_id() == 0 && w < NW) flags[p * NW + w] = bal;
  }
  cnt = block_sum<256>(cnt, redi);
  if (tid == 0) {
    params[p * 5 + 0] = ma; params[p * 5 + 1] = mb;
    params[p * 5 + 2] = (float)Caa; params[p * 5 + 3] = (float)Cab; params[p * 5 + 4] = (float)Cbb;
    count[p] = cnt;
  }
}

FM_API int fm_bivariate(const float* ha, const float* hb, int64_t ld_h, int T, const float* ca, const float* cb,
                        int64_t ld_c, int n, int64_t P, const float* thr, float* params, float* dist,
                        unsigned long long* flags, int NW, int* count, hipStream_t stream) {
  if (P <= 0) return 0;
  if ((ld_h & 3) || (((uintptr_t)ha) & 15) || (((uintptr_t)hb) & 15) || NW * 64 < n) return (int)hipErrorInvalidValue;
  const int nq = (T + 3) / 4;
  const dim3 grid((unsigned)P), block(256);
#define FM_BV(NVV) hipLaunchKernelGGL(bivariate_kernel<NVV>, grid, block, 0, stream, ha, hb, ld_h, T, ca, cb, ld_c, n, \
                                      P, thr, params, dist, flags, NW, count)
  if (nq <= 256 * 2) FM_BV(2);
  else if (nq <= 256 * 4) FM_BV(4);
  else if (nq <= 256 * 8) FM_BV(8);
  else if (nq <= 256 * 10) FM_BV(10);
  else if (nq <= 256 * 16) FM_BV(16);
  else return (int)hipErrorInvalidValue;
#undef FM_BV
  FM_LAUNCH_CHECK();
  return 0;
}
