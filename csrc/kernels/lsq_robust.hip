// K36: robust prophet fit, Huber IRLS on a per-row weighted Gram matrix
// (foremast_amd/ops/lsq.py ref_prophet_fit_robust is the definition).  K10
// (lsq.hip) projects every row onto ONE orthonormal basis U and so needs no
// Gram matrix; with per-sample weights (Huber weights for incidents, zero for a
// missing sample) every row has its own G = U^T W U, and it changes with every
// reweighting.  Here a 256-thread workgroup owns ROWS rows and runs the whole
// fit of them in one launch:
//
//   stage    r = y - c as order-preserving keys in LDS (fm_radix_select.h: a
//            missing sample is the missing key), 16-B loads.  r is the only
//            per-sample state; weights are recomputed from (r, k s) on use.
//   1 + iters passes, each:
//     gram     the four waves split the row's 64-sample chunks.  Lane (i =
//              lane & 31, h = lane >> 5) loads XT[i][tb .. tb + 32), tb = t0 +
//              32 h (K10's permuted reduction order: 8 x 16-B loads, whole
//              128-B lines), reads the 32 keys of its half from LDS (broadcast)
//              and issues 32 v_mfma_f32_32x32x2_f32 with A = w_t x, B = x into
//              one 16-VGPR tile per row; g_i += (w_t x) r_t rides on the VALU.
//              With ROWS = 2 the loaded x feeds both rows' MFMAs.
//     reduce   the waves' tiles and g partials meet in LDS; all threads sum
//              and symmetrise G in fp32.
//     solve    wave rho solves row rho in fp64 with the matrix in registers:
//              lane j holds column j of G and g_j below it (the augmented
//              row), a right-looking Cholesky broadcasts the pivot column by
//              readlane, which leaves y = L^-1 g in the augmented row; the
//              back substitution runs over the same columns.  z += dz.
//     update   r_t -= sum_i XT[i][t] dz_i, every thread its quads (coalesced
//              along t), the new keys' count and range tallied on the way.
//     scale    s = K13's sigma of r: median_sigma over the LDS words
//              (LdsSpan: the deviations on the fly, the keys stay).  s == 0
//              ends the row's passes.
//   outputs  z, c, the last s, the finite count, the sum of the last weights
//            and the fallback flag (fewer than 2 p finite samples: not fitted).
//
// LDS per workgroup: the shared block below (bins, 4 tiles a row, G, partials)
// and ROWS rows of keys rounded up to whole 64-sample chunks; at T = 10,080
// and ROWS = 1 that is 70 KB, so two workgroups share a CU's 160 KB.
#include "fm_chol_regs.h"
#include "fm_common.h"
#include "fm_radix_select.h"

using namespace fm;

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int kNT = 256;
constexpr int kWaves = kNT / FM_WAVE;
constexpr int kF = 32;
constexpr double kRidge = 1e-6;                  // foremast_amd/ops/lsq.py LSQ_ROBUST_RIDGE mirrors it
constexpr int kMaxIters = 16;
constexpr size_t kCuLds = 160 * 1024;            // a single gfx950 workgroup may take the whole LDS
constexpr int kDefaultRows = 1;

template <int ROWS>
struct RobustShared {
  SelectScratch<kNT> sc;
  alignas(16) float tile[ROWS][kWaves][kF * kF];  // a wave's partial Gram tile
  alignas(16) float G[ROWS][kF * kF];             // their symmetrised sum
  float gpart[ROWS][kWaves][kF];
  double z[ROWS][kF];
  float dz[ROWS][kF];
};

constexpr int padded(int T) { return (T + 63) & ~63; }
template <int ROWS>
constexpr size_t lds_bytes(int T) {
  return sizeof(RobustShared<ROWS>) + (size_t)ROWS * padded(T) * sizeof(unsigned);
}

// Huber weight of the sample with key `key` at threshold ks = k s (+inf: plain
// least squares); r = the residual, 0 for a missing sample, whose weight is 0.
__device__ __forceinline__ float huber_weight(unsigned key, float ks, float& r) {
  const bool fin = key != kMissing;
  r = fin ? dec_key(key) : 0.f;
  return fin ? fminf(1.f, ks * __builtin_amdgcn_rcpf(fabsf(r))) : 0.f;
}

// One wave: dz = (G + ridge)^-1 g in fp64, z += dz (the ridge conditions the
// solve only: with no - ridge z in g the corrections converge to the
// unregularised solution).  Lane j and lane j + 32 hold the same column; the
// columns >= p (dropped from the basis: G is zero there) get a unit diagonal
// and a zero right-hand side.
__device__ __forceinline__ void solve_row(const float* G, const float (*gpart)[kF], double* z, float* dz, int p) {
  const int lane = lane_id(), j = lane & 31;
  double a[kF + 1];
#pragma unroll
  for (int i = 0; i < kF; ++i) {
    a[i] = (double)G[i * kF + j];
    if (i == j) a[i] = j < p ? a[i] + kRidge : 1.0;
  }
  float g = 0.f;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) g += gpart[w][j];
  const double zj = z[j];
  a[kF] = j < p ? (double)g : 0.0;
  // right-looking Cholesky (fm_chol_regs.h): a[i] = L[i][j] below the diagonal,
  // a[j] = 1 / L[j][j], and the augmented row turns into y = L^-1 g
  chol_columns<kF, kF + 1>(a, j);
  // L^T x = y: lane m finishes x_m, the lanes below it take L[m][j] x_m off
  double acc = a[kF], x = 0.0;
#pragma unroll
  for (int m = kF - 1; m >= 0; --m) {
    const double xm = bcast_f64(acc * a[m], m);
    x = j == m ? xm : x;
    acc = j < m ? fma(-a[m], xm, acc) : acc;
  }
  if (lane < kF) {
    z[j] = zj + x;
    dz[j] = (float)x;
  }
}

// (the second launch bound: two waves a SIMD for the one-row form, whose LDS lets two workgroups share a CU)
template <int ROWS>
__global__ __launch_bounds__(kNT, 3 - ROWS) void lsq_robust_fit_kernel(
    const float* __restrict__ Y, int64_t ld_y, int T, int64_t R, const float* __restrict__ XT, int64_t ld_x, int p,
    float khub, int iters, float* __restrict__ Z, float* __restrict__ shift, float* __restrict__ sigma,
    int* __restrict__ nfin, float* __restrict__ wsum, int* __restrict__ fallback) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_mem[];
  static_assert(sizeof(RobustShared<ROWS>) % 16 == 0, "the keys behind the shared block stay 16-B aligned");
  RobustShared<ROWS>& s = *reinterpret_cast<RobustShared<ROWS>*>(s_mem);
  unsigned* const keys = reinterpret_cast<unsigned*>(s_mem) + sizeof(RobustShared<ROWS>) / sizeof(unsigned);
  const int TP = padded(T);
  const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
  const int64_t row0 = (int64_t)blockIdx.x * ROWS;
  const float inf = __uint_as_float(0x7F800000u);
  const bool huber = isfinite(khub) && khub > 0.f;

  // ---- stage: r = y - c as keys, the words behind T missing
  s.sc.clear_bins();
  if (tid < ROWS * kF) s.z[tid / kF][tid % kF] = 0.0;
  int n[ROWS];
  float c0[ROWS], ks[ROWS], sg[ROWS];
  bool fit[ROWS], act[ROWS];
#pragma unroll
  for (int q = 0; q < ROWS; ++q) {
    unsigned* kw = keys + q * TP;
    RowTally tl;
    c0[q] = 0.f;
    if (row0 + q < R) {
      const float* yr = Y + (row0 + q) * ld_y;
      float c = yr[0];
      if (!isfinite(c)) c = 0.f;
      c0[q] = c;
      const int nq = T >> 2;
      for (int u = tid; u < nq; u += kNT) {
        const float4 v = reinterpret_cast<const float4*>(yr)[u];
        const uint4 key = make_uint4(enc_key(v.x - c), enc_key(v.y - c), enc_key(v.z - c), enc_key(v.w - c));
        tl(key.x); tl(key.y); tl(key.z); tl(key.w);
        reinterpret_cast<uint4*>(kw)[u] = key;
      }
      for (int t = 4 * nq + tid; t < TP; t += kNT) {
        const unsigned key = t < T ? enc_key(yr[t] - c) : kMissing;
        tl(key);
        kw[t] = key;
      }
    } else {
      for (int t = tid; t < TP; t += kNT) kw[t] = kMissing;
    }
    n[q] = uniform(block_sum<kNT>(tl.n, s.sc.redi));          // (barriers: keys, bins and z visible)
    fit[q] = act[q] = n[q] >= 2 * p;                          // (p >= 1: an empty row is not fitted)
    ks[q] = inf;                                              // the first pass is least squares
    sg[q] = 0.f;
  }

  const int i = lane & 31, h = lane >> 5;
  const float* xr = XT + (int64_t)i * ld_x;
  for (int pass = 0; pass <= iters; ++pass) {
    bool any = false;
#pragma unroll
    for (int q = 0; q < ROWS; ++q) any |= act[q];
    if (!any) break;

    // ---- gram: G += (w x) x^T over this wave's chunks, g += (w x) r
    f32x16 acc[ROWS];
    float gl[ROWS];
#pragma unroll
    for (int q = 0; q < ROWS; ++q) {
      acc[q] = f32x16{};
      gl[q] = 0.f;
    }
    for (int t0 = 64 * wv; t0 < T; t0 += 64 * kWaves) {
      const int tb = t0 + 32 * h;
      float xv[32];
      if (tb + 32 <= T) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const float4 b = *reinterpret_cast<const float4*>(xr + tb + 4 * u);
          xv[4 * u + 0] = b.x; xv[4 * u + 1] = b.y; xv[4 * u + 2] = b.z; xv[4 * u + 3] = b.w;
        }
      } else {
#pragma unroll
        for (int u = 0; u < 32; ++u) xv[u] = tb + u < T ? xr[tb + u] : 0.f;   // (the keys there are missing)
      }
#pragma unroll
      for (int q = 0; q < ROWS; ++q) {
        if (!act[q]) continue;
        const uint4* k4 = reinterpret_cast<const uint4*>(keys + q * TP + tb);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const uint4 kq = k4[u];
          const unsigned ke[4] = {kq.x, kq.y, kq.z, kq.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float r;
            const float x = xv[4 * u + e];
            const float wx = huber_weight(ke[e], ks[q], r) * x;
            acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(wx, x, acc[q], 0, 0, 0);
            gl[q] = fmaf(wx, r, gl[q]);
          }
        }
      }
    }
    // C/D map: col = lane & 31, row = (e & 3) + 8 * (e >> 2) + 4 * h
#pragma unroll
    for (int q = 0; q < ROWS; ++q) {
      if (!act[q]) continue;
#pragma unroll
      for (int e = 0; e < 16; ++e) s.tile[q][wv][((e & 3) + 8 * (e >> 2) + 4 * h) * kF + i] = acc[q][e];
      const float g = gl[q] + xor_lane<32>(gl[q]);
      if (h == 0) s.gpart[q][wv][i] = g;
    }
    __syncthreads();

    // ---- reduce: the waves' tiles summed and symmetrised
#pragma unroll
    for (int q = 0; q < ROWS; ++q) {
      if (!act[q]) continue;
      for (int e = tid; e < kF * kF; e += kNT) {
        const int et = (e & 31) * kF + (e >> 5);
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
          a += s.tile[q][w][e];
          b += s.tile[q][w][et];
        }
        s.G[q][e] = 0.5f * (a + b);
      }
    }
    __syncthreads();

    // ---- solve: wave q solves row q
#pragma unroll
    for (int q = 0; q < ROWS; ++q)
      if (wv == q && act[q]) solve_row(s.G[q], s.gpart[q], s.z[q], s.dz[q], p);
    __syncthreads();

    // ---- update: r -= U dz, the new keys tallied
    float dzr[ROWS][kF];
    RowTally tl[ROWS];
#pragma unroll
    for (int q = 0; q < ROWS; ++q)
#pragma unroll
      for (int f = 0; f < kF; ++f) dzr[q][f] = act[q] ? s.dz[q][f] : 0.f;
    for (int u = tid, nq = (T + 3) >> 2; u < nq; u += kNT) {
      float4 d[ROWS];
#pragma unroll
      for (int q = 0; q < ROWS; ++q) d[q] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int f = 0; f < kF; ++f) {
        const float4 x = *reinterpret_cast<const float4*>(XT + (int64_t)f * ld_x + 4 * u);
#pragma unroll
        for (int q = 0; q < ROWS; ++q) {
          d[q].x = fmaf(x.x, dzr[q][f], d[q].x);
          d[q].y = fmaf(x.y, dzr[q][f], d[q].y);
          d[q].z = fmaf(x.z, dzr[q][f], d[q].z);
          d[q].w = fmaf(x.w, dzr[q][f], d[q].w);
        }
      }
#pragma unroll
      for (int q = 0; q < ROWS; ++q) {
        if (!act[q]) continue;
        uint4* k4 = reinterpret_cast<uint4*>(keys + q * TP) + u;
        uint4 kq = *k4;
        kq.x = kq.x == kMissing ? kMissing : enc_key(dec_key(kq.x) - d[q].x);
        kq.y = kq.y == kMissing ? kMissing : enc_key(dec_key(kq.y) - d[q].y);
        kq.z = kq.z == kMissing ? kMissing : enc_key(dec_key(kq.z) - d[q].z);
        kq.w = kq.w == kMissing ? kMissing : enc_key(dec_key(kq.w) - d[q].w);
        tl[q](kq.x); tl[q](kq.y); tl[q](kq.z); tl[q](kq.w);
        *k4 = kq;
      }
    }

    // ---- scale: K13's sigma of the finite residuals
#pragma unroll
    for (int q = 0; q < ROWS; ++q) {
      if (!act[q]) continue;
      const int nr = uniform(block_sum<kNT>(tl[q].n, s.sc.redi));   // (barriers: the new keys visible)
      const KeyRange range = block_range(tl[q].range, &s.sc);
      float center, sig = 0.f;
      if (nr > 0) {
        LdsSpan<kNT> span{keys + q * TP, 0, T};
        median_sigma(span, (unsigned)nr, range, &s.sc, center, sig);
      }
      sg[q] = sig;
      if (sig > 0.f) {
        ks[q] = huber ? khub * sig : inf;
      } else {                                                // every residual alike: nothing set aside
        ks[q] = inf;
        act[q] = false;
      }
    }
  }

  // ---- outputs
#pragma unroll
  for (int q = 0; q < ROWS; ++q) {
    const int64_t row = row0 + q;
    if (row >= R) continue;                                   // (uniform over the workgroup)
    double ws = 0.0;
    if (fit[q]) {
      const uint4* k4 = reinterpret_cast<const uint4*>(keys + q * TP);
      for (int u = tid, nq = (T + 3) >> 2; u < nq; u += kNT) {
        const uint4 kq = k4[u];
        float r;
        ws += (double)huber_weight(kq.x, ks[q], r);
        ws += (double)huber_weight(kq.y, ks[q], r);
        ws += (double)huber_weight(kq.z, ks[q], r);
        ws += (double)huber_weight(kq.w, ks[q], r);
      }
      ws = block_sum<kNT>(ws, s.sc.redd);
    }
    if (tid < kF) Z[row * kF + tid] = fit[q] ? (float)s.z[q][tid] : 0.f;
    if (tid == 0) {
      shift[row] = c0[q];
      sigma[row] = fit[q] ? sg[q] : quiet_nan();
      nfin[row] = n[q];
      wsum[row] = (float)ws;
      fallback[row] = fit[q] ? 0 : 1;
    }
  }
}

template <int ROWS>
int launch(const float* Y, int64_t ld_y, int T, int64_t R, const float* XT, int64_t ld_x, int p, float k, int iters,
           float* Z, float* shift, float* sigma, int* nfin, float* wsum, int* fallback, hipStream_t stream) {
  const size_t lds = lds_bytes<ROWS>(T);
  if (lds > kCuLds) return (int)hipErrorInvalidValue;
  if (lds > 65536) {
    static bool done = false;            // once per instantiation (idempotent if raced)
    if (!done) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(lsq_robust_fit_kernel<ROWS>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCuLds);
      done = true;
    }
  }
  hipLaunchKernelGGL((lsq_robust_fit_kernel<ROWS>), dim3((unsigned)((R + ROWS - 1) / ROWS)), dim3(kNT), lds, stream, Y,
                     ld_y, T, R, XT, ld_x, p, k, iters, Z, shift, sigma, nfin, wsum, fallback);
  FM_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// 1 when fm_lsq_robust_fit takes histories of T samples: two one-row
// workgroups of that length share a CU's LDS.
FM_API int fm_lsq_robust_supported(int T) { return T >= 1 && lds_bytes<1>(T) <= kCuLds / 2; }

// Robust fit of every row of Y [R, >= T] on the basis XT [32][ld_x] (U^T, zero
// beyond column T and in the rows >= p, the kept rank): Huber threshold k
// sigmas (not finite or <= 0: least squares over the finite samples), one
// least-squares pass and `iters` reweighted ones.  Z [R, 32], shift, sigma,
// wsum [R] fp32, nfin, fallback [R] int32.  rows = 1 or 2 rows a workgroup, 0 =
// the default.  hipErrorInvalidValue, and nothing launched, for a misaligned Y
// or XT, a leading dimension that is no multiple of 4 or too short, T beyond
// fm_lsq_robust_supported, iters outside 0 ... 16 or p outside 1 ... 32.
FM_API int fm_lsq_robust_fit(const float* Y, int64_t ld_y, int T, int64_t R, const float* XT, int64_t ld_x, int p,
                             float k, int iters, int rows, float* Z, float* shift, float* sigma, int* nfin,
                             float* wsum, int* fallback, hipStream_t stream) {
  if ((ld_y & 3) || (ld_x & 3) || (((uintptr_t)Y) & 15) || (((uintptr_t)XT) & 15)) return (int)hipErrorInvalidValue;
  if (!fm_lsq_robust_supported(T) || ld_y < T || ld_x < ((T + 3) & ~3) || iters < 0 || iters > kMaxIters || p < 1 ||
      p > kF || rows < 0 || rows > 2 || R > 0x7FFFFFFF)
    return (int)hipErrorInvalidValue;
  if (R <= 0) return 0;
  if ((rows ? rows : kDefaultRows) == 2)
    return launch<2>(Y, ld_y, T, R, XT, ld_x, p, k, iters, Z, shift, sigma, nfin, wsum, fallback, stream);
  return launch<1>(Y, ld_y, T, R, XT, ld_x, p, k, iters, Z, shift, sigma, nfin, wsum, fallback, stream);
}
