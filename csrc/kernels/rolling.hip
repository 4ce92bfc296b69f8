// K1 rolling bands: per-time-point mean / population std of the finite samples
// in a trailing window of w points, for every row of a [R, T] fp32 batch
// (NaN = missing sample).  This is the [S*M, T] band output of SURVEY §2.4 K1
// (the dashboard's metric bands, foremast-dashboard/src/config/metrics.js:21-29,
// over the brain's moving_average window; deploy/foremast/3_brain/
// foremast-brain.yaml:24-25 names the algorithm).
//
// One 256-thread workgroup per row walks it in tiles of 2048 samples; thread
// i owns the 8 contiguous samples / outputs [8i, 8i + 8) of a tile (two 16-B
// loads, two 16-B stores per band).  Per tile: the shifted samples d = x - c
// (c = mean of the row's first tile, so squares do not swamp the variance;
// NaN kept for missing samples) go to an LDS ring of two tiles, a block scan
// gives each thread the tile-local exclusive prefix of (count, sum d, sum d^2)
// (sums fp64), and those 256 prefixes go to a second small ring.  A thread's
// first window sum is P(t0) - P(t0 - w): P(t0) is its own prefix, P(t0 - w)
// the owner segment's prefix plus up to 8 ring samples.  Its next 7 windows
// slide in registers (+ own sample, - the sample leaving the window).
// Because t0 is a multiple of 8, the offset (t0 - w) mod 8 = (-w) mod 8 is the
// same for every thread, so the leaving samples are a fixed rotation of two
// ring segments (a switch on a uniform value).  w <= 2048 keeps every window
// inside this tile and the previous one, bridged by the previous tile's
// totals, so prefixes stay tile-local.  LDS 26 KB: several workgroups per CU
// keep enough rows in flight (a first version held full fp64 prefix rings,
// 72 KB, two workgroups per CU: 2.45 TB/s).  HBM traffic: the row read once,
// the two bands written once.
//
// Numerics: d = x - c is the only fp32 rounding of the samples (c itself from
// fp64 sums).  Every sum of d and of d^2, the per-thread partials included,
// is fp64, d^2 being exact there; the mean is c + fl32(s / n) and the
// variance (n q - s^2) / n^2.  So mean and std are within 2^-24 max|x - c| of
// exact plus their own fp32 rounding, wherever c lies relative to the window
// (tests/test_series_edges.py states the bound).  What is left is the fp64
// rounding of the tile prefixes, 2^-53 of up to 2048 d^2: on a window of
// equal samples far from c it shows as a std of 5e-7 max|d| / sqrt(n) instead
// of 0.  Windows of w <= 16 are summed straight from the ring and do not
// carry it.
#include "fm_common.h"

using namespace fm;

namespace {

constexpr int kTile = 2048;           // samples per tile = 256 threads x 8
constexpr int kRing = 2 * kTile;      // sample ring: this tile + the previous one

struct Tri {
  float n;
  double s, q;
};

__device__ __forceinline__ Tri tri_add(Tri a, Tri b) { return Tri{a.n + b.n, a.s + b.s, a.q + b.q}; }

// inclusive block scan of one Tri per thread (256 threads); the last thread's
// result is the block total.  scratch: 4 Tri in LDS.
__device__ __forceinline__ Tri block_incl_scan(Tri v, Tri* scratch) {
  Tri w{wave_incl_sum(v.n), wave_incl_sum(v.s), wave_incl_sum(v.q)};
  const int wid = wave_id();
  if (lane_id() == 63) scratch[wid] = w;
  __syncthreads();
  Tri off{0.f, 0.0, 0.0};
  for (int i = 0; i < wid; ++i) off = tri_add(off, scratch[i]);
  __syncthreads();   // scratch is reused by the next tile
  return tri_add(w, off);
}

// contributions of one (shifted) sample that is ``in`` the sum: finite count
// and d (0 when missing; selected in fp32, then widened).  Callers square d in
// fp64, where the 48-bit product is exact: fl32(d^2) is off by 2^-24 d^2,
// which a one-sample window showed as a std of 2.4e-4 |d|.
__device__ __forceinline__ void contrib(float d, bool in, float& n, double& s) {
  const bool f = isfinite(d) && in;
  n = f ? 1.f : 0.f;
  s = (double)(f ? d : 0.f);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void rolling_stats_kernel(const float* __restrict__ x, int64_t ld_x, int T,
                                                            int w, int min_count, float* __restrict__ mean,
                                                            float* __restrict__ sd, int64_t ld_o) {
  __shared__ float4 ring4[kRing / 4];              // shifted samples (NaN = missing)
  __shared__ float exn[2 * 256];                    // per-thread exclusive prefixes, two tiles
  __shared__ double exs[2 * 256], exq[2 * 256];
  __shared__ Tri scratch[4];
  __shared__ Tri totals[2];                         // tile totals, by ring half (block-uniform: kept out of the VGPRs)
  __shared__ double red[4];
  const int64_t row = blockIdx.x;
  const float* __restrict__ xr = x + row * ld_x;
  float* __restrict__ mr = mean + row * ld_o;
  float* __restrict__ sr = sd + row * ld_o;
  const int tid = threadIdx.x;
  const float NaNf = __builtin_nanf("");
  const float* ring = reinterpret_cast<const float*>(ring4);
  auto load8 = [&](int tb, float (&v)[8]) {
    const int e0 = tb + 8 * tid;
    if (e0 + 8 <= T) {
      const float4 a = *reinterpret_cast<const float4*>(xr + e0);
      const float4 b = *reinterpret_cast<const float4*>(xr + e0 + 4);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = e0 + k < T ? xr[e0 + k] : NaNf;
    }
  };
  const int r = (-w) & 7;                     // (t0 - w) mod 8, the same for every thread
  const int segback = (w + r) >> 3;           // owner segment of t0 - w is (own segment) - segback
  const bool direct = segback <= 2;           // w <= 16: window 0 is summed from the ring samples
  float c = 0.f;
  float nx[8];
  load8(0, nx);
  for (int tb = 0, tile = 0; tb < T; tb += kTile, ++tile) {
    float d[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = nx[k];
    if (tb + kTile < T) load8(tb + kTile, nx);   // in flight while this tile is scanned and written
    if (tile == 0) {
      // summed in fp64, so that a constant row gets c = its value and d = 0 exactly
      double ls = 0.0;
      float lc = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (isfinite(d[k])) { ls += (double)d[k]; lc += 1.f; }
      const double s = block_sum<256>(ls, red);
      const double n = block_sum<256>((double)lc, red);
      c = n > 0 ? (float)(s / n) : 0.f;
    }
    float an = 0.f;
    double as = 0.0, aq = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      d[k] = d[k] - c;                        // NaN stays NaN
      float n;
      double s;
      contrib(d[k], true, n, s);
      an += n; as += s; aq = fma(s, s, aq);
    }
    const int half = tile & 1;
    ring4[half * (kTile / 4) + 2 * tid] = make_float4(d[0], d[1], d[2], d[3]);
    ring4[half * (kTile / 4) + 2 * tid + 1] = make_float4(d[4], d[5], d[6], d[7]);
    const Tri incl = block_incl_scan(Tri{an, as, aq}, scratch);
    if (tid == 255) totals[half] = incl;
    const float en = incl.n - an;
    const double es = incl.s - as, eq = incl.q - aq;
    exn[half * 256 + tid] = en;
    exs[half * 256 + tid] = es;
    exq[half * 256 + tid] = eq;
    __syncthreads();
    // P(t0 - w), relative to this tile's carry, and the 8 samples leaving
    // the 8 windows: positions g0 .. g0 + 7 (g0 = t0 - w)
    const int seg = (tb >> 3) + tid - segback;        // global owner segment of g0 (may be < 0)
    float lv[16];
    // window 0 less its own first sample: P(t0) - P(g0), or, for w <= 16, the
    // w - 1 samples before t0 themselves
    double wn = direct ? 0.0 : (double)en, ws = direct ? 0.0 : es, wq = direct ? 0.0 : eq;
    if (seg + 1 >= 0) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int sg = seg + h;
        float4 a = make_float4(NaNf, NaNf, NaNf, NaNf), b = a;
        if (sg >= 0) {
          const int rbase = ((sg >> 8) & 1) * (kTile / 4) + (sg & 255) * 2;
          a = ring4[rbase];
          b = ring4[rbase + 1];
        }
        lv[8 * h + 0] = a.x; lv[8 * h + 1] = a.y; lv[8 * h + 2] = a.z; lv[8 * h + 3] = a.w;
        lv[8 * h + 4] = b.x; lv[8 * h + 5] = b.y; lv[8 * h + 6] = b.z; lv[8 * h + 7] = b.w;
      }
      if (direct) {
        // lv[r + 1 .. 8 segback - 1], summed as they are and not as a
        // difference of two tile prefixes, which carries 2^-53 of a prefix of
        // up to 2048 d^2: under the square root that is 5e-7 max|d| on a
        // window of (nearly) equal samples, w = 1 included
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          float n;
          double s;
          contrib(lv[i], i > r && i < 8 * segback, n, s);
          wn += n; ws += s; wq = fma(s, s, wq);
        }
      } else if (seg >= 0) {
        const int eh = ((seg >> 8) & 1) * 256 + (seg & 255);
        double pn = exn[eh], ps = exs[eh], pq = exq[eh];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float n;
          double s;
          contrib(lv[i], i <= r, n, s);
          pn += n; ps += s; pq = fma(s, s, pq);
        }
        if ((seg >> 8) != tile) {
          const Tri pt = totals[half ^ 1];
          pn -= pt.n; ps -= pt.s; pq -= pt.q;
        }
        wn -= pn; ws -= ps; wq -= pq;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) lv[i] = NaNf;
    }
    // leaving sample of window k is lv[r + 1 + k] (k < 7 slides); rotate by the uniform r
    float out[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) out[k] = lv[k + 8];
    switch (r) {
#define FM_ROT(RR) case RR: _Pragma("unroll") for (int k = 0; k < 8; ++k) out[k] = lv[RR + 1 + k < 16 ? RR + 1 + k : 15]; break;
      FM_ROT(0) FM_ROT(1) FM_ROT(2) FM_ROT(3) FM_ROT(4) FM_ROT(5) FM_ROT(6) FM_ROT(7)
#undef FM_ROT
    }
    // window k = window k-1 + own d[k] - leaving out[k-1]
    float om[8], os[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float n;
      double s;
      contrib(d[k], true, n, s);
      wn += n; ws += s; wq = fma(s, s, wq);
      if (k > 0) {
        contrib(out[k - 1], true, n, s);
        wn -= n; ws -= s; wq = fma(-s, s, wq);
      }
      if (wn >= (double)min_count && wn > 0.5) {
        // 1 / wn: the 1-ulp fp32 reciprocal and one Newton step in fp64 (no
        // fp64 divide sequence per output).  The seed alone is not enough: m
        // is a mean about c, which may lie far from the window (a row that
        // starts with missing samples or changes level), and c + m would
        // carry 2^-23 |m|.
        const double i0 = (double)__builtin_amdgcn_rcpf((float)wn);
        const double inv = i0 * fma(-wn, i0, 2.0);
        const double m = ws * inv;
        om[k] = c + (float)m;
        // variance as (n q - s^2) / n^2, not q / n - m^2: either product
        // carries 2^-53 of itself and the reciprocal only scales the result,
        // whereas its error in m^2 alone, 2 eps m^2, comes out of the square
        // root as |m| sqrt(2 eps)
        os[k] = sqrtf((float)(fmax(fma(wn, wq, -(ws * ws)), 0.0) * (inv * inv)));
      } else {
        om[k] = NaNf;
        os[k] = NaNf;
      }
    }
    const int t0 = tb + 8 * tid;
    if (t0 + 8 <= T && (ld_o & 3) == 0) {
      *reinterpret_cast<float4*>(mr + t0) = make_float4(om[0], om[1], om[2], om[3]);
      *reinterpret_cast<float4*>(mr + t0 + 4) = make_float4(om[4], om[5], om[6], om[7]);
      *reinterpret_cast<float4*>(sr + t0) = make_float4(os[0], os[1], os[2], os[3]);
      *reinterpret_cast<float4*>(sr + t0 + 4) = make_float4(os[4], os[5], os[6], os[7]);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (t0 + k < T) { mr[t0 + k] = om[k]; sr[t0 + k] = os[k]; }
    }
    // the next tile overwrites the ring half this tile read as "previous"
    __syncthreads();
  }
}

}  // namespace

// x [R, ld_x] fp32 (16-B aligned rows), 1 <= w <= 2048; mean / sd [R, ld_o].
FM_API int fm_rolling_stats(const float* x, int64_t ld_x, int T, int64_t R, int w, int min_count, float* mean,
                            float* sd, int64_t ld_o, hipStream_t stream) {
  if (R <= 0 || T <= 0) return 0;
  if (w < 1 || w > kTile || (ld_x & 3) != 0 || (((uintptr_t)x) & 15) != 0 || ld_o < T || ld_x < T)
    return (int)hipErrorInvalidValue;
  if (R > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(rolling_stats_kernel, dim3((unsigned)R), dim3(256), 0, stream, x, ld_x, T, w, min_count, mean,
                     sd, ld_o);
  FM_LAUNCH_CHECK();
  return 0;
}
