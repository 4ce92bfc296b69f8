// fm-hipcc-flags: -mllvm -pragma-unroll-threshold=1000000 -ffp-contract=off
// K34 rolling robust bands: per-time-point median / MAD sigma / finite count
// of the trailing window of w points, for every row of a [R, T] fp32 batch
// (NaN, +-inf = missing sample).  The robust counterpart of K1 (rolling.hip):
// every output is K13's (center, sigma, n) of x[r, max(0, t-w+1) : t+1]
// (foremast_amd/ops/misc.py ref_rolling_robust_stats is the definition).
//
// A sliding order statistic: the window's sorted order is carried from t to
// t + 1, never rebuilt.  One wave owns a (row, chunk of kChunk outputs) pair
// and keeps the window as 64 K sorted keys in registers, K = 1, 2, 4, 8, 16
// chosen from w (w <= 64 K).  The keys are K13's order-preserving uint32 keys
// (fm_radix_select.h): a missing sample is the maximal key, and so is every
// slot the window does not fill, so the structure always holds exactly 64 K
// keys whose n smallest are the finite samples.  A partial window at the
// start of a row, a missing sample that arrives or leaves and a run of
// missing samples that empties the window are all the one step below.
//
// Layout: lane-major, sorted position p at register p % K of lane p / K, so a
// position's neighbours are the registers beside it, with one DPP wave shift
// per direction for the lane boundary.
//
// Slide (replace the leaving key a by the arriving key b; a, b wave-uniform):
//   b >= a: a position with a <= key <= b takes min(right neighbour, b)
//   b <  a: a position with b <  key <= a takes max(left neighbour, b)
// and every other position keeps its key: 6 VALU per register, no loop over
// the window, no search for where a sits or where b goes.  Ties need no care:
// equal keys are the same value, whichever of them "leaves".
//
// First window of a chunk: the w samples before it, loaded register-major,
// sorted by the pairwise kernels' bitonic network (fm_pairwise.h) and turned
// lane-major through the wave's LDS mirror.  The leaving and arriving keys of
// 64 slides are two coalesced loads (one sample per lane), handed out by
// v_readlane; the halo is read from global memory again (L2), not staged.
//
// Median and MAD read the sorted window at wave-uniform positions: for K = 1
// straight from the register (v_readlane), for K > 1 through an LDS mirror
// (position p at word p; a lane rewrites its K words only when one of them
// changed; reads are broadcasts).  With n known the two middles are two reads.
// MAD: e_p = fl(s_p - m) is non-decreasing in p, so the j-th smallest |e| is
//   min over L of max(-e[L], e[L + j])
// (the block of j + 1 consecutive samples nearest m), and since -e[L] falls
// and e[L + j] rises with L the minimum sits at the first L with
// e[L + j] >= -e[L]: a wave-uniform binary search, started from the previous
// point's answer, which a slide moves by a position or two (the bracket test
// is exact, so a bad guess costs steps, never the result).  For an even n the
// second middle's L is that one or the one before it: one more step.
// sigma = 1.4826 mad, or where more than half the window ties (mad == 0) the
// fallback 1.2533 mean|x - m|: a wave sum in fp64 over the registers.
//
// Outputs: lane i keeps the results of slide i of a 64-block; the wave stores
// three coalesced rows of 64 per block.
//
// LDS: the mirror only, 256 K bytes a wave (none at K = 1); 4 waves a workgroup.
#include "fm_pairwise.h"
#include "fm_radix_select.h"

namespace {

constexpr int kChunk = 512;                  // outputs per wave (foremast_amd/ops/misc.py ROLLING_ROBUST_CHUNK)
constexpr int kWaves = 4;                    // waves per workgroup
constexpr int kMaxWindow = 1024;             // 64 lanes x K <= 16 registers (ROLLING_ROBUST_MAX_WINDOW)
static_assert(kChunk % FM_WAVE == 0, "a chunk is whole 64-slide blocks");
static_assert(kWaves * kMaxWindow * sizeof(unsigned) == 16 * 1024, "LDS at K = 16: 16 KiB a workgroup");
static_assert(160 * 1024 / (kWaves * kMaxWindow * sizeof(unsigned)) >= 8,
              "8 workgroups (32 waves) fit a CU's 160 KiB even at K = 16: registers, not LDS, bound occupancy");

// a wave's own LDS writes, made visible to its own reads (and the other way round)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a predicate every lane agrees on, as a scalar: the branch on it is a scalar branch
__device__ __forceinline__ bool uniform_pred(bool p) { return uniform(p ? 1 : 0) != 0; }
__device__ __forceinline__ unsigned umin(unsigned a, unsigned b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }

// The sorted window of one wave: v in registers (lane-major), m its LDS mirror.
template <int K>
struct Window {
  unsigned v[K];
  unsigned* m;

  // position p's key, the same in every lane: a broadcast read of the mirror,
  // or for K = 1, where position p is lane p, v_readlane (no mirror at all)
  __device__ __forceinline__ unsigned key(int p) const {
    if constexpr (K == 1) return (unsigned)__builtin_amdgcn_readlane((int)v[0], p);
    else return uniform(m[p]);
  }
  // e_p = fl(s_p - c)
  __device__ __forceinline__ float dev(int p, float c) const { return dec_key(key(p)) - c; }

  __device__ __forceinline__ void store_mirror() {
    const int l = lane_id();
    if constexpr (K >= 4) {
#pragma unroll
      for (int q = 0; q < K / 4; ++q)
        reinterpret_cast<uint4*>(m)[l * (K / 4) + q] = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    } else if constexpr (K == 2) {
      reinterpret_cast<uint2*>(m)[l] = make_uint2(v[0], v[1]);
    } else {
      m[l] = v[0];
    }
  }

  // The w samples before t0 (indices t0 - w .. t0 - 1, missing below 0), sorted.
  __device__ __forceinline__ int init(const float* __restrict__ xr, int t0, int w) {
    const int l = lane_id();
    int n = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = k * 64 + l, idx = t0 - w + i;
      v[k] = (i < w && idx >= 0) ? enc_key(xr[idx]) : kMissing;
      n += __popcll(__ballot(v[k] != kMissing));
    }
    int unused[K];
    bitonic_sort<K, false, false>(v, unused);
    if constexpr (K == 1) return n;
    // register-major (position k * 64 + lane) -> lane-major, through the mirror
    wave_lds_sync();                           // the mirror's earlier readers are done
#pragma unroll
    for (int k = 0; k < K; ++k) m[k * 64 + l] = v[k];
    wave_lds_sync();
    if constexpr (K >= 4) {
#pragma unroll
      for (int q = 0; q < K / 4; ++q) {
        const uint4 u = reinterpret_cast<const uint4*>(m)[l * (K / 4) + q];
        v[4 * q] = u.x; v[4 * q + 1] = u.y; v[4 * q + 2] = u.z; v[4 * q + 3] = u.w;
      }
    } else if constexpr (K == 2) {
      const uint2 u = reinterpret_cast<const uint2*>(m)[l];
      v[0] = u.x; v[1] = u.y;
    }
    return n;
  }

  // One key a of the window replaced by b (both wave-uniform); the mirror follows.
  __device__ __forceinline__ void slide(unsigned a, unsigned b) {
    if (a == b) return;
    bool changed = false;
    if (b > a) {
      unsigned right = lane_next(v[0], kMissing);    // the next lane's smallest key
#pragma unroll
      for (int k = K - 1; k >= 0; --k) {
        const unsigned own = v[k];
        const unsigned nv = (own >= a && own <= b) ? umin(right, b) : own;
        changed |= nv != own;
        v[k] = nv;
        right = own;
      }
    } else {
      unsigned left = lane_prev(v[K - 1], 0u);        // the previous lane's largest key
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const unsigned own = v[k];
        const unsigned nv = (own > b && own <= a) ? umax(left, b) : own;
        changed |= nv != own;
        v[k] = nv;
        left = own;
      }
    }
    if constexpr (K > 1) {
      wave_lds_sync();
      if (changed) store_mirror();
      wave_lds_sync();
    }
  }

  // sum of |x - c| over the n finite samples (fp32 differences, summed in fp64)
  __device__ __forceinline__ double dev_sum(float c) const {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (v[k] != kMissing) s += (double)fabsf(dec_key(v[k]) - c);
    return uniform(wave_sum(s));
  }
};

// The j-th smallest (0-based) of |e_p| over the n sorted samples, with
// P(L) = e[L + j] >= -e[L] monotone over L in [0, n - j): returns the first L
// with P(L) (n - j when there is none).  [lo, hi] brackets the answer on
// entry: P is false below lo and true from hi on.  `guess` only orders the
// probes.
template <int K>
__device__ __forceinline__ int first_nearer(const Window<K>& win, float c, int j, int lo, int hi, int guess) {
  auto P = [&](int L) { return uniform_pred(win.dev(L + j, c) >= -win.dev(L, c)); };
  const int gl = guess - 2, gh = guess + 2;
  if (gl > lo && gl <= hi) {
    if (P(gl - 1)) hi = gl - 1; else lo = gl;
  }
  if (gh >= lo && gh < hi) {
    if (P(gh)) hi = gh; else lo = gh + 1;
  }
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (P(mid)) hi = mid; else lo = mid + 1;
  }
  return lo;
}
// the distance itself: the smaller of the two blocks that meet at L
template <int K>
__device__ __forceinline__ float nearer_value(const Window<K>& win, float c, int j, int L, int n) {
  float d = INFINITY;
  if (L < n - j) d = win.dev(L + j, c);                // P(L): the block's far end is its right one
  if (L > 0) d = fminf(d, -win.dev(L - 1, c));         // not P(L - 1): its left one
  return d;
}

template <int K>
__global__ __launch_bounds__(kWaves * FM_WAVE) void rolling_robust_kernel(
    const float* __restrict__ x, int64_t ld_x, int T, int64_t npairs, int nchunks, int w, int min_count,
    float* __restrict__ center, float* __restrict__ sigma, int* __restrict__ cnt, int64_t ld_o) {
  __shared__ alignas(16) unsigned mirror[kWaves][64 * K];
  const int64_t pair = (int64_t)blockIdx.x * kWaves + wave_id();
  if (pair >= npairs) return;                          // wave-uniform; the kernel has no block barrier
  const int64_t row = pair / nchunks;
  const int t0 = (int)(pair - row * nchunks) * kChunk;
  const float* __restrict__ xr = x + row * ld_x;
  float* __restrict__ cr = center + row * ld_o;
  float* __restrict__ sr = sigma + row * ld_o;
  int* __restrict__ nr = cnt + row * ld_o;
  const int l = lane_id();
  const int need = min_count > 1 ? min_count : 1;

  Window<K> win;
  win.m = mirror[wave_id()];
  int n = win.init(xr, t0, w);
  int guess = 0;

  for (int tb = t0; tb < t0 + kChunk && tb < T; tb += FM_WAVE) {
    // the keys leaving and arriving in the next 64 slides, one of each per lane
    const int ia = tb - w + l, ib = tb + l;
    const unsigned ka = (ia >= 0 && ia < T) ? enc_key(xr[ia]) : kMissing;
    const unsigned kb = ib < T ? enc_key(xr[ib]) : kMissing;
    const int steps = T - tb < FM_WAVE ? T - tb : FM_WAVE;
    float oc = quiet_nan(), os = quiet_nan();
    int on = 0;
    for (int i = 0; i < steps; ++i) {
      const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)ka, i);
      const unsigned b = (unsigned)__builtin_amdgcn_readlane((int)kb, i);
      win.slide(a, b);
      n += (b != kMissing ? 1 : 0) - (a != kMissing ? 1 : 0);
      float c = quiet_nan(), s = quiet_nan();
      if (n >= need) {
        const int j0 = (n - 1) >> 1, j1 = n >> 1;
        c = mid_value(win.key(j0), win.key(j1));
        const int L0 = first_nearer(win, c, j0, 0, n - j0, guess);
        float mad = nearer_value(win, c, j0, L0, n);
        if (j1 != j0) {
          const int L1 = first_nearer(win, c, j1, L0 > 0 ? L0 - 1 : 0, L0 < n - j1 ? L0 : n - j1, L0);
          mad = 0.5f * mad + 0.5f * nearer_value(win, c, j1, L1, n);
        } else {
          mad = 0.5f * mad + 0.5f * mad;
        }
        guess = L0;
        s = uniform_pred(mad > 0.f) ? 1.4826f * mad : 1.2533f * (float)(win.dev_sum(c) / (double)n);
      }
      if (l == i) { oc = c; os = s; on = n; }
    }
    if (l < steps) {
      cr[tb + l] = oc;
      sr[tb + l] = os;
      nr[tb + l] = on;
    }
  }
}

template <int K>
int launch(const float* x, int64_t ld_x, int T, int64_t R, int w, int min_count, float* center, float* sigma,
           int* cnt, int64_t ld_o, hipStream_t stream) {
  const int nchunks = (T + kChunk - 1) / kChunk;
  const int64_t npairs = R * nchunks, blocks = (npairs + kWaves - 1) / kWaves;
  if (blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(rolling_robust_kernel<K>, dim3((unsigned)blocks), dim3(kWaves * FM_WAVE), 0, stream, x, ld_x, T,
                     npairs, nchunks, w, min_count, center, sigma, cnt, ld_o);
  FM_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// x [R, ld_x] fp32 (4-byte aligned rows, unit column stride), 1 <= w <= 1024;
// center / sigma fp32 and cnt int32, each [R, ld_o].
FM_API int fm_rolling_robust_stats(const float* x, int64_t ld_x, int T, int64_t R, int w, int min_count, float* center,
                                   float* sigma, int* cnt, int64_t ld_o, hipStream_t stream) {
  if (R < 0 || T < 1 || T > 0x7fffffff - kChunk - kMaxWindow || w < 1 || w > kMaxWindow || ld_o < T || ld_x < T || (((uintptr_t)x) & 3) != 0 || !x ||
      !center || !sigma || !cnt || R > 0x7fffffffLL)
    return (int)hipErrorInvalidValue;
  if (R == 0) return 0;
  if (w <= 64) return launch<1>(x, ld_x, T, R, w, min_count, center, sigma, cnt, ld_o, stream);
  if (w <= 128) return launch<2>(x, ld_x, T, R, w, min_count, center, sigma, cnt, ld_o, stream);
  if (w <= 256) return launch<4>(x, ld_x, T, R, w, min_count, center, sigma, cnt, ld_o, stream);
  if (w <= 512) return launch<8>(x, ld_x, T, R, w, min_count, center, sigma, cnt, ld_o, stream);
  return launch<16>(x, ld_x, T, R, w, min_count, center, sigma, cnt, ld_o, stream);
}
