// K13 robust history statistics: per-row median and MAD (Hampel band) by an
// exact MSB-first radix selection, one 512-thread workgroup per row.
//
// The row is read from HBM once (16-B loads after a peeled head, so the row
// needs 4-byte alignment only) and kept in LDS as order-preserving uint32
// keys: negatives have all bits flipped, non-negatives get the sign bit set.
// NaN / +-inf become the key 0xFFFFFFFF, which no finite value maps to and
// which sorts above every finite key, so ranks below the finite count n
// never see it and the keys need no compaction.  The position of a key in
// LDS does not matter to a selection: the aligned body is stored first and
// the peeled head / tail elements behind it.
//
// The keys and the selection (MSB-first radix passes of up to 11 bits over
// 2,048 LDS bins) are fm_radix_select.h, shared with K14.  Phase two
// overwrites the keys with the bits of |x - centre| (non-negative floats are
// monotone as they are), sums them in fp64 and selects again.
//
// Rows longer than the LDS capacity run the same passes re-reading global
// memory (no limit on T; not a fast path).  The contract is
// foremast_amd/ops/misc.py ref_robust_stats; centre and MAD are exact.
#include "fm_common.h"
#include "fm_radix_select.h"

using namespace fm;

namespace {

constexpr int kRobustThreads = 512;

template <int NT, bool LDS>
__global__ __launch_bounds__(NT) void robust_stats_kernel(const float* __restrict__ hist, int64_t ld, int T, int64_t R,
                                                          float* __restrict__ out /*[R,3]*/) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_keys[];
  __shared__ __attribute__((aligned(16))) unsigned s_bins[kBins];
  __shared__ unsigned s_sel[3];
  __shared__ unsigned s_redu[NT / FM_WAVE];
  __shared__ int s_redi[NT / FM_WAVE];
  __shared__ double s_redd[NT / FM_WAVE];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float* p = hist + row * ld;
  RowKeys<NT, LDS> rk{p, T, s_keys, (T + 3) >> 2, false, 0.f};
  for (int i = tid; i < kBins; i += NT) s_bins[i] = 0u;

  // ---- the row -> keys; finite count and key range
  int n = 0;
  unsigned kmin = kMissing, kmax = 0u;
  auto track = [&](unsigned k) {
    if (k != kMissing) {
      ++n;
      kmin = k < kmin ? k : kmin;
      kmax = k > kmax ? k : kmax;
    }
  };
  if constexpr (LDS) {
    int head = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);   // elements before the 16-B boundary
    if (head > T) head = T;
    const int nb = (T - head) >> 2, edge = T - 4 * nb;                        // edge = head + tail elements, < 7
    const float4* b4 = reinterpret_cast<const float4*>(p + head);
    for (int q = tid; q < nb; q += NT) {
      const float4 x = b4[q];
      const uint4 k = make_uint4(enc_key(x.x), enc_key(x.y), enc_key(x.z), enc_key(x.w));
      track(k.x); track(k.y); track(k.z); track(k.w);
      s_keys[q] = k;
    }
    if (tid < 4 * (rk.nq - nb)) {                                             // head, tail, padding to whole quads
      unsigned k = kMissing;
      if (tid < edge) k = enc_key(p[tid < head ? tid : 4 * nb + tid]);
      track(k);
      reinterpret_cast<unsigned*>(s_keys)[4 * nb + tid] = k;
    }
  } else {
    rk.sweep(track);
  }
  n = block_sum<NT>(n, s_redi);                                               // (barriers: keys and bins visible)
  if (n == 0) {
    if (tid == 0) {
      out[row * 3 + 0] = __uint_as_float(0x7FC00000u);
      out[row * 3 + 1] = __uint_as_float(0x7FC00000u);
      out[row * 3 + 2] = 0.f;
    }
    return;
  }
  kmin = block_min_u32<NT>(kmin, s_redu);
  kmax = ~block_min_u32<NT>(~kmax, s_redu);

  // ---- median
  unsigned klo, kup;
  select_middles<NT, LDS>(rk, kmin, kmax, (unsigned)n, s_bins, s_sel, s_redu, klo, kup);
  const float center = 0.5f * dec_key(klo) + 0.5f * dec_key(kup);

  // ---- deviations: keys, fp64 sum, range
  double sum = 0.0;
  unsigned dmin = kMissing, dmax = 0u;
  auto track_dev = [&](unsigned d) {
    if (d != kMissing) {
      sum += (double)__uint_as_float(d);
      dmin = d < dmin ? d : dmin;
      dmax = d > dmax ? d : dmax;
    }
  };
  if constexpr (LDS) {
    for (int q = tid; q < rk.nq; q += NT) {
      const uint4 v = s_keys[q];
      const uint4 d = make_uint4(dev_key(v.x, center), dev_key(v.y, center), dev_key(v.z, center),
                                 dev_key(v.w, center));
      track_dev(d.x); track_dev(d.y); track_dev(d.z); track_dev(d.w);
      s_keys[q] = d;
    }
  } else {
    rk.dev = true;
    rk.c = center;
    rk.sweep(track_dev);
  }
  sum = block_sum<NT>(sum, s_redd);
  dmin = block_min_u32<NT>(dmin, s_redu);
  dmax = ~block_min_u32<NT>(~dmax, s_redu);

  // ---- MAD
  unsigned dlo, dup;
  select_middles<NT, LDS>(rk, dmin, dmax, (unsigned)n, s_bins, s_sel, s_redu, dlo, dup);
  const float mad = 0.5f * __uint_as_float(dlo) + 0.5f * __uint_as_float(dup);
  if (tid == 0) {
    out[row * 3 + 0] = center;
    out[row * 3 + 1] = mad > 0.f ? 1.4826f * mad : 1.2533f * (float)(sum / (double)n);
    out[row * 3 + 2] = (float)n;
  }
}

}  // namespace

// out [R,3] fp32 = (centre, sigma, finite count) of hist[r, :T]; hist and ld
// need 4-byte alignment only.  Rows up to kRobustLdsKeys samples are selected
// in LDS, longer ones from global memory; the choice is per launch.
FM_API int fm_robust_stats(const float* hist, int64_t ld, int T, int64_t R, float* out, hipStream_t stream) {
  if (R <= 0) return 0;
  if (T < 0 || R > 0x7FFFFFFF || (((uintptr_t)hist) & 3) != 0) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)R), block(kRobustThreads);
  if (T <= kRobustLdsKeys) {
    const size_t lds = (size_t)((T + 3) / 4) * sizeof(uint4);
    hipLaunchKernelGGL((robust_stats_kernel<kRobustThreads, true>), grid, block, lds, stream, hist, ld, T, R, out);
  } else {
    hipLaunchKernelGGL((robust_stats_kernel<kRobustThreads, false>), grid, block, 0, stream, hist, ld, T, R, out);
  }
  FM_LAUNCH_CHECK();
  return 0;
}
