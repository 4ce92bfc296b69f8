// fm-hipcc-flags: -mllvm -pragma-unroll-threshold=1000000 -ffp-contract=off -Xclang -target-feature -Xclang -packed-fp32-ops
// (the unroll threshold keeps the 16 walkers of a thread in registers.
// Contraction is off for the reason given at the top of pairwise_effect.hip:
// the gate and the medians are separately rounded fp32 operations; for the
// same contract the device code uses no packed fp32 instructions.)
//
// K28: the effect size of current vs baseline (K19's outputs, bit for bit) for
// a row whose pooled sample is too wide for one wave: n_cur + n_base up to
// kPairwiseWideMax in any split.  One 256-thread workgroup per row,
// grid-stride over rows.
//
// Both sides go to LDS as order-preserving keys and are sorted each on its own
// by K21's network (fm_lds_sort.h); the finite samples are then the first n1 /
// n2 words, and the keys are decoded to floats in place.  Over the N = n1 n2
// pairs d = fl32(x - y), never materialised, K19's selection runs at
// workgroup scale.  fp32 round-to-nearest subtraction is monotone, so for a
// threshold t the pairs with d > t are a prefix of the sorted baseline for a
// fixed x and a suffix of the sorted current window for a fixed y.  The
// SHORTER side walks (at most 4096 = 16 x 256 samples: up to 16 per thread in
// registers, sample k * 256 + tid so that neighbouring lanes search
// neighbouring places), the longer one is searched in LDS; whichever walks,
// the difference is x - y in that operand order.  Each walker keeps the
// bracket [blo, bhi] of its boundary in the searched side over the key
// interval still in play (the boundary is monotone in t) and searches only
// inside it.  #{d <= t} is the workgroup's sum of the walkers' counts: an
// integer wave reduction, then the four waves through LDS behind ONE barrier
// (two sets of slots taken in turn: a wave that writes a set again has passed
// the barrier behind which every wave had read it).
//
// The Hodges-Lehmann shift is bisected MSB-first over the 32-bit key of d,
// the trial key decoded to a float once per step, stopping as soon as one pair
// is left in the interval; gt and lt are the counts at the keys of +0 and -0;
// the upper middle of an even N is the smallest key just outside the brackets
// (all of it K19's scheme, see pairwise_effect.hip).  N <= 4096^2 = 2^24: the
// counts fit int32, float(N) and float(gt - lt) are exact.
#include "fm_effect.h"
#include "fm_lds_sort.h"

using namespace fm;

namespace {

constexpr int kEffTests = 6;                                 // N_TESTS of fm_pairwise.h
constexpr int kWalk = kPairwiseWideMax / 2 / kWideNT;       // walkers of a thread
static_assert(kWalk * kWideNT * 2 == kPairwiseWideMax, "the shorter side fits the walkers");

struct EffectShared {
  alignas(16) unsigned keys[kWideWords];    // the sorted sides: keys, then the floats' bits
  unsigned red[2][kWideWaves];
};
// 32.2 KiB: within the plain launch limit, four workgroups per CU by LDS
static_assert(sizeof(EffectShared) <= kLaunchLds && 4 * sizeof(EffectShared) <= 160 * 1024, "LDS of a workgroup");

// An integer folded over the workgroup with an exact, commutative op, behind
// one barrier; the result is scalar.  par picks the slots and flips.
template <typename T, typename Op>
__device__ __forceinline__ T block_fold(T v, Op op, EffectShared* sh, int& par) {
  static_assert(sizeof(T) == 4, "32-bit");
  const T w = wave_reduce_uniform(v, op);
  if (lane_id() == 0) sh->red[par][wave_id()] = (unsigned)w;
  __syncthreads();
  T r = (T)sh->red[par][0];
#pragma unroll
  for (int i = 1; i < kWideWaves; ++i) r = op(r, (T)sh->red[par][i]);
  par ^= 1;
  return uniform(r);
}
__device__ __forceinline__ int block_count(int v, EffectShared* sh, int& par) {
  return block_fold(v, [](int a, int b) { return a + b; }, sh, par);
}
__device__ __forceinline__ unsigned block_min_key(unsigned v, EffectShared* sh, int& par) {
  return block_fold(v, [](unsigned a, unsigned b) { return a < b ? a : b; }, sh, par);
}

// d of a walker's sample w and a searched sample s.  CW: the current window
// walks and the baseline is searched; else the other way round.
template <bool CW>
__device__ __forceinline__ float pair_diff(float w, float s) { return CW ? w - s : s - w; }

// One counting step.  The boundary b[k] of walker k in the searched side
// s[0..ns) (floats' bits, ascending): CW, the length of the prefix with
// x - s[j] > t; else the length of the prefix with s[i] - y <= t.  Either way
// the words below b[k] are those where (d > t) == CW.  Searched inside the
// bracket br[k] = blo | bhi << 16 (both at most 8191; packed, the kernel
// stays within 128 registers and four workgroups share a CU); a walker without
// a sample carries an empty bracket that counts nothing.  Returns this
// thread's share of #{pairs with d <= t}.  The searches of a thread advance
// together, so their LDS reads overlap.
template <bool CW>
__device__ __forceinline__ int count_step(const float (&w)[kWalk], int nk, const unsigned* __restrict__ s, int ns,
                                          float t, const unsigned (&br)[kWalk], int (&b)[kWalk]) {
  int lo[kWalk], hi[kWalk];
#pragma unroll
  for (int k = 0; k < kWalk; ++k) { lo[k] = (int)(br[k] & 0xFFFFu); hi[k] = (int)(br[k] >> 16); }
  bool more;
  do {
    more = false;
#pragma unroll
    for (int k = 0; k < kWalk; ++k) {
      if (k < nk) {
        const bool act = lo[k] < hi[k];
        const int mid = act ? (lo[k] + hi[k]) >> 1 : 0;           // lo <= mid < hi <= ns: inside the searched side
        const bool g = (pair_diff<CW>(w[k], __uint_as_float(s[mid])) > t) == CW;
        lo[k] = act && g ? mid + 1 : lo[k];
        hi[k] = act && !g ? mid : hi[k];
        more |= lo[k] < hi[k];
      }
    }
  } while (more);
  int c = 0;
#pragma unroll
  for (int k = 0; k < kWalk; ++k) {
    b[k] = lo[k];
    if (k < nk) c += CW ? ns - lo[k] : lo[k];
  }
  return c;
}

// This thread's smallest key among the pairs just above the threshold the
// boundaries q belong to (the brackets' upper ends if high, else the lower):
// CW, the pair (x, s[q - 1]), the last of the prefix; else (s[q], y), the
// first of the suffix.  0xFFFFFFFF if there is none.
template <bool CW>
__device__ __forceinline__ unsigned min_key_at(const float (&w)[kWalk], int nk, int nw, const unsigned* __restrict__ s,
                                               int ns, const unsigned (&br)[kWalk], bool high) {
  unsigned m = 0xFFFFFFFFu;
#pragma unroll
  for (int k = 0; k < kWalk; ++k) {
    if (k < nk) {
      const int q = (int)(high ? br[k] >> 16 : br[k] & 0xFFFFu), j = CW ? q - 1 : q;
      const bool ok = k * kWideNT + (int)threadIdx.x < nw && j >= 0 && j < ns;
      const unsigned kk = eff_key(pair_diff<CW>(w[k], __uint_as_float(s[ok ? j : 0])));
      if (ok) m = kk < m ? kk : m;
    }
  }
  return m;
}

// gt, lt and the lower and upper middle keys of the N = nw ns > 0 pairs of
// the walking side wk[0..nw) and the searched side s[0..ns), both sorted
// floats' bits in LDS, visible on entry.
template <bool CW>
__device__ __forceinline__ void effect_pairs(const unsigned* __restrict__ wk, int nw, const unsigned* __restrict__ s,
                                             int ns, EffectShared* sh, int& par, int& gt, int& lt, unsigned& klo,
                                             unsigned& kup) {
  const int N = nw * ns, nk = (nw + kWideNT - 1) / kWideNT;
  float w[kWalk];
  // brackets of the boundaries, blo | bhi << 16: blo at the interval's end
  // with the smaller boundary, bhi at the other (CW: the prefix shrinks as t
  // grows, so blo belongs to the upper end; else to the lower end)
  unsigned br[kWalk];
  int b[kWalk];
#pragma unroll
  for (int k = 0; k < kWalk; ++k) {
    const int i = k * kWideNT + (int)threadIdx.x;
    const bool ok = i < nw;
    w[k] = ok ? __uint_as_float(wk[i]) : 0.f;
    br[k] = (unsigned)(ok || !CW ? 0 : ns) | (unsigned)(ok || CW ? ns : 0) << 16;
  }
  gt = N - block_count(count_step<CW>(w, nk, s, ns, 0.f, br, b), sh, par);      // #{d <= +0}
  // lower middle: the smallest key whose "<=" count reaches rank + 1.
  // Invariant: c_lo = #{key < pre} < need <= c_hi = #{key <= pre | rest}.
  const int need = ((N - 1) >> 1) + 1;
  unsigned pre = 0;
  int c_lo = 0, c_hi = N, bit = 31;
  // (the first step always runs: it is also the count of the negatives)
  for (; bit >= 0 && (bit == 31 || c_hi - c_lo > 1); --bit) {
    const unsigned trial = pre | ((1u << bit) - 1u);
    int cnt = 0;
    if (trial >= kKeyNegInf) {
      cnt = block_count(count_step<CW>(w, nk, s, ns, eff_threshold(trial), br, b), sh, par);
    } else {
#pragma unroll
      for (int k = 0; k < kWalk; ++k) b[k] = (int)(CW ? br[k] >> 16 : br[k] & 0xFFFFu);     // no d is <= trial
    }
    if (bit == 31) lt = cnt;                                           // trial == key(-0): #{d < 0}
    const bool upper = cnt >= need;
    if (upper) c_hi = cnt; else { c_lo = cnt; pre |= 1u << bit; }
#pragma unroll
    for (int k = 0; k < kWalk; ++k) {
      br[k] = upper == CW ? (br[k] & 0xFFFF0000u) | (unsigned)b[k] : (br[k] & 0xFFFFu) | (unsigned)b[k] << 16;
    }
  }
  // all bits decided: the interval is the key itself; stopped early: the one
  // pair left in it is the smallest above its lower end
  klo = bit < 0 ? pre : block_min_key(min_key_at<CW>(w, nk, nw, s, ns, br, CW), sh, par);
  // #{key <= klo} == c_hi either way; the upper middle is the next pair up
  kup = klo;
  if ((N & 1) == 0 && c_hi < need + 1) kup = block_min_key(min_key_at<CW>(w, nk, nw, s, ns, br, !CW), sh, par);
}

__global__ __launch_bounds__(kWideNT) void pairwise_effect_wide_kernel(
    const float* __restrict__ cur, int64_t ld_c, int n_cur, const float* __restrict__ base, int64_t ld_b, int n_base,
    int64_t R, float min_effect, float min_shift, float min_shift_abs, int directional,
    const int* __restrict__ bound, int M, const float* __restrict__ pvals_in, float* __restrict__ effect,
    int* __restrict__ counts, int8_t* __restrict__ passed, float* __restrict__ pvals_gated) {
  __shared__ EffectShared sh;
  const int tid = threadIdx.x;
  const Side sa{sh.keys, chunks_up(n_cur), pow2_up(chunks_up(n_cur))};
  const Side sb{sh.keys + sa.n16, chunks_up(n_base), pow2_up(chunks_up(n_base))};
  const float qnan = quiet_nan();
  int par = 0;
  for (int64_t row = blockIdx.x; row < R; row += gridDim.x) {
    const float* c = cur + row * ld_c;
    const float* b = base + row * ld_b;
    int fin1 = 0, fin2 = 0;
    for (int i = tid; i < sa.n16; i += kWideNT) {
      const unsigned k = i < n_cur ? sample_key(c[i]) : kMissing;
      sa.k[i] = k;
      fin1 += k != kMissing ? 1 : 0;
    }
    for (int i = tid; i < sb.n16; i += kWideNT) {
      const unsigned k = i < n_base ? sample_key(b[i]) : kMissing;
      sb.k[i] = k;
      fin2 += k != kMissing ? 1 : 0;
    }
    const int n1 = block_count(fin1, &sh, par), n2 = block_count(fin2, &sh, par);     // (barriers: keys visible)
    const int N = n1 * n2;
    int gt = 0, lt = 0;
    float delta = qnan, shift = qnan, bmed = qnan;
    if (N > 0) {
      sort_sides(sa, sb);
      for (int i = tid; i < sa.n16 + sb.n16; i += kWideNT) sh.keys[i] = __float_as_uint(dec_key(sh.keys[i]));
      __syncthreads();
      unsigned klo, kup;
      if (n1 <= n2) effect_pairs<true>(sa.k, n1, sb.k, n2, &sh, par, gt, lt, klo, kup);
      else effect_pairs<false>(sb.k, n2, sa.k, n1, &sh, par, gt, lt, klo, kup);
      delta = __fdiv_rn((float)(gt - lt), (float)N);
      shift = 0.5f * eff_val(klo) + 0.5f * eff_val(kup);
      bmed = 0.5f * __uint_as_float(sb.k[(n2 - 1) >> 1]) + 0.5f * __uint_as_float(sb.k[n2 >> 1]);
    }
    const bool pass = effect_passes(N, delta, shift, bmed, row, min_effect, min_shift, min_shift_abs, directional,
                                    bound, M);
    if (tid == 0) effect_store(row, delta, shift, bmed, N, gt, lt, pass, effect, counts, passed);
    if (pvals_in != nullptr && tid < kEffTests)
      pvals_gated[row * kEffTests + tid] = pass ? pvals_in[row * kEffTests + tid] : qnan;
    __syncthreads();                         // the sides are overwritten by the next row
  }
}

}  // namespace

// K19's outputs (fm_pairwise_effect, same parameters) for rows of up to
// kPairwiseWideMax pooled columns in any split.
FM_API int fm_pairwise_effect_wide(const float* cur, int64_t ld_c, int n_cur, const float* base, int64_t ld_b,
                                   int n_base, int64_t R, float min_effect, float min_shift, float min_shift_abs,
                                   int directional, const int* bound, int M, const float* pvals_in, float* effect,
                                   int* counts, int8_t* passed, float* pvals_gated, hipStream_t stream) {
  if (R <= 0) return 0;
  if (n_cur < 0 || n_base < 0 || (int64_t)n_cur + n_base > kPairwiseWideMax || M <= 0 ||
      (pvals_in != nullptr && pvals_gated == nullptr))
    return (int)hipErrorInvalidValue;
  constexpr int64_t kMaxBlocks = 4096;       // beyond what the CUs hold at once the rows are strided
  const dim3 grid((unsigned)(R < kMaxBlocks ? R : kMaxBlocks)), block(kWideNT);
  hipLaunchKernelGGL(pairwise_effect_wide_kernel, grid, block, 0, stream, cur, ld_c, n_cur, base, ld_b, n_base, R,
                     min_effect, min_shift, min_shift_abs, directional, bound, M, pvals_in, effect, counts, passed,
                     pvals_gated);
  FM_LAUNCH_CHECK();
  return 0;
}
