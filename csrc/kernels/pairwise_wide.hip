// K21: the pairwise rank tests' sufficient statistics for a row whose pooled
// sample does not fit the registers of one wave (n_cur + n_base > 1024, up to
// kPairwiseWideMax).  One 256-thread workgroup per row, grid-stride over rows;
// the 14 numbers per row are exactly what pw_store_suff (fm_pairwise.h) writes
// and eval_test reads, so fm_pvalues / fm_pvalues_only finish the row.
//
// Tag-free counting form on two sorted sides.  The two samples go to LDS as
// order-preserving keys (enc_key: NaN / +-inf -> the missing key, which sorts
// last; -0.0 is made +0.0 first, so it ties with 0.0 as the float compare of
// the wave kernel has it; denormals stay distinct).  Each side is sorted on
// its own, and every count comes from binary searches: for a finite x with
// lt_s / le_s = #(side s < x) / #(side s <= x),
//   t       = (le_1 - lt_1) + (le_2 - lt_2)            size of x's tie run
//   2 rank  = 2 (lt_1 + lt_2) + t + 1
//   tie     = sum over samples of (t^2 - 1)            = sum over runs of t^3 - t
//   KS num. = max |le_1 n2 - le_2 n1|                  (equal inside a run)
// (the identities of pw_compute_count).  The Wilcoxon ranks are the same thing
// once more: the |d| of the positive pairs are side 1, of the negative pairs
// side 2, rplus is side 1's rank sum and the tie term the pooled one.  The
// pairs are read again from global memory, so their keys take over the LDS of
// the pooled phase: 2 min(n_cur, n_base) <= n_cur + n_base words.
//
// Sort: a bitonic network whose comparators all put the smaller key at the
// lower index (the first step of a merge pairs i with i ^ (size - 1), the
// rest i with i + stride).  With every comparator pointing the same way a
// virtual tail of maximal keys never moves, so a side of any length n sorts as
// the next power of two with the comparators that touch the tail left out: no
// padding to a power of two in LDS (8191 + 1 fits like 4096 + 4096).  A side
// is padded to whole chunks of 16 keys with the missing key; sizes up to 16
// and the strides 8..1 of every later merge run in the registers of the
// thread that holds the chunk, the other steps are four comparators per
// thread on uint4.
//
// Integers stay integers: counts and the KS numerator in 32 bits (<= 2^26),
// the doubled rank sums and the tie terms (<= n^3 - n = 5.5e11) in 64.  The
// Welch moments are fp64 sums of the fp32 samples.
#include "fm_radix_select.h"

using namespace fm;

namespace {

constexpr int kWideNT = 256;
constexpr int kPairwiseWideMax = 8192;      // mirrored as PAIRWISE_WIDE_MAX in foremast_amd/ops/canary.py
constexpr int kChunk = 16;                  // keys a thread sorts in registers
constexpr int kWideWords = kPairwiseWideMax + 2 * kChunk;   // both sides padded to whole chunks
constexpr int kWideSuff = 14;
constexpr int kWideWaves = kWideNT / FM_WAVE;

struct WideShared {
  alignas(16) unsigned keys[kWideWords];
  unsigned long long redu[3][kWideWaves];
  double redd[2][kWideWaves];
  int redi[kWideWaves];
};
// 32.3 KiB: within the plain launch limit, four workgroups per CU by LDS
static_assert(sizeof(WideShared) <= kLaunchLds && 4 * sizeof(WideShared) <= 160 * 1024, "LDS of a workgroup");

// One side in LDS: n16 words (a multiple of kChunk), P = the power of two the
// network is laid out for (>= n16; 0 for an empty side).
struct Side {
  unsigned* k;
  int n16;
  int P;
};

__device__ __forceinline__ int chunks_up(int n) { return (n + kChunk - 1) & ~(kChunk - 1); }
__device__ __forceinline__ int pow2_up(int n) { return n <= 0 ? 0 : (n <= 1 ? 1 : 1 << (32 - __clz(n - 1))); }

__device__ __forceinline__ void cx(unsigned& a, unsigned& b) {
  const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

// strides N/2 .. 1 of a merge over N keys in registers
template <int N>
__device__ __forceinline__ void merge_tail_regs(unsigned (&e)[N]) {
#pragma unroll
  for (int s = N >> 1; s > 0; s >>= 1)
#pragma unroll
    for (int i = 0; i < N; ++i)
      if ((i & s) == 0) cx(e[i], e[i + s]);
}
template <int N>
__device__ __forceinline__ void sort_regs(unsigned (&e)[N]) {
#pragma unroll
  for (int size = 2; size <= N; size <<= 1) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int j = i ^ (size - 1);
      if (j > i) cx(e[i], e[j]);
    }
#pragma unroll
    for (int s = size >> 2; s > 0; s >>= 1)
#pragma unroll
      for (int i = 0; i < N; ++i)
        if ((i & s) == 0) cx(e[i], e[i + s]);
  }
}

// every chunk of the side through f in registers
template <class F>
__device__ __forceinline__ void chunk_pass(Side s, F f) {
  uint4* k4 = reinterpret_cast<uint4*>(s.k);
  for (int q = threadIdx.x; q * kChunk < s.n16; q += kWideNT) {
    unsigned e[kChunk];
#pragma unroll
    for (int j = 0; j < kChunk / 4; ++j) {
      const uint4 v = k4[q * (kChunk / 4) + j];
      e[4 * j] = v.x; e[4 * j + 1] = v.y; e[4 * j + 2] = v.z; e[4 * j + 3] = v.w;
    }
    f(e);
#pragma unroll
    for (int j = 0; j < kChunk / 4; ++j)
      k4[q * (kChunk / 4) + j] = make_uint4(e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]);
  }
}

// first step of the merge of size 2^lsz >= 32: i with i ^ (size - 1).  Four
// comparators a thread: i0..i0+3 against jb+3..jb, both quads aligned.
__device__ __forceinline__ void flip_step(Side s, int lsz) {
  const int size = 1 << lsz;
  if (size > s.P) return;
  uint4* k4 = reinterpret_cast<uint4*>(s.k);
  const int half = size >> 1;
  for (int g = threadIdx.x; g < (s.P >> 3); g += kWideNT) {
    const int c = 4 * g, blk = c >> (lsz - 1), off = c & (half - 1);
    const int i0 = (blk << lsz) + off, jb = (blk << lsz) + size - 4 - off;
    if (i0 >= s.n16) break;
    if (jb >= s.n16) continue;               // the partners lie in the virtual tail
    uint4 a = k4[i0 >> 2], b = k4[jb >> 2];
    cx(a.x, b.w); cx(a.y, b.z); cx(a.z, b.y); cx(a.w, b.x);
    k4[i0 >> 2] = a;
    k4[jb >> 2] = b;
  }
}
// a later step of a merge: i with i + st, st >= kChunk
__device__ __forceinline__ void stride_step(Side s, int st) {
  uint4* k4 = reinterpret_cast<uint4*>(s.k);
  for (int g = threadIdx.x; g < (s.P >> 3); g += kWideNT) {
    const int c = 4 * g;
    const int i0 = 2 * c - (c & (st - 1)), j0 = i0 + st;
    if (i0 >= s.n16) break;
    if (j0 >= s.n16) continue;
    uint4 a = k4[i0 >> 2], b = k4[j0 >> 2];
    cx(a.x, b.x); cx(a.y, b.y); cx(a.z, b.z); cx(a.w, b.w);
    k4[i0 >> 2] = a;
    k4[j0 >> 2] = b;
  }
}

// Both sides sorted ascending in place, in the same steps (one barrier a
// step for the two).  Keys visible on entry; sorted and visible on return.
__device__ __forceinline__ void sort_sides(Side a, Side b) {
  chunk_pass(a, [](unsigned (&e)[kChunk]) { sort_regs(e); });
  chunk_pass(b, [](unsigned (&e)[kChunk]) { sort_regs(e); });
  __syncthreads();
  const int pmax = a.P > b.P ? a.P : b.P;
  for (int lsz = 5; (1 << lsz) <= pmax; ++lsz) {
    flip_step(a, lsz);
    flip_step(b, lsz);
    __syncthreads();
    for (int st = 1 << (lsz - 2); st >= kChunk; st >>= 1) {
      if ((1 << lsz) <= a.P) stride_step(a, st);
      if ((1 << lsz) <= b.P) stride_step(b, st);
      __syncthreads();
    }
    if ((1 << lsz) <= a.P) chunk_pass(a, [](unsigned (&e)[kChunk]) { merge_tail_regs(e); });
    if ((1 << lsz) <= b.P) chunk_pass(b, [](unsigned (&e)[kChunk]) { merge_tail_regs(e); });
    __syncthreads();
  }
}

// #(k[0..n) < x) and #(k[0..n) <= x) of a sorted run
__device__ __forceinline__ int count_lt(const unsigned* k, int n, unsigned x) {
  int lo = 0, len = n;
  while (len > 0) {
    const int half = len >> 1;
    const bool r = k[lo + half] < x;
    lo = r ? lo + half + 1 : lo;
    len = r ? len - half - 1 : half;
  }
  return lo;
}
__device__ __forceinline__ int count_le(const unsigned* k, int n, unsigned x) {
  int lo = 0, len = n;
  while (len > 0) {
    const int half = len >> 1;
    const bool r = k[lo + half] <= x;
    lo = r ? lo + half + 1 : lo;
    len = r ? len - half - 1 : half;
  }
  return lo;
}

// N sums over the workgroup behind one pair of barriers
template <int N, typename T>
__device__ __forceinline__ void block_sums(T (&v)[N], T (*scratch)[kWideWaves]) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const T w = wave_sum(v[j]);
    if (lane_id() == 0) scratch[j][wave_id()] = w;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < N; ++j) {
    T r = 0;
#pragma unroll
    for (int w = 0; w < kWideWaves; ++w) r += scratch[j][w];
    v[j] = r;
  }
  __syncthreads();
}

// The sorted sides a (n1 finite keys) and b (n2): doubled rank sum of side a,
// pooled tie term and the KS numerator, over the workgroup.
__device__ __forceinline__ void rank_sides(const unsigned* a, int n1, const unsigned* b, int n2, WideShared* sh,
                                           bool want_ks, unsigned long long& r1x2, unsigned long long& tie,
                                           int& dnum) {
  unsigned long long acc[2] = {0ull, 0ull};
  int dmax = 0;
  for (int e = threadIdx.x; e < n1 + n2; e += kWideNT) {
    const bool first = e < n1;
    const unsigned x = first ? a[e] : b[e - n1];
    const int lt1 = count_lt(a, n1, x), le1 = count_le(a, n1, x);
    const int lt2 = count_lt(b, n2, x), le2 = count_le(b, n2, x);
    const int t = (le1 - lt1) + (le2 - lt2);
    if (first) acc[0] += (unsigned long long)(2 * (lt1 + lt2) + t + 1);
    acc[1] += (unsigned long long)((long long)t * t - 1);
    const int dd = abs(le1 * n2 - le2 * n1);                 // <= 8192^2 / 4
    dmax = dd > dmax ? dd : dmax;
  }
  if (want_ks) dnum = (n1 > 0 && n2 > 0) ? block_max<kWideNT>(dmax, sh->redi) : 0;
  block_sums(acc, sh->redu);
  r1x2 = acc[0];
  tie = acc[1];
}

__device__ __forceinline__ unsigned sample_key(float x) { return enc_key(x == 0.f ? 0.f : x); }

__global__ __launch_bounds__(kWideNT) void pairwise_wide_kernel(
    const float* __restrict__ cur, int64_t ld_c, int n_cur, const float* __restrict__ base, int64_t ld_b,
    int n_base, int64_t R, double* __restrict__ suff) {
  __shared__ WideShared sh;
  const int tid = threadIdx.x;
  const int npair = n_cur < n_base ? n_cur : n_base;
  const Side sa{sh.keys, chunks_up(n_cur), pow2_up(chunks_up(n_cur))};
  const Side sb{sh.keys + sa.n16, chunks_up(n_base), pow2_up(chunks_up(n_base))};
  const Side wp{sh.keys, chunks_up(npair), pow2_up(chunks_up(npair))};
  const Side wn{sh.keys + wp.n16, wp.n16, wp.P};
  for (int64_t row = blockIdx.x; row < R; row += gridDim.x) {
    const float* c = cur + row * ld_c;
    const float* b = base + row * ld_b;
    // ---- pooled sample: keys, counts and fp64 sums
    unsigned long long cnt[3] = {0ull, 0ull, 0ull};
    double sum[2] = {0.0, 0.0};
    for (int i = tid; i < sa.n16; i += kWideNT) {
      const unsigned k = i < n_cur ? sample_key(c[i]) : kMissing;
      sa.k[i] = k;
      if (k != kMissing) { ++cnt[0]; sum[0] += (double)dec_key(k); }
    }
    for (int i = tid; i < sb.n16; i += kWideNT) {
      const unsigned k = i < n_base ? sample_key(b[i]) : kMissing;
      sb.k[i] = k;
      if (k != kMissing) { ++cnt[1]; sum[1] += (double)dec_key(k); }
    }
    block_sums(cnt, sh.redu);
    block_sums(sum, sh.redd);
    const int n1 = (int)cnt[0], n2 = (int)cnt[1];
    const double m1 = sum[0] / (double)(n1 > 0 ? n1 : 1), m2 = sum[1] / (double)(n2 > 0 ? n2 : 1);
    double q[2] = {0.0, 0.0};
    for (int i = tid; i < sa.n16; i += kWideNT) {
      const unsigned k = sa.k[i];
      if (k != kMissing) { const double d = (double)dec_key(k) - m1; q[0] += d * d; }
    }
    for (int i = tid; i < sb.n16; i += kWideNT) {
      const unsigned k = sb.k[i];
      if (k != kMissing) { const double d = (double)dec_key(k) - m2; q[1] += d * d; }
    }
    block_sums(q, sh.redd);
    sort_sides(sa, sb);
    unsigned long long r1x2, tie;
    int dnum = 0;
    rank_sides(sa.k, n1, sb.k, n2, &sh, true, r1x2, tie, dnum);

    // ---- Wilcoxon / Friedman: position pairs, |d| of the positive pairs on
    // one side and of the negative pairs on the other
    cnt[0] = cnt[1] = cnt[2] = 0ull;
    for (int j = tid; j < wp.n16; j += kWideNT) {
      unsigned kp = kMissing, kn = kMissing;
      if (j < npair) {
        const float xc = c[j], xb = b[j];
        const float d = xc - xb;
        if (isfinite(xc) && isfinite(xb)) {
          const unsigned mag = __float_as_uint(fabsf(d));    // a finite |d|, or +inf on overflow, orders as its bits
          if (d > 0.f) { kp = mag; ++cnt[0]; }
          else if (d < 0.f) { kn = mag; ++cnt[1]; }
          else ++cnt[2];
        }
      }
      wp.k[j] = kp;
      wn.k[j] = kn;
    }
    block_sums(cnt, sh.redu);
    const int npos = (int)cnt[0], nneg = (int)cnt[1], nzero = (int)cnt[2];
    sort_sides(wp, wn);
    unsigned long long rp2, tiew;
    int unused = 0;
    rank_sides(wp.k, npos, wn.k, nneg, &sh, false, rp2, tiew, unused);

    if (tid == 0) {
      double* o = suff + row * kWideSuff;
      o[0] = n1; o[1] = n2; o[2] = npos + nneg; o[3] = 0.5 * (double)r1x2; o[4] = (double)tie;
      o[5] = (n1 > 0 && n2 > 0) ? (double)dnum / ((double)n1 * n2) : 0.0;
      o[6] = 0.5 * (double)rp2; o[7] = (double)tiew; o[8] = m1; o[9] = m2; o[10] = q[0]; o[11] = q[1];
      o[12] = npos; o[13] = nzero;
    }
  }
}

}  // namespace

// suff [R, 14] fp64 of rows with n_cur + n_base <= kPairwiseWideMax columns
// (fm_pvalues / fm_pvalues_only turn them into p-values).
FM_API int fm_pairwise_suff_wide(const float* cur, int64_t ld_c, int n_cur, const float* base, int64_t ld_b,
                                 int n_base, int64_t R, double* suff, hipStream_t stream) {
  if (n_cur < 0 || n_base < 0 || (int64_t)n_cur + n_base > kPairwiseWideMax) return (int)hipErrorInvalidValue;
  if (R <= 0) return 0;
  constexpr int64_t kMaxBlocks = 4096;       // beyond what the CUs hold at once the rows are strided
  const dim3 grid((unsigned)(R < kMaxBlocks ? R : kMaxBlocks)), block(kWideNT);
  hipLaunchKernelGGL(pairwise_wide_kernel, grid, block, 0, stream, cur, ld_c, n_cur, base, ld_b, n_base, R, suff);
  FM_LAUNCH_CHECK();
  return 0;
}
