// fm-hipcc-flags: -mllvm -pragma-unroll-threshold=1000000 -ffp-contract=off -Xclang -target-feature -Xclang -packed-fp32-ops
// (pairwise_drift.hip's line, for the same reason: the fp64 sums are defined
// op by op as the numpy reference evaluates them, and the device code uses no
// packed fp32 instructions.  The unroll threshold is pairwise_pods.hip's: the
// K = 16 bitonic network must unroll fully to stay in registers.)
//
// K32: the tail canary test (docs/BRAIN_SPEC.md 4.6): per level q, the share
// of each side's samples beyond the pooled q-quantile, judged by the exact
// conditional (Fisher / Mood) test, Bonferroni over the levels that count.
// The contract is foremast_amd/ops/reference.py pairwise_tail / tail_verdict.
//
// Per row, NaN / +-inf missing, n_c and n_b the finite counts, N their sum.
// A slot is (side, level), slot = side * L + level, side 0 the upper tail and
// side 1 the lower one.  For the upper side k = min(N - 1, ceil(q N / 10000)),
// t the k-th smallest pooled value, a / b the current / baseline samples above
// t and m = a + b; the lower side is the upper side of the negated samples: t
// the k-th largest value, a / b the samples below it.  Both tiers only produce
// these integers and t per slot (TailLevels, in LDS); tail_finish does the rest.
//
// Wave tier (n_cur + n_base <= 1024): one wave per row, four rows per
// workgroup.  The pooled row is sorted once in registers with the side as the
// tag (bitonic_sort<K, TAGGED>, fm_pairwise.h); slot i = 64 k + lane then
// holds the i-th smallest value, the pads (+inf) behind the N real ones.  A
// threshold is a lane read of the sorted image; the end of the tie run that
// holds it is the popcount of the ballots of `v <= t` (upper) or `v < t`
// (lower: the same sorted row read from the other end, never negated or
// sorted again), and the current side's share is the popcount of those
// ballots under the ballots of the tag, taken once per row.
//
// Workgroup tier (<= kPairwiseWideMax): one 256-thread workgroup per row, no
// sort.  The pooled keys (fm_radix_select.h, -0.0 folded into 0.0 so that the
// two tie) go to LDS once, the side of a key being its column; the ranks of
// all slots are selected in ONE radix_select_ranks, whose first pass is
// shared; its cnt / resid give the run of every threshold and so every m with
// no further pass; one sweep over the current side's keys counts, per thread
// and against all thresholds at once, the samples beyond each, and the
// per-thread counts are reduced over the workgroup into TailLevels.
//
// tail_finish (both tiers, one whole wave): the counting levels (m >=
// min_tail, m unlike the previous counting level's of its side), J, then all
// hypergeometric tails together: the (slot, x) terms of all counting levels
// are dealt to the 64 lanes, a term being exp of nine entries of the
// log-factorial table lf[n] = lgamma(n + 1), n = 0 .. 8192, which the host
// builds and hands over (read through L2: the nine reads of a term scatter
// over the table, docs/PERF.md K32); wave_sum per slot; then the deciding
// level, the verdict and every store.
//
// Whatever the inputs hold, a rank lies in [1, N - 1], a table index is
// clamped to [0, 8192], a slot to [0, 2 L), and a column is read only below
// the row's width: no input makes an access leave its array.
#include "fm_pairwise.h"
#include "fm_radix_select.h"
#include "fm_segments.h"

namespace {

constexpr int kTailWaveMax = 1024;           // pooled columns, wave tier (PAIRWISE_MAX in ops/canary.py)
constexpr int kTailLevels = 4;               // levels per row, at most (TAIL_MAX_LEVELS in ops/canary.py)
constexpr int kTailSlots = 2 * kTailLevels;
constexpr int kTailTableMax = 8192;          // lf[0 .. 8192] (TAIL_TABLE_MAX in ops/reference.py)
constexpr int kTailNT = 256;                 // threads of a wide-tier workgroup
static_assert(kTailTableMax >= kPairwiseWideMax, "the table covers every N a row can have");

struct TailCfg {
  int L;
  int q[kTailLevels];                        // levels in parts per 10,000, increasing
  int need, min_tail;
  float p_thr, min_excess;
  int sides;                                 // 0: the row's bound code; 1 upper, 2 lower, 3 both
  const int* __restrict__ bound;             // [M], read when sides == 0
  int M;
  const double* __restrict__ lf;             // [kTailTableMax + 1]
};

struct TailOut {
  float* __restrict__ tail;                  // [R, 4]
  int* __restrict__ which;                   // [R]
  int* __restrict__ J;                       // [R]
  int* __restrict__ n;                       // [R, 2]
  int* __restrict__ counts;                  // [R, 2, L, 3]
  int8_t* __restrict__ tail_diff;            // [R]
};

// One row's integers per slot, in LDS
struct TailLevels {
  int a[kTailSlots];                         // current samples beyond t
  int m[kTailSlots];                         // pooled samples beyond t
  int k[kTailSlots];
  float t[kTailSlots];
};

// the bound code of a row: 1 = the upper side alone, 2 = the lower side alone, anything else both
__device__ __forceinline__ int tail_code(const TailCfg& cfg, int64_t row) {
  return cfg.sides != 0 ? cfg.sides : cfg.bound[row % cfg.M];
}
__device__ __forceinline__ bool side_runs(int code, int side) { return side == 0 ? code != 2 : code != 1; }

// k = min(N - 1, ceil(q N / 10000)), held to [1, N - 1] (N >= 2; q N < 2^27)
__device__ __forceinline__ int tail_rank(int q, int N) {
  int k = (q * N + 9999) / 10000;
  k = k < N - 1 ? k : N - 1;
  return k > 1 ? k : 1;
}

// Entry i (wave-uniform) of the sorted register image: slot 64 k + lane
template <int K>
__device__ __forceinline__ float sorted_at(const float (&v)[K], int i) {
  i = i < 0 ? 0 : (i > 64 * K - 1 ? 64 * K - 1 : i);
  float r = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float t = lane_bcast(v[k], i & 63);
    r = (i >> 6) == k ? t : r;
  }
  return r;
}

// The finishing pass of a row, run by one whole wave once lv is complete and
// visible.  n_c, n_b, applies and code are wave-uniform.
__device__ __forceinline__ void tail_finish(const TailLevels* lv, int n_c, int n_b, bool applies, int code,
                                            const TailCfg& cfg, int64_t row, const TailOut& out) {
  const int lane = lane_id();
  const int L = cfg.L, N = n_c + n_b;
  const double* __restrict__ lf = cfg.lf;
  auto table = [&](int i) { return lf[i < 0 ? 0 : (i > kTailTableMax ? kTailTableMax : i)]; };
  // ---- the levels that count, and the terms x = a .. min(m, n_c) of each (none where the sum is 1 exactly)
  int off[kTailSlots + 1];
  unsigned counting = 0u, summed = 0u;
  int J = 0, prev = -1;
  off[0] = 0;
#pragma unroll
  for (int j = 0; j < kTailSlots; ++j) {
    int terms = 0;
    if (j < 2 * L) {
      if (j == L) prev = -1;
      const int a = uniform(lv->a[j]), m = uniform(lv->m[j]);
      if (applies && side_runs(code, j >= L ? 1 : 0) && m >= cfg.min_tail && m != prev) {
        prev = m;
        ++J;
        counting |= 1u << j;
        const int floor_x = m - n_b > 0 ? m - n_b : 0;
        const int top = m < n_c ? m : n_c;
        if (a > floor_x && top >= a) {
          terms = top - a + 1;
          summed |= 1u << j;
        }
      }
    }
    off[j + 1] = off[j] + terms;
  }
  // ---- all terms of all levels over the 64 lanes
  double acc[kTailSlots];
#pragma unroll
  for (int j = 0; j < kTailSlots; ++j) acc[j] = 0.0;
  const int total = off[kTailSlots];
  if (total > 0) {
    const double lfN = table(N), lfc = table(n_c), lfb = table(n_b);
    for (int idx = lane; idx < total; idx += FM_WAVE) {
      int j = 0, first = 0;
#pragma unroll
      for (int jj = 1; jj < kTailSlots; ++jj) {
        const bool in = idx >= off[jj];
        j += in ? 1 : 0;
        first = in ? off[jj] : first;
      }
      const int m = lv->m[j], x = lv->a[j] + (idx - first);
      double s = table(m) - table(x);
      s -= table(m - x);
      s += table(N - m);
      s -= table(n_c - x);
      s -= table(N - m - n_c + x);
      s -= lfN;
      s += lfc;
      s += lfb;
      const double term = exp(s);
#pragma unroll
      for (int jj = 0; jj < kTailSlots; ++jj) acc[jj] += j == jj ? term : 0.0;
    }
  }
  // ---- the deciding level: the smallest p, the lower slot on ties
  double pmin = 2.0;
  int best = -1;
#pragma unroll
  for (int j = 0; j < kTailSlots; ++j) {
    if (counting >> j & 1u) {
      double p = 1.0;
      if (summed >> j & 1u) {
        p = wave_sum(acc[j]);
        p = p > 1.0 ? 1.0 : p;
      }
      if (p < pmin) {
        pmin = p;
        best = j;
      }
    }
  }
  if (lane < 2 * L) {
    const bool runs = applies && side_runs(code, lane >= L ? 1 : 0);
    int* o = out.counts + (row * 2 * L + lane) * 3;
    const int a = lv->a[lane], m = lv->m[lane];
    o[0] = runs ? a : 0;
    o[1] = runs ? m - a : 0;
    o[2] = runs ? lv->k[lane] : 0;
  }
  if (lane == 0) {
    const double NaN = __builtin_nan("");
    double p = NaN, pm = NaN, ex = NaN;
    float t = __builtin_nanf("");
    if (best >= 0) {
      const int a = lv->a[best], b = lv->m[best] - a;
      pm = pmin;
      p = (double)J * pmin;
      p = p > 1.0 ? 1.0 : p;
      ex = (double)a / (double)n_c - (double)b / (double)n_b;
      t = lv->t[best];
    }
    const float pf = (float)p, ef = (float)ex;
    float* o = out.tail + row * 4;
    o[0] = pf; o[1] = (float)pm; o[2] = ef; o[3] = t;
    out.which[row] = best;
    out.J[row] = J;
    out.n[row * 2] = n_c;
    out.n[row * 2 + 1] = n_b;
    out.tail_diff[row] = (best >= 0 && pf < cfg.p_thr && ef >= cfg.min_excess) ? 1 : 0;
  }
}

struct TailWideShared {
  alignas(16) unsigned keys[kPairwiseWideMax];
  SelectScratch<kTailNT> sc;
  unsigned sel[3 * kTailSlots];
  TailLevels lv;
};
// 40.4 KiB: within the plain launch limit, three workgroups per CU by LDS
static_assert(sizeof(TailWideShared) <= kLaunchLds && 3 * sizeof(TailWideShared) <= 160 * 1024, "LDS of a workgroup");

// key of a sample with -0.0 as 0.0: equal floats have equal keys
__device__ __forceinline__ unsigned tail_key(float x) {
  const unsigned b = __float_as_uint(x);
  return enc_key(__uint_as_float(b == 0x80000000u ? 0u : b));
}

// The slots of the S sides that run (S == 1: the side `one`), all ranks in one
// selection, then the current side's counts by one sweep.  Every thread of the
// workgroup calls it; lv->a is zero on entry; no barrier after the last add.
template <int L, int S>
__device__ __forceinline__ void wide_levels(TailWideShared* sh, int nq, KeyRange range, int n_cur, int N, int one,
                                            const TailCfg& cfg) {
  constexpr int NR = L * S;
  const int tid = threadIdx.x;
  unsigned rank[NR], key[NR], resid[NR], cnt[NR];
  int k[NR];
  bool low[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    low[j] = S == 2 ? j >= L : one != 0;
    k[j] = tail_rank(cfg.q[j % L], N);
    rank[j] = (unsigned)(low[j] ? N - k[j] : k[j] - 1);
  }
  const LdsRow<kTailNT> rk{reinterpret_cast<uint4*>(sh->keys), nq};
  radix_select_ranks<kTailNT, NR>(rk, range, rank, (unsigned)N, &sh->sc, sh->sel, key, resid, cnt);
  int a[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) a[j] = 0;
  const uint4* k4 = reinterpret_cast<const uint4*>(sh->keys);
  for (int q = tid; 4 * q < n_cur; q += kTailNT) {
    const uint4 v = k4[q];
    const unsigned e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned x = 4 * q + u < n_cur ? e[u] : kMissing;   // (the quad the two sides share)
#pragma unroll
      for (int j = 0; j < NR; ++j) a[j] += (low[j] ? x < key[j] : (x > key[j] && x != kMissing)) ? 1 : 0;
    }
  }
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int slot = (low[j] ? L : 0) + j % L;
    const int s = (int)wave_sum_uniform((unsigned)a[j]);
    if (lane_id() == 0 && s != 0) atomicAdd(&sh->lv.a[slot], s);
    if (tid == 0) {
      const int below = (int)(rank[j] - resid[j]);             // pooled keys below t
      sh->lv.m[slot] = low[j] ? below : N - below - (int)cnt[j];
      sh->lv.k[slot] = k[j];
      sh->lv.t[slot] = dec_key(key[j]);
    }
  }
}

}  // namespace

template <int K>
__global__ __launch_bounds__(256) void tail_wave_kernel(const float* __restrict__ cur, int64_t ld_c, int n_cur,
                                                        const float* __restrict__ base, int64_t ld_b, int n_base,
                                                        int64_t R, TailCfg cfg, TailOut out) {
  __shared__ TailLevels s_lv[4];
  TailLevels* lv = &s_lv[wave_id()];
  const int lane = lane_id();
  const int n_pooled = n_cur + n_base;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave_id(); row < R; row += (int64_t)gridDim.x * 4) {
    const float* c = cur + row * ld_c;
    const float* b = base + row * ld_b;
    float v[K];
    int tag[K];
    unsigned long long is_cur[K];
    int n_c = 0, n_b = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = k * 64 + lane;
      float x = i < n_cur ? c[i] : (i < n_pooled ? b[i - n_cur] : kPad);
      int t = i < n_cur ? 0 : (i < n_pooled ? 1 : -1);
      if (!isfinite(x)) { x = kPad; t = -1; }
      v[k] = x; tag[k] = t;
      n_c += __popcll(__ballot(t == 0));
      n_b += __popcll(__ballot(t == 1));
    }
    const int N = n_c + n_b;
    const bool applies = n_c >= cfg.need && n_b >= cfg.need;
    const int code = uniform(tail_code(cfg, row));
    if (applies) {
      bitonic_sort<K, false, true>(v, tag);
#pragma unroll
      for (int k = 0; k < K; ++k) is_cur[k] = __ballot(tag[k] == 0);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (!side_runs(code, s)) continue;
#pragma unroll
        for (int l = 0; l < kTailLevels; ++l) {
          if (l < cfg.L) {
            const int kq = tail_rank(cfg.q[l], N);
            const float t = sorted_at<K>(v, s == 0 ? kq - 1 : N - kq);
            // the run of t ends where `v <= t` does (upper), starts where `v < t` ends (lower); pads compare false
            int side = 0, mine = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
              const unsigned long long in = __ballot(s == 0 ? v[k] <= t : v[k] < t);
              side += __popcll(in);
              mine += __popcll(in & is_cur[k]);
            }
            if (lane == 0) {
              const int slot = s * cfg.L + l;
              lv->a[slot] = s == 0 ? n_c - mine : mine;
              lv->m[slot] = s == 0 ? N - side : side;
              lv->k[slot] = kq;
              lv->t[slot] = t;
            }
          }
        }
      }
    }
    wave_lds_sync();
    tail_finish(lv, n_c, n_b, applies, code, cfg, row, out);
    wave_lds_sync();                                          // lv is reused by the next row
  }
}

template <int L>
__global__ __launch_bounds__(kTailNT) void tail_wide_kernel(const float* __restrict__ cur, int64_t ld_c, int n_cur,
                                                            const float* __restrict__ base, int64_t ld_b, int n_base,
                                                            int64_t R, TailCfg cfg, TailOut out) {
  __shared__ TailWideShared sh;
  const int tid = threadIdx.x;
  const int n_pooled = n_cur + n_base;
  const int nq = (n_pooled + 3) >> 2;
  sh.sc.clear_bins();
  for (int64_t row = blockIdx.x; row < R; row += gridDim.x) {
    const float* c = cur + row * ld_c;
    const float* b = base + row * ld_b;
    // ---- the keys, once; the finite counts of both sides packed into one sum
    int packed = 0;
    KeyRange mine;
    for (int i = tid; i < 4 * nq; i += kTailNT) {
      unsigned key = kMissing;
      if (i < n_pooled) {
        key = tail_key(i < n_cur ? c[i] : b[i - n_cur]);
        if (key != kMissing) {
          packed += i < n_cur ? 1 : 1 << 16;
          mine.add(key);
        }
      }
      sh.keys[i] = key;
    }
    if (tid < kTailSlots) sh.lv.a[tid] = 0;
    packed = uniform(block_sum<kTailNT>(packed, sh.sc.redi));   // (barriers: keys, bins and lv.a visible)
    const int n_c = packed & 0xFFFF, n_b = packed >> 16;
    const bool applies = n_c >= cfg.need && n_b >= cfg.need;
    const int code = uniform(tail_code(cfg, row));
    if (applies) {
      const KeyRange range = block_range(mine, &sh.sc);
      if (code == 1 || code == 2) wide_levels<L, 1>(&sh, nq, range, n_cur, n_c + n_b, code == 2, cfg);
      else wide_levels<L, 2>(&sh, nq, range, n_cur, n_c + n_b, 0, cfg);
    }
    __syncthreads();
    if (tid < FM_WAVE) tail_finish(&sh.lv, n_c, n_b, applies, code, cfg, row, out);
    __syncthreads();                                          // the keys and lv are reused by the next row
  }
}

// Per row: tail [R, 4] fp32 = (p, p_min, excess, t of the deciding level),
// which [R] int32 = side * L + level of the deciding level or -1, J [R] int32,
// n [R, 2] int32, counts [R, 2, L, 3] int32 = (a, b, k), tail_diff [R] int8;
// every output of every row is written (NaN / -1 / 0 where the test does not
// apply).  q0 .. q3: the L levels in parts per 10,000, increasing.  sides 0:
// bound [M] int32 gives row r the code bound[r % M] (1 upper, 2 lower, else
// both); 1 / 2 / 3: upper / lower / both for every row.  lf [8193] fp64 =
// lgamma(n + 1).  tier 0: the wave tier up to 1024 pooled columns, else the
// wide tier; tier 2: the wide tier.  n_cur + n_base <= 8192.
FM_API int fm_pairwise_tail(const float* cur, int64_t ld_c, int n_cur, const float* base, int64_t ld_b, int n_base,
                            int64_t R, int L, int q0, int q1, int q2, int q3, int sides, const int* bound, int M,
                            int min_points, int min_tail, float p_thr, float min_excess, const double* lf, int tier,
                            float* tail, int* which, int* J, int* n, int* counts, int8_t* tail_diff,
                            hipStream_t stream) {
  const int q[kTailLevels] = {q0, q1, q2, q3};
  if (n_cur < 0 || n_base < 0 || R < 0 || L < 1 || L > kTailLevels || (int64_t)n_cur + n_base > kPairwiseWideMax ||
      (tier != 0 && tier != 2) || sides < 0 || sides > 3 || (sides == 0 && (bound == nullptr || M < 1)))
    return (int)hipErrorInvalidValue;
  for (int l = 0; l < L; ++l)
    if (q[l] < 1 || q[l] > 9999 || (l > 0 && q[l] <= q[l - 1])) return (int)hipErrorInvalidValue;
  if (lf == nullptr || tail == nullptr || which == nullptr || J == nullptr || n == nullptr || counts == nullptr ||
      tail_diff == nullptr)
    return (int)hipErrorInvalidValue;
  if (R == 0) return 0;
  TailCfg cfg;
  cfg.L = L;
  for (int l = 0; l < kTailLevels; ++l) cfg.q[l] = l < L ? q[l] : 9999;
  cfg.need = min_points > 1 ? min_points : 1;
  cfg.min_tail = min_tail > 1 ? min_tail : 1;
  cfg.p_thr = p_thr;
  cfg.min_excess = min_excess;
  cfg.sides = sides;
  cfg.bound = bound;
  cfg.M = M > 1 ? M : 1;
  cfg.lf = lf;
  const TailOut out{tail, which, J, n, counts, tail_diff};
  const int np = n_cur + n_base;
#define FM_TAIL(KERNEL, KK, GRID, NT)                                                                                \
  hipLaunchKernelGGL(KERNEL<KK>, GRID, dim3(NT), 0, stream, cur, ld_c, n_cur, base, ld_b, n_base, R, cfg, out)
  if (tier == 0 && np <= kTailWaveMax) {
    const dim3 grid((unsigned)((R + 3) / 4 < 0x7FFFFFFF ? (R + 3) / 4 : 0x7FFFFFFF));
    if (np <= 64) FM_TAIL(tail_wave_kernel, 1, grid, 256);
    else if (np <= 128) FM_TAIL(tail_wave_kernel, 2, grid, 256);
    else if (np <= 256) FM_TAIL(tail_wave_kernel, 4, grid, 256);
    else if (np <= 512) FM_TAIL(tail_wave_kernel, 8, grid, 256);
    else FM_TAIL(tail_wave_kernel, 16, grid, 256);
  } else {
    constexpr int64_t kMaxBlocks = 4096;     // beyond what the CUs hold at once the rows are strided
    const dim3 grid((unsigned)(R < kMaxBlocks ? R : kMaxBlocks));
    if (L == 1) FM_TAIL(tail_wide_kernel, 1, grid, kTailNT);
    else if (L == 2) FM_TAIL(tail_wide_kernel, 2, grid, kTailNT);
    else if (L == 3) FM_TAIL(tail_wide_kernel, 3, grid, kTailNT);
    else FM_TAIL(tail_wide_kernel, 4, grid, kTailNT);
  }
#undef FM_TAIL
  FM_LAUNCH_CHECK();
  return 0;
}
