// Pairwise rank tests (K4), the device code shared by every canary-scoring
// unit that runs them: pairwise.hip (stand-alone kernels), canary_rows.hip
// (fused row kernel) and tick_front.hip (role-split front kernel).
// pw_compute with K = 16 needs the per-file flag
// `-mllvm -pragma-unroll-threshold=1000000` (see pairwise.hip).
//
// Reference behaviour being rebuilt (foremast-brain is external; see
// docs/BRAIN_SPEC.md): per (service, metric) the brain fits a historical model
// (ML_ALGORITHM=moving_average_all, deploy/foremast/3_brain/foremast-brain.yaml:24-25),
// compares canary vs baseline with pairwise tests (foremast-brain/README.md:32-38,
// docs/guides/design.md:35) and flags current points outside the bounds
// (design.md:43, fail fast).
//
// Layout: rows = services x metrics, row r -> metric r % M.  history [R, ld_h]
// fp32 (NaN = missing sample), current [R, ld_c], baseline [R, ld_b].
#pragma once
#include "fm_common.h"

using namespace fm;

// ---------------------------------------------------------------------------
// K4: pairwise tests. One wave per (service, metric) row, 4 rows per 256-thread
// workgroup.  The pooled sample (n1 + n2 <= 64*K) is sorted in registers with a
// bitonic network (in-register swaps for strides >= 64, __shfl_xor below),
// average ranks with ties come from a max-scan / suffix-min-scan over tie runs
// (a sorted array without ties skips them: the run-free path of avg_ranks).
// The front kernels with a baseline cache leave the last merge of the split
// layout out for a row without ties: each current value is searched in the
// sorted baseline instead (pw_rank_search).
// ---------------------------------------------------------------------------
namespace {

constexpr float kPad = INFINITY;

// SPLIT (K == 2 only): register 0 holds sample 1 and register 1 sample 2
// (each <= 64 values).  Every stage up to size 64 then stays inside one
// register, so a value's sample is its register index and the tags need no
// exchange; they are rebuilt (k, or -1 for pads) before the final 128-merge.
// That drops the tag exchange and select from 21 of the 27 lane-exchange
// steps.
// TAGGED = false sorts bare keys (the Wilcoxon sort: the sign rides in bit 0
// of an unsigned key, see pw_compute) and never touches `tag`.
//
// LO, HI: only the stages of sizes LO .. HI of the network run (powers of
// two; the whole sort is 2 .. 64 K).  REGS (HI <= 64 only, where no stage
// crosses registers): bit k set = register k takes part.  The split layout
// with a baseline cache (pw_compute) sorts register 0 alone up to size 64,
// takes register 1 as it stood at that point from the cache, and then runs
// the 128-merge by itself.
template <int K, bool SPLIT = false, bool TAGGED = true, int LO = 2, int HI = 64 * K, unsigned REGS = ~0u, typename T>
__device__ __forceinline__ void bitonic_sort(T (&v)[K], int (&tag)[K]) {
  // Branch-free compare-exchange (selects, no exec-mask branches): strides
  // >= 64 swap registers inside the lane, smaller strides exchange with the
  // partner lane through DPP / permlane (cmpx_lane_any).
  static_assert(!SPLIT || (K == 2 && TAGGED), "split layout is two tagged 64-lane registers");
  static_assert(REGS == ~0u || HI <= 64, "a register subset only while no stage crosses registers");
  const int lane = lane_id();
#pragma unroll
  for (int size = LO; size <= HI; size <<= 1) {
    const bool tags = TAGGED && (!SPLIT || size > 64);
    if constexpr (SPLIT) {
      if (size == 128) {
#pragma unroll
        for (int k = 0; k < K; ++k) tag[k] = v[k] == kPad ? -1 : k;
      }
    }
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (stride >= 64) {
        const int ks = stride / 64;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int p = k ^ ks;
          if (p > k) {
            const int i = k * 64 + lane;
            const bool asc = (i & size) == 0;
            const T a = v[k], b = v[p];
            // the smaller value goes to register k of an ascending pair
            const bool first = (a < b) == asc;
            v[k] = first ? a : b; v[p] = first ? b : a;
            if (tags) {
              const int ta = tag[k], tb = tag[p];
              tag[k] = first ? ta : tb; tag[p] = first ? tb : ta;
            }
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int i = k * 64 + lane;
          const bool asc = (i & size) == 0;
          const bool lower = (lane & stride) == 0;
          // keep the smaller value in the lower lane of an ascending pair
          const bool keep_min = lower == asc;
          if (REGS != ~0u && ((REGS >> k) & 1u) == 0u) {
          } else if (tags) {
            cmpx_lane_any(v[k], tag[k], stride, keep_min);
          } else {
            cmpx_lane_any(v[k], stride, keep_min);
          }
        }
      }
    }
  }
}

// Average (1-based) ranks for a sorted register array whose first n entries are
// real.  The return value is this lane's share of the tie term sum(t^3 - t)
// over tie runs (the caller reduces it, packed with its other integer sums);
// is_end marks the last element of each run (where empirical CDFs are
// evaluated).
//
// Run-free path: when no two neighbours among the n real entries are equal
// (decided for the whole wave by ballot, so the branch is scalar), every tie
// run has length 1: rank2 = 2 i + 2, is_end = i < n and the tie term is 0,
// and none of the scans below runs.  A sorted array takes this path if and
// only if its tie term is 0.  Equality is T's own == (float: -0.0 ties +0.0),
// the comparison the tied path uses for its run starts, and the tied path
// reuses the neighbour compare made here.
// REDUCE: the return value is the wave-uniform tie term itself, reduced inside
// the tied path (for a caller that has nothing to pack it with: the run-free
// path then pays no reduction for a sum known to be 0).
template <int K, bool REDUCE, typename T>
__device__ __forceinline__ int avg_ranks(const T (&v)[K], int n, int (&rank2)[K], bool (&is_end)[K]) {
  // rank2 = 2 x (1-based average rank) = start + end + 2: exact integers, so
  // rank sums and the tie term sum(t^3 - t) (<= 1024^3 < 2^31) need no doubles.
  const int lane = lane_id();
  bool ne_prev[K];   // v[i] != v[i - 1] (lane 0 of register 0: against the edge value, unused)
  unsigned long long tied = 0;
  T last_prev = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const T prev = lane_prev(v[k], last_prev);
    ne_prev[k] = v[k] != prev;
    // 0 < i < n as a scalar lane mask: pads (+inf) sit at i >= n and equal each
    // other, and lane 0 of register 0 has no left neighbour
    const int nk = n - 64 * k;
    const unsigned long long real = nk >= 64 ? ~0ull : (nk > 0 ? (1ull << nk) - 1ull : 0ull);
    tied |= __ballot(v[k] == prev) & (k == 0 ? real & ~1ull : real);
    if (k + 1 < K) last_prev = lane_bcast(v[k], 63);
  }
  if (tied == 0) {
    // Everything here is a function of the lane id and n alone.  It is formed
    // from an opaque copy of the lane id: as loop invariants the compiler would
    // hoist the K rank constants (and the i of i < n) out of the caller's row
    // loop and hold that many more registers through both sorts.  One add per
    // register either way: hoisted, this arm is K copies.
    int lo = lane;
    asm volatile("" : "+v"(lo));
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = k * 64 + lo;
      rank2[k] = 2 * i + 2;
      is_end[k] = i < n;
    }
    return 0;
  }
  int start_idx[K];
  int carry = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int i = k * 64 + lane;
    const bool st = (i == 0) || ne_prev[k];
    int s = st ? i : 0;
    s = wave_incl_max(s, 0);
    s = s > carry ? s : carry;
    start_idx[k] = s;
    carry = lane_bcast(s, 63);
  }
  int carry_e = 0x7fffffff;
  T next_first = 0;
  int tl = 0;
#pragma unroll
  for (int k = K - 1; k >= 0; --k) {
    const int i = k * 64 + lane;
    const T next = lane_next(v[k], next_first);
    const bool en = (i < n) && ((i == n - 1) || (v[k] != next));
    int e = en ? i : 0x7fffffff;
    e = wave_incl_suffix_min(e, 0x7fffffff);
    e = e < carry_e ? e : carry_e;
    carry_e = lane_bcast(e, 0);
    next_first = lane_bcast(v[k], 0);
    is_end[k] = en;
    rank2[k] = start_idx[k] + e + 2;
    if (i < n && i == start_idx[k]) {
      // t <= 1024: t^2 - 1 and t both fit the full-rate 24-bit multiplier
      const int t = e - start_idx[k] + 1;
      tl += __mul24(__mul24(t, t) - 1, t);
    }
  }
  if constexpr (REDUCE) tl = (int)wave_sum_uniform((unsigned)tl);
  return tl;
}

// Bits needed for an integer sum whose total is at most `bound`.
constexpr int pw_bits(long long bound) { return bound <= 0 ? 0 : 1 + pw_bits(bound >> 1); }

}  // namespace

enum { T_MW = 0, T_WIL = 1, T_KRU = 2, T_KS = 3, T_T = 4, T_FRI = 5, N_TESTS = 6 };
constexpr int kSuff = 14;

// Per-row pairwise inputs, split into a LOAD half (raw samples into
// registers, no arithmetic that would wait on them) and a COMPUTE half, so a
// fused kernel can put other loads in flight between the two.
template <int K>
struct PwIn {
  static constexpr int KW = (K + 1) / 2;
  float v[K];     // pooled sample slot i = k*64 + lane: cur[i] (i < n_cur) or base[i - n_cur]
  float pc[KW];   // position-paired cur[j], base[j] (Wilcoxon / Friedman)
  float pb[KW];
};

// SPLIT (K == 2, n_cur <= 64, n_base <= 64): v[0] = current, v[1] = baseline
// instead of the pooled order (see bitonic_sort).
template <int K, bool SPLIT = false>
__device__ __forceinline__ void pw_load(const float* __restrict__ c, const float* __restrict__ b, int n_cur,
                                        int n_base, PwIn<K>& in) {
  const int lane = lane_id();
  if constexpr (SPLIT) {
    in.v[0] = lane < n_cur ? c[lane] : kPad;
    in.v[1] = lane < n_base ? b[lane] : kPad;
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = k * 64 + lane;
      in.v[k] = i < n_cur ? c[i] : (i < n_cur + n_base ? b[i - n_cur] : kPad);
    }
  }
  const int npair = n_cur < n_base ? n_cur : n_base;
#pragma unroll
  for (int k = 0; k < PwIn<K>::KW; ++k) {
    const int j = k * 64 + lane;
    in.pc[k] = j < npair ? c[j] : 0.f;
    in.pb[k] = j < npair ? b[j] : 0.f;
  }
}

// Hook of pw_compute for a caller with work of its own to place inside the
// row (tick_front.hip requests its next row index): loaded() runs once every
// loaded sample has been consumed into registers (no load outstanding, the
// sorts still ahead), done() after the last reduction, before the row's
// stores.  store() is the row's sink: it gets the 14 statistics as they stand
// after the reductions (wave-uniform integers and floats) and decides where
// they go.  The default does nothing in loaded() / done() and has lane 0
// convert them to the doubles of `o` (pw_store_suff).
__device__ __forceinline__ void pw_store_suff(double* __restrict__ o, int n1, int n2, int nw, unsigned r1s,
                                              unsigned tie, int dnum, unsigned rps, unsigned tiew, float m1, float m2,
                                              float q1, float q2, int npos, int nzero) {
  o[0] = n1; o[1] = n2; o[2] = nw; o[3] = 0.5 * (double)r1s; o[4] = (double)tie;
  o[5] = (n1 > 0 && n2 > 0) ? (double)dnum / ((double)n1 * n2) : 0.0;
  o[6] = 0.5 * (double)rps; o[7] = (double)tiew; o[8] = m1; o[9] = m2; o[10] = q1; o[11] = q2;
  o[12] = npos; o[13] = nzero;
}

struct PwNoHook {
  __device__ __forceinline__ void loaded() const {}
  __device__ __forceinline__ void done() const {}
  __device__ __forceinline__ void store(double* __restrict__ o, int n1, int n2, int nw, unsigned r1s, unsigned tie,
                                        int dnum, unsigned rps, unsigned tiew, float m1, float m2, float q1, float q2,
                                        int npos, int nzero) const {
    if (lane_id() == 0) pw_store_suff(o, n1, n2, nw, r1s, tie, dnum, rps, tiew, m1, m2, q1, q2, npos, nzero);
  }
};

// Baseline cache of the split layout (tick_front.hip).  A canary job's
// baseline window is a fixed past interval: tick after tick a row brings the
// same n_base numbers, and everything pw_compute derives from them alone is
// the same too -- register 1 as it enters the 128-merge (finite-checked and
// through the stages up to size 64), the count n2 and the Welch moments m2,
// q2.  One entry per row keeps exactly those words, next to a bit copy of
// the baseline they were computed from:
//   raw[64]     b[lane] as loaded, lanes < n_base
//   sorted[64]  register 1 right before the size-128 stage, that lane order, pads included
//   stats       n2, bits(m2), bits(q2), n_base (0: empty entry)
// The row is a hit if and only if stats.w == n_base and the 32-bit patterns
// of all n_base raw lanes equal the loaded baseline's (a NaN equals itself,
// -0.0 against +0.0 is a miss): decided on the device, per row, wave-uniform.
// A hit takes register 1 and the three statistics from the entry and sorts
// register 0 alone; the state entering the merge (or, with SEARCH, the rank
// search that stands in for it: pw_rank_search) is bit for bit the miss
// path's, so every output word is.  A miss computes as without a cache and
// writes the entry (plain vector stores; a row belongs to one wave per
// launch, and launches that share a cache run one at a time).
// load() is called between pw_load and pw_compute, so the entry's loads are
// in flight with the row's; `sorted` is issued ahead of `stats`, whose wait
// (the hit test, ahead of hook.loaded()) therefore covers it.
struct PwNoBase {
  static constexpr bool kOn = false;
};
struct PwBaseCache {
  static constexpr bool kOn = true;
  // the three arrays and this row's entry in them; 32-bit indices (the host
  // keeps 64 rows < 2^32), so one lane offset serves raw and sorted
  unsigned* __restrict__ raw;
  unsigned* __restrict__ sorted;
  uint4* __restrict__ stats;
  unsigned row;
  unsigned r = 0, s = 0;
  uint4 st = {0u, 0u, 0u, 0u};
  __device__ __forceinline__ unsigned at() const { return row * 64u + (unsigned)lane_id(); }
  __device__ __forceinline__ void load(int n_base) {
    r = lane_id() < n_base ? raw[at()] : 0u;
    s = sorted[at()];
    st = stats[row];
  }
  __device__ __forceinline__ bool hit(float b, int n_base) const {
    const bool differs = (lane_id() < n_base && __float_as_uint(b) != r) || st.w != (unsigned)n_base;
    return __ballot(differs) == 0ull;
  }
};

// Search form of the pooled ranks (split layout with a baseline cache,
// SEARCH = true).  When the size-64 stages are done both registers are sorted:
// x = register 0 holds the n1 finite current values ascending (pads behind
// them), b = register 1 the n2 finite baseline values descending (pads in
// front).  Nothing a row outputs needs the two interleaved; it needs the
// doubled rank sum of the current sample, the pooled tie term and the KS
// numerator, and without a tie in the pooled sample all three follow from
//   c_i = #{finite baseline y : y < x_i},   c_-1 = 0
// of the current lanes i < n1 alone:
//   tie  = 0
//   r1x2 = sum_i 2 (i + c_i) + 2            (the doubled pooled rank of x_i)
//   dnum = max_i of |(i + 1) n2 - c_i n1|                          (at x_i)
//                   |i n2 - c_i n1|, |i n2 - (c_(i-1) + 1) n1|     (c_i > c_(i-1) only)
//                   |n1 n2 - (c_i + 1) n1|                         (i = n1 - 1 and c_i < n2 only)
// |F1 - F2| is linear in the baseline count between two current points, so
// over the baseline points of a gap it peaks at the gap's first or last one:
// the second line; the third is the gap above the largest current value.
// (docs/PERF.md, "Rank search"; tests/test_rank_search.py checks both
// identities, and the shorter form of the maximum computed below, against
// the pooled order.)  n1 and n2 are wave-uniform.
// c_i comes from a branch-free binary search, seven probes for the 65
// outcomes, each a per-lane read of register 1 (ds_bpermute_b32: the LDS
// crossbar, no LDS memory).  The search keeps the byte address a = 4 (64 - c)
// of the first lane of b known to be below x: b is descending, so c counts
// lanes from the top, and a pad (+inf) is never below a finite value.  The
// seventh probe reads the smallest baseline value not below x_i (when there
// is one): it equals x_i exactly when x_i has a tie across the samples.
// Returns false, with r1x2 and dnum untouched, when the pooled sample has a
// tie -- between neighbours of x, between neighbours of b (real lanes only:
// pads equal each other) or across; float ==, the comparison of avg_ranks,
// so -0.0 ties +0.0.  That is exactly when avg_ranks would leave its
// run-free arm on the merged array, and the caller then takes the merge.
// Wave-uniform result; one scalar branch.
__device__ __forceinline__ bool pw_rank_search(float x, float b, int n1, int n2, unsigned& r1x2, int& dnum) {
  const unsigned long long real0 = n1 >= 64 ? ~0ull : (1ull << n1) - 1ull;          // lanes i < n1
  const unsigned long long pairs1 = n2 >= 2 ? ~0ull << (65 - n2) : 0ull;           // lanes 65 - n2 .. 63
  const float xp = lane_prev(x, 0.f), bp = lane_prev(b, 0.f);
  int a = 256;
  float y = 0.f;
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    const int t = a - (s < 6 ? (128 >> s) : 4);   // steps of 32, 16, 8, 4, 2, 1 and 1 lanes
    y = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(t, __builtin_bit_cast(int, b)));
    a = y < x ? t : a;
  }
  const unsigned long long tied =
      (__ballot(x == xp) & real0 & ~1ull) | (__ballot(b == bp) & pairs1) | (__ballot(y == x) & real0);
  if (tied != 0ull) return false;
  // Branch-free from here, in terms of g = 64 - c = a / 4 (seven known bits,
  // so the products are 24-bit multiplies without a mask).  With
  //   e_i = i n2 - c_i n1
  // the candidates of lane i are |e_i + n2|, |e_i| and |e'_i|,
  //   e'_i = i n2 - (c_(i-1) + 1) n1 = e_(i-1) + n2 - n1   (e'_0 = -n1),
  // the last only when c_i > c_(i-1), which is e'_i >= e_i.  |e_i| needs no
  // condition: where c_i = c_(i-1) it is lane i - 1's first candidate over
  // again (and e_0 = 0 there).  The gap above the largest current value needs
  // no candidate either: n1 (n2 - c - 1) is below that lane's first candidate
  // n1 (n2 - c).
  const int i = lane_id();
  const unsigned g = ((unsigned)a >> 2) & 127u;
  // g n1 + (i n2 - 64 n1) as one full-rate v_mad_u32_u24 (left to itself the
  // compiler, knowing every factor small, picks the 64-bit v_mad_u64_u32)
  const unsigned t0 = __umul24((unsigned)i, (unsigned)n2 & 127u) - 64u * (unsigned)n1;
  unsigned eu;
  asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(eu) : "v"(g), "s"(n1), "v"(t0));
  const int e = (int)eu;
  const int e1 = lane_prev(e, -n2) + (n2 - n1);
  const int ea = abs(e + n2), eb = abs(e), ec = e1 >= e ? abs(e1) : 0;
  int d = ea > eb ? ea : eb;
  d = ec > d ? ec : d;
  const bool real = i < n1;
  r1x2 = real ? 2u * (unsigned)(i - (int)g) + 130u : 0u;   // 2 (i + c) + 2
  dnum = real && n2 > 0 ? d : 0;
  return true;
}

// SEARCH (the split layout with a baseline cache only): a row without a tie
// in its pooled sample is ranked by pw_rank_search instead of the size-128
// merge; a tied row takes the merge as without it.  Same output words.
template <int K, bool SPLIT = false, class Hook = PwNoHook, class Base = PwNoBase, bool SEARCH = false>
__device__ __forceinline__ void pw_compute(PwIn<K>& in, int n_cur, int n_base, double* __restrict__ o,
                                           Hook hook = Hook(), Base bc = Base()) {
  // Everything exact is carried in integers (counts, doubled rank sums, tie
  // terms, the KS numerator); only the Welch moments are floating point.
  // Counts come from ballots (scalar popcounts), the integer sums are reduced
  // after both sorts, packed into as few words as their bounds allow, and
  // every reduction result is wave-uniform (only lane 0 writes the row).
  static_assert(!Base::kOn || SPLIT, "the baseline cache belongs to the split layout");
  const int lane = lane_id();
  float (&v)[K] = in.v;
  int tag[K];
  float s1 = 0.f, s2 = 0.f;
  int n1 = 0, n2 = 0, n;
  float m1, m2, q1 = 0.f, q2 = 0.f;
  bool hit = false;   // wave-uniform
  if constexpr (Base::kOn) {
    hit = bc.hit(v[1], n_base);
    if (!hit && lane < n_base) bc.raw[bc.at()] = __float_as_uint(v[1]);
  }
  if (Base::kOn && hit) {
    if constexpr (Base::kOn) {
      // register 0 alone, with the operations of the general form below
      // (tag[1] is rebuilt ahead of the merge, like every tag of the split layout)
      int t = lane < n_cur ? 0 : -1;
      float x = v[0];
      if (!isfinite(x)) { x = kPad; t = -1; }
      v[0] = x; tag[0] = t; tag[1] = 1;
      if (t == 0) s1 += x;
      n1 += __popcll(__ballot(t == 0));
      m1 = wave_sum_f32_uniform(s1) / (float)(n1 > 0 ? n1 : 1);
      if (tag[0] == 0) { const float d = v[0] - m1; q1 += d * d; }
      q1 = wave_sum_f32_uniform(q1);
      n2 = __builtin_amdgcn_readfirstlane((int)bc.st.x);
      m2 = __uint_as_float(bc.st.y); q2 = __uint_as_float(bc.st.z);
      n = n1 + n2;
      v[1] = __uint_as_float(bc.s);
      // needed at the merge only, but waited for here: no wait for a load may
      // follow hook.loaded()
      asm volatile("" : "+v"(v[1]));
    }
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = k * 64 + lane;
      int t = SPLIT ? (lane < (k == 0 ? n_cur : n_base) ? k : -1) : (i < n_cur ? 0 : (i < n_cur + n_base ? 1 : -1));
      float x = v[k];
      if (!isfinite(x)) { x = kPad; t = -1; }
      v[k] = x; tag[k] = t;
      if (t == 0) s1 += x;
      if (t == 1) s2 += x;
      n1 += __popcll(__ballot(t == 0));
      n2 += __popcll(__ballot(t == 1));
    }
    n = n1 + n2;
    m1 = wave_sum_f32_uniform(s1) / (float)(n1 > 0 ? n1 : 1);
    m2 = wave_sum_f32_uniform(s2) / (float)(n2 > 0 ? n2 : 1);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (tag[k] == 0) { const float d = v[k] - m1; q1 += d * d; }
      if (tag[k] == 1) { const float d = v[k] - m2; q2 += d * d; }
    }
    q1 = wave_sum_f32_uniform(q1); q2 = wave_sum_f32_uniform(q2);
    if constexpr (Base::kOn) {
      if (lane == 0)
        bc.stats[bc.row] = make_uint4((unsigned)n2, __float_as_uint(m2), __float_as_uint(q2), (unsigned)n_base);
    }
  }

  // ---- Wilcoxon signed-rank on position-paired differences (zero_method='wilcox')
  // One unsigned key per pair: (bits(|d|) << 1) | (d > 0).  |d| > 0 or the
  // +inf pad, so bit 31 of its pattern is clear and the shift loses nothing;
  // unsigned order of the keys is the order of |d| (fp32 denormals are kept in
  // this build, .amdhsa_float_denorm_mode_32 = 3, so a float compare tells
  // subnormal |d| apart exactly as the integer compare does), key >> 1 gives
  // |d|-equality for the tie runs and key & 1 the sign.  Pads: (+inf << 1).
  constexpr int KW = PwIn<K>::KW;
  constexpr unsigned kPadMag = 0x7F800000u;
  unsigned dk[KW];
  const int npair = n_cur < n_base ? n_cur : n_base;
  int nw = 0, npos = 0, nzero = 0;
#pragma unroll
  for (int k = 0; k < KW; ++k) {
    const int j = k * 64 + lane;
    const float xc = in.pc[k], xb = in.pb[k];
    const float dd = xc - xb;
    const bool ok = j < npair && isfinite(xc) && isfinite(xb);
    const bool nz = ok && dd != 0.f, pos = nz && dd > 0.f;
    dk[k] = nz ? ((__float_as_uint(fabsf(dd)) << 1) | (pos ? 1u : 0u)) : (kPadMag << 1);
    nw += __popcll(__ballot(nz));
    npos += __popcll(__ballot(pos));
    nzero += __popcll(__ballot(ok && !nz));
  }

  hook.loaded();
  // The four integer sums, packed by their bounds at n <= 64 K pooled values
  // and nw <= 64 KW pairs (what the registers hold): tie <= n^3 - n (one run),
  // r1x2 <= n (n + 1) (the doubled average ranks of all n values sum to that),
  // likewise tiew and rplus2 over nw.  K = 1: two words; K = 2 and 4: three;
  // K >= 8: four.  A tie term that shares no word comes reduced from avg_ranks.
  constexpr long long N = 64LL * K, NW = 64LL * KW;
  constexpr int bTie = pw_bits(N * N * N - N), bR1 = pw_bits(N * (N + 1));
  constexpr int bTiew = pw_bits(NW * NW * NW - NW), bRp = pw_bits(NW * (NW + 1));
  static_assert(bTie <= 32 && bTiew <= 32 && bR1 <= 32 && bRp <= 32, "32-bit sums");
  constexpr bool packA = bTie + bR1 <= 32;                        // tie | r1x2
  constexpr bool packB = bTiew + bRp <= 32;                       // tiew | rplus2
  constexpr bool packC = !packA && !packB && bR1 + bRp <= 32;     // r1x2 | rplus2
  static_assert(!SEARCH || (Base::kOn && !packA), "the search form: split layout with a baseline cache, unpacked tie term");
  unsigned r1x2 = 0;
  int dnum = 0;   // max |a1 n2 - a2 n1| over tie-run ends = D n1 n2
  int tie_l = 0;
  int dt_unused[KW];
  bool ranked = false;   // wave-uniform: the search form gave r1x2 and dnum (and the tie term is 0)
  if constexpr (Base::kOn) {
    // a hit: register 1 already stands where these stages would leave it
    if (hit) {
      bitonic_sort<K, SPLIT, true, 2, 64, 1u>(v, tag);
    } else {
      bitonic_sort<K, SPLIT, true, 2, 64>(v, tag);
      bc.sorted[bc.at()] = __float_as_uint(v[1]);
    }
    if constexpr (SEARCH) {
      // the Wilcoxon sort ahead of the branch: it is independent of the probe
      // chain (seven dependent crossbar reads), and in one block with it the
      // scheduler can fill the chain's latency with the sort's exchanges
      bitonic_sort<KW, false, false>(dk, dt_unused);
      ranked = pw_rank_search(v[0], v[1], n1, n2, r1x2, dnum);
    }
    if (!ranked) bitonic_sort<K, SPLIT, true, 128, 128>(v, tag);
  } else {
    bitonic_sort<K, SPLIT>(v, tag);
  }
  if (!ranked) {
    int rk2[K];
    bool en[K];
    tie_l = avg_ranks<K, !packA>(v, n, rk2, en);
    int base12 = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (tag[k] == 0) r1x2 += (unsigned)rk2[k];
      // KS: inclusive prefix counts of both samples along the sorted order, one packed scan
      const int a12 = wave_incl_sum(tag[k] == 0 ? 1 : (tag[k] == 1 ? (1 << 16) : 0)) + base12;
      base12 = lane_bcast(a12, 63);
      if (en[k] && n1 > 0 && n2 > 0) {
        const int a1 = a12 & 0xFFFF, a2 = a12 >> 16;
        const int dd = abs(__mul24(a1, n2) - __mul24(a2, n1));   // counts <= 1024
        dnum = dd > dnum ? dd : dnum;
      }
    }
  }
  dnum = wave_max_uniform(dnum);

  if constexpr (!SEARCH) bitonic_sort<KW, false, false>(dk, dt_unused);
  unsigned dmag[KW];
#pragma unroll
  for (int k = 0; k < KW; ++k) dmag[k] = dk[k] >> 1;
  int rw2[KW];
  bool ew[KW];
  const int tiew_l = avg_ranks<KW, !packB>(dmag, nw, rw2, ew);
  unsigned rplus2 = 0;
#pragma unroll
  for (int k = 0; k < KW; ++k)
    if ((dk[k] & 1u) != 0u) rplus2 += (unsigned)rw2[k];

  unsigned tie, tiew, r1s, rps;
  auto lowbits = [](unsigned w, int b) { return b >= 32 ? w : (w & ((1u << (b & 31)) - 1u)); };
  if constexpr (packA) {
    const unsigned w = wave_sum_uniform((unsigned)tie_l | (r1x2 << bTie));
    tie = lowbits(w, bTie); r1s = w >> bTie;
  } else {
    tie = (unsigned)tie_l;   // reduced by avg_ranks, in its tied path only
  }
  if constexpr (packB) {
    const unsigned w = wave_sum_uniform((unsigned)tiew_l | (rplus2 << bTiew));
    tiew = lowbits(w, bTiew); rps = w >> bTiew;
  } else {
    tiew = (unsigned)tiew_l;
  }
  if constexpr (packC) {
    const unsigned w = wave_sum_uniform(r1x2 | (rplus2 << bR1));
    r1s = lowbits(w, bR1); rps = w >> bR1;
  } else {
    if constexpr (!packA) r1s = wave_sum_uniform(r1x2);
    if constexpr (!packB) rps = wave_sum_uniform(rplus2);
  }

  hook.done();
  // Per-row sufficient statistics; p-values are evaluated one row per THREAD
  // by pvalue_kernel (the double-precision special functions would otherwise
  // run on lane 0 with 63 lanes idle).
  hook.store(o, n1, n2, nw, r1s, tie, dnum, rps, tiew, m1, m2, q1, q2, npos, nzero);
}

// ---------------------------------------------------------------------------
// Counting form of the same statistics (no sort).  Every average rank is
// 2*rank = 2*#(v < x) + #(v == x) + 1, the KS empirical CDFs at x are the
// "<=" counts per sample, the tie term is sum over samples of (t_i^2 - 1)
// (t_i = size of x's tie run), and the Wilcoxon ranks are the same counts over
// the non-zero |d|.  The row's values go to LDS once; each lane then sweeps
// them with broadcast ds_read_b128 (4 values per instruction, one address for
// the whole wave: conflict-free), so the work is ~n independent compare/adds
// per owned value instead of the bitonic network's dependent exchange chain.
// ---------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void pw_compute_count(PwIn<K>& in, int n_cur, int n_base, double* __restrict__ o,
                                                 float* __restrict__ lds /* >= 3*64*K + 12 floats */) {
  constexpr int KW = PwIn<K>::KW;
  const int lane = lane_id();
  const int n = n_cur + n_base;
  const int nc4 = (n_cur + 3) & ~3, nb4 = (n_base + 3) & ~3;
  float* pc = lds;                      // current sample, +inf for missing / padding
  float* pb = lds + 64 * K + 4;         // baseline sample
  float* pd = lds + 128 * K + 8;        // |d| of non-zero pairs, +inf otherwise
  float x[K];
  int tag[K];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int i = k * 64 + lane;
    int t = i < n_cur ? 0 : (i < n ? 1 : -1);
    float v = in.v[k];
    if (!isfinite(v)) { v = kPad; t = -1; }
    x[k] = v; tag[k] = t;
    if (t == 0) s1 += v;
    if (t == 1) s2 += v;
    if (i < n_cur) pc[i] = v;
    else if (i < n) pb[i - n_cur] = v;
  }
  if (lane < 4) {
    if (n_cur + lane < nc4) pc[n_cur + lane] = kPad;
    if (n_base + lane < nb4) pb[n_base + lane] = kPad;
  }
  int n1 = 0, n2 = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    n1 += __popcll(__ballot(tag[k] == 0));
    n2 += __popcll(__ballot(tag[k] == 1));
  }
  const float m1 = wave_sum(s1) / (float)(n1 > 0 ? n1 : 1), m2 = wave_sum(s2) / (float)(n2 > 0 ? n2 : 1);
  float q1 = 0.f, q2 = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (tag[k] == 0) { const float d = x[k] - m1; q1 += d * d; }
    if (tag[k] == 1) { const float d = x[k] - m2; q2 += d * d; }
  }
  q1 = wave_sum(q1); q2 = wave_sum(q2);

  const int npair = n_cur < n_base ? n_cur : n_base;
  const int npp4 = (npair + 3) & ~3;
  float dabs[KW];
  int dsgn[KW];   // 1 positive, 0 negative, -1 excluded
  int npos = 0, nneg = 0, nzero = 0;
#pragma unroll
  for (int k = 0; k < KW; ++k) {
    const int j = k * 64 + lane;
    float d = kPad;
    int t = -1;
    bool zero = false;
    if (j < npair) {
      const float xc = in.pc[k], xb = in.pb[k];
      if (isfinite(xc) && isfinite(xb)) {
        const float dd = xc - xb;
        if (dd != 0.f) { d = fabsf(dd); t = dd > 0.f ? 1 : 0; }
        else zero = true;
      }
    }
    dabs[k] = d; dsgn[k] = t;
    npos += __popcll(__ballot(t == 1));
    nneg += __popcll(__ballot(t == 0));
    nzero += __popcll(__ballot(zero));
    if (j < npp4) pd[j] = d;
  }
  const int nw = npos + nneg;
  __builtin_amdgcn_wave_barrier();   // LDS stores of this wave visible to its own reads
  __builtin_amdgcn_s_waitcnt(0xc07f);

  // pooled sample: per owned value, "<" and "==" counts against cur and base
  int lt_c[K], eq_c[K], lt_b[K], eq_b[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { lt_c[k] = 0; eq_c[k] = 0; lt_b[k] = 0; eq_b[k] = 0; }
  for (int j = 0; j < nc4; j += 4) {
    const float4 w = *reinterpret_cast<const float4*>(pc + j);
#pragma unroll
    for (int k = 0; k < K; ++k)
      lt_c[k] += (w.x < x[k]) + (w.y < x[k]) + (w.z < x[k]) + (w.w < x[k]),
      eq_c[k] += (w.x == x[k]) + (w.y == x[k]) + (w.z == x[k]) + (w.w == x[k]);
  }
  for (int j = 0; j < nb4; j += 4) {
    const float4 w = *reinterpret_cast<const float4*>(pb + j);
#pragma unroll
    for (int k = 0; k < K; ++k)
      lt_b[k] += (w.x < x[k]) + (w.y < x[k]) + (w.z < x[k]) + (w.w < x[k]),
      eq_b[k] += (w.x == x[k]) + (w.y == x[k]) + (w.z == x[k]) + (w.w == x[k]);
  }
  int r1x2 = 0, tie = 0, dnum = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (tag[k] >= 0) {
      const int lt = lt_c[k] + lt_b[k], t = eq_c[k] + eq_b[k];
      if (tag[k] == 0) r1x2 += 2 * lt + t + 1;
      tie += t * t - 1;
      if (n1 > 0 && n2 > 0) {
        const int a1 = lt_c[k] + eq_c[k], a2 = lt_b[k] + eq_b[k];
        const int dd = abs(a1 * n2 - a2 * n1);
        dnum = dd > dnum ? dd : dnum;
      }
    }
  }
  r1x2 = wave_sum(r1x2);
  tie = wave_sum(tie);
  dnum = wave_max(dnum);

  // Wilcoxon ranks among the non-zero |d|
  int rp2 = 0, tiew = 0;
  {
    int ltw[KW], eqw[KW];
#pragma unroll
    for (int k = 0; k < KW; ++k) { ltw[k] = 0; eqw[k] = 0; }
    for (int j = 0; j < npp4; j += 4) {
      const float4 w = *reinterpret_cast<const float4*>(pd + j);
      const float wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int k = 0; k < KW; ++k) ltw[k] += wv[u] < dabs[k], eqw[k] += wv[u] == dabs[k];
    }
#pragma unroll
    for (int k = 0; k < KW; ++k) {
      if (dsgn[k] >= 0) {
        tiew += eqw[k] * eqw[k] - 1;
        if (dsgn[k] == 1) rp2 += 2 * ltw[k] + eqw[k] + 1;
      }
    }
  }
  rp2 = wave_sum(rp2);
  tiew = wave_sum(tiew);
  __builtin_amdgcn_wave_barrier();   // the LDS slot is reused by the next row

  if (lane == 0) {
    o[0] = n1; o[1] = n2; o[2] = nw; o[3] = 0.5 * r1x2; o[4] = tie;
    o[5] = (n1 > 0 && n2 > 0) ? (double)dnum / ((double)n1 * n2) : 0.0;
    o[6] = 0.5 * rp2; o[7] = tiew; o[8] = m1; o[9] = m2; o[10] = q1; o[11] = q2;
    o[12] = npos; o[13] = nzero;
  }
}

// One row's sufficient statistics (sort form): the split layout when both
// samples fit one register each (the usual 5 pods x 10 points per side).
template <int K>
__device__ __forceinline__ void pw_row(const float* __restrict__ c, const float* __restrict__ b, int n_cur,
                                       int n_base, double* __restrict__ o) {
  PwIn<K> in;
  if constexpr (K == 2) {
    if (n_cur <= 64 && n_base <= 64) {
      pw_load<K, true>(c, b, n_cur, n_base, in);
      pw_compute<K, true>(in, n_cur, n_base, o);
      return;
    }
  }
  pw_load<K>(c, b, n_cur, n_base, in);
  pw_compute<K>(in, n_cur, n_base, o);
}

// p-value of ONE test for one row from its sufficient statistics (NaN when the
// test is gated out).  t is uniform per workgroup (grid y), so the fp64
// special-function code paths never diverge inside a wave.
__device__ __forceinline__ void eval_test(int t, const double* __restrict__ o, int min_mw, int min_wil, int min_kru,
                                          double& pv, double& sv) {
  const int n1 = (int)o[0], n2 = (int)o[1], nw = (int)o[2];
  const double r1 = o[3], tie = o[4], dmax = o[5], rplus = o[6], tiew = o[7];
  const double m1 = o[8], m2 = o[9], q1 = o[10], q2 = o[11];
  const int n = n1 + n2;
  const double NaN = __builtin_nan("");
  pv = NaN;
  sv = NaN;
  const double dn1 = n1, dn2 = n2, dn = n;
  switch (t) {
    case T_MW:
      if (n1 >= min_mw && n2 >= min_mw && n1 > 0 && n2 > 0) {
        const double u1 = r1 - dn1 * (dn1 + 1.0) / 2.0;
        const double u2 = dn1 * dn2 - u1;
        const double u = u1 > u2 ? u1 : u2;
        const double mu = dn1 * dn2 / 2.0;
        const double var = dn1 * dn2 / 12.0 * ((dn + 1.0) - tie / (dn * (dn - 1.0)));
        sv = u1;
        if (var > 0) {
          const double z = (u - mu - 0.5) / sqrt(var);
          double pp = 2.0 * norm_sf(z);
          pv = pp > 1.0 ? 1.0 : pp;
        } else {
          pv = 1.0;
        }
      }
      break;
    case T_KRU:
      if (n1 >= min_kru && n2 >= min_kru && n1 > 0 && n2 > 0) {
        const double r2 = dn * (dn + 1.0) / 2.0 - r1;
        double h = 12.0 / (dn * (dn + 1.0)) * (r1 * r1 / dn1 + r2 * r2 / dn2) - 3.0 * (dn + 1.0);
        const double corr = 1.0 - tie / (dn * dn * dn - dn);
        if (corr > 0) {
          sv = h / corr;
          pv = h / corr > 0 ? erfc(sqrt(0.5 * h / corr)) : 1.0;   // chi2(1) survival
        }
      }
      break;
    case T_KS:
      if (n1 >= min_mw && n2 >= min_mw && n1 > 0 && n2 > 0) {
        const double en_ = dn1 * dn2 / (dn1 + dn2);
        sv = dmax;
        pv = kolmogorov_sf(sqrt(en_) * dmax);
      }
      break;
    case T_T:
      if (n1 >= 2 && n2 >= 2 && n1 >= min_kru && n2 >= min_kru) {
        const double v1 = q1 / (dn1 - 1.0), v2 = q2 / (dn2 - 1.0);
        const double se2 = v1 / dn1 + v2 / dn2;
        if (se2 > 0) {
          const double tt = (m1 - m2) / sqrt(se2);
          const double a = v1 / dn1, bb = v2 / dn2;
          const double df = se2 * se2 / (a * a / (dn1 - 1.0) + bb * bb / (dn2 - 1.0));
          sv = tt;
          pv = student_t_2sided(tt, df);
        }
      }
      break;
    case T_WIL:
      if (nw >= min_wil && nw > 0) {
        const double dnw = nw;
        const double tot = dnw * (dnw + 1.0) / 2.0;
        const double rminus = tot - rplus;
        const double T = rplus < rminus ? rplus : rminus;
        const double mn = dnw * (dnw + 1.0) / 4.0;
        const double se = sqrt(dnw * (dnw + 1.0) * (2.0 * dnw + 1.0) / 24.0 - tiew / 48.0);
        sv = T;
        if (se > 0) {
          double pp = 2.0 * norm_sf(fabs((T - mn) / se));
          pv = pp > 1.0 ? 1.0 : pp;
        }
      }
      break;
    default: {  // T_FRI: k = 2 treatments over paired blocks, (n+ - n-)^2 / (n+ + n-), chi2(1)
      const int npos = (int)o[12], nzero = (int)o[13];
      const int nneg = nw - npos, b = nw + nzero;
      if (b >= min_wil && b > 0) {
        const double q = nw > 0 ? (double)(npos - nneg) * (npos - nneg) / nw : 0.0;
        sv = q;
        pv = q > 0 ? erfc(sqrt(0.5 * q)) : 1.0;
      }
    }
  }
}
