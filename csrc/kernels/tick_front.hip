// fm-hipcc-flags: -mllvm -pragma-unroll-threshold=1000000 -mllvm -amdgpu-atomic-optimizer-strategy=None
// (the 1024-sample pairwise sort, K = 16: past LLVM's default pragma-unroll
// size limit the stage loops stayed rolled -- runtime register indexing
// through scratch (132 B/lane) and s_set_gpr_idx; fully unrolled: 0 scratch.
// Atomic optimizer off: every fetch-add here is already issued by one lane,
// and the pass's wave aggregation reads the result back -- a vmcnt(0) --
// right behind the instruction, which is what the pairwise row queue places
// its request inside the row to avoid.)
#include "fm_pairwise.h"
#include "fm_row_stats.h"

// ---------------------------------------------------------------------------
// Horizontally fused front half of the canary tick: ONE launch whose
// workgroups take one of two roles by blockIdx.
//   * blockIdx <  nP: pairwise role — grid-stride over rows, one wave per row
//     (sorted-rank sufficient statistics), then the workgroup evaluates the
//     six p-values of its own rows, one (test, row) pair per thread,
//     test-major so a wave mostly runs one special function;
//   * blockIdx >= nP: history role — mean / std / count of a 7-day row per
//     workgroup (HBM-bound, grid-stride over rows).
// The compute-bound and the HBM-bound halves share every CU without a
// second stream: no fork/join in the graph (the side branch of a two-stream
// graph starts ~11-13 us late, and whether the branches land on different
// hardware queues varied run to run: profiles/tick_timeline_*.txt).  The
// pairwise workgroups have the lowest ids, so the dispatcher places them
// first and the history workgroups fill the remaining slots.  (A steady
// launch with the pairwise row queue, tick_front_dyn_kernel, turns the order
// round: see tick_front_body.)
// ---------------------------------------------------------------------------
// Out-of-line p-value evaluation for the fused kernel: inlined into the
// role-split kernel the special functions pushed it to 256 VGPRs (one wave
// per SIMD); as a call the kernel keeps the history role's 96.
__device__ __attribute__((noinline)) void eval_test_call(int t, const double* __restrict__ o, int min_mw, int min_wil,
                                                         int min_kru, double& pv, double& sv) {
  eval_test(t, o, min_mw, min_wil, min_kru, pv, sv);
}

// FM_FRONT_TIMING builds (tools/front_timing.py): every workgroup of the
// front kernel records its start / end on the 100 MHz real-time counter, so
// the critical role (pairwise or history) of a shape can be read off; a
// pairwise workgroup also records the barrier between its rank-test rows and
// its p-values (mark 2; a history workgroup leaves that slot alone) and the
// number of rows it ranked (mark 3, a count, not a time).
#ifdef FM_FRONT_TIMING
constexpr int kFtMarks = 4;
__device__ unsigned long long g_front_t[kFtMarks * 8192];
#define FM_FT_MARK(k) \
  do { if (threadIdx.x == 0 && blockIdx.x < 8192) g_front_t[kFtMarks * blockIdx.x + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define FM_FT_ROWS(n) \
  do { if (threadIdx.x == 0 && blockIdx.x < 8192) g_front_t[kFtMarks * blockIdx.x + 3] = (unsigned long long)(n); } while (0)
#else
#define FM_FT_MARK(k) do {} while (0)
#define FM_FT_ROWS(n) do {} while (0)
#endif

// Everything a front launch reads and writes, the kernel's one argument.
// rowmap, cache / valid and queue may be null; scan: the history role tests
// the row-statistics cache (front_hist_scan) instead of streaming every row.
// The fields are grouped by who reads them, and the order is part of the
// kernel's register budget: the compiler merges the loads of adjacent fields
// into one wide scalar load whose registers stay live as long as any of them
// does.  With R among the history pointers, or the p-value fields ahead of
// the rank-test fields, the NV >= 10 instantiations spilled SGPRs into 3-8
// more VGPRs (NV = 12: 91 -> 98, a wave per SIMD less).
struct FrontArgs {
  int64_t R;
  int nP, scan, T;
  // history roles
  const float* hist;
  int64_t ld_h;
  float* hs;   // [R, 3]
  const int* rowmap;
  float* cache;
  unsigned* valid;
  unsigned* queue;
  // pairwise roles: the rank-test rows ...
  const float* cur;
  int64_t ld_c;
  const float* base;
  int64_t ld_b;
  double* suff;
  int n_cur, n_base;
  // ... and their p-values
  float *pvals, *pstats;
  int min_mw, min_wil, min_kru;
  // the baseline cache of the rank-test rows (fm_pairwise.h PwBaseCache), or
  // all three null.  Last, so that a kernel without it (BC = false) reads the
  // fields above exactly where it always did.
  unsigned *bc_raw, *bc_sorted;
  uint4* bc_stats;
};

// Control block of the front kernel's history queue (uint32 words from
// queue[kXcdCtl]; the queue is 8 x 32 counters + this block, zeroed by the
// host, kCtlOn set to 1 to enable the balancing): a split-is-set flag, the
// ranges done this tick, the 9 range bounds as fractions of the rows (2^-24
// fixed point, so a split survives the row count changing with fleet churn:
// range x is rows [R f[x] >> 24, R f[x+1] >> 24)), and per-XCD start / end
// times (u64, 100 MHz) of this tick.
constexpr int kXcdCtl = 256, kCtlR = 0, kCtlDone = 1, kCtlB = 2, kCtlOn = 31, kCtlT0 = 32, kCtlT1 = 48;
constexpr int64_t kXcdMinRows = 32768;
constexpr int kFracBits = 24;
// Rebalance only when the ranges ended more than kXcdBand apart, and then
// 1 / kXcdStep of the way; rows per grab of the history queue.
constexpr double kXcdBand = 1.015, kXcdStep = 3.0;
constexpr int kHistChunk = 1;
__device__ inline int64_t xcd_bound(int64_t R, unsigned f) { return (R * (int64_t)f) >> kFracBits; }

// The last workgroup of XCD range ``xcd``: its end time; the last range of
// the tick to finish computes the next tick's bounds.
__device__ __attribute__((noinline)) void xcd_rebalance(unsigned* ctl, int xcd, int64_t R) {
  unsigned long long* t0 = reinterpret_cast<unsigned long long*>(ctl + kCtlT0);
  unsigned long long* t1 = reinterpret_cast<unsigned long long*>(ctl + kCtlT1);
  __hip_atomic_store(t1 + xcd, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned g = __hip_atomic_fetch_add(ctl + kCtlDone, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  if (g != 7u) return;
  __hip_atomic_store(ctl + kCtlDone, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (R < 64 || R > 0x7fffffff) return;
  const bool had = __hip_atomic_load(ctl + kCtlR, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
  constexpr double one = (double)(1u << kFracBits);
  double b[9], f[9], rate[8], tot = 0.0;
  for (int x = 0; x <= 8; ++x) {   // this tick's bounds, exactly as the history role derived them
    const unsigned fx = __hip_atomic_load(ctl + kCtlB + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    b[x] = had ? (double)xcd_bound(R, fx) : (double)(R * x / 8);
    f[x] = had ? (double)fx / one : (double)x / 8.0;
  }
  for (int x = 0; x < 8; ++x) {
    const unsigned long long a = __hip_atomic_load(t0 + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long e = __hip_atomic_load(t1 + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double rows = b[x + 1] - b[x];
    if (!(e > a) || e - a > 100000000ull || rows < 1.0) return;   // (a range with no start this tick: keep the split)
    rate[x] = rows / (double)(e - a);
    tot += rate[x];
  }
  // a third of the way towards the split that would have ended every range
  // together, and only when the ranges ended more than 1.5 % apart (per-tick
  // noise is not steered by)
  double dmin = 1e300, dmax = 0.0;
  for (int x = 0; x < 8; ++x) {
    const double d = (b[x + 1] - b[x]) / rate[x];
    dmin = d < dmin ? d : dmin;
    dmax = d > dmax ? d : dmax;
  }
  if (had && dmax < kXcdBand * dmin) return;
  // in fraction space; every range keeps at least 1/64 of the rows (an XCD a
  // quarter of the mean speed), so no range empties and stops being timed
  constexpr double minf = 1.0 / 64.0;
  double acc = 0.0, prev = 0.0;
  unsigned nf[9];
  nf[0] = 0;
  for (int x = 0; x < 8; ++x) {
    acc += rate[x] / tot;
    double v = ((kXcdStep - 1.0) * f[x + 1] + acc) / kXcdStep;   // (1 / kXcdStep of the way)
    const double minv = prev + minf, maxv = 1.0 - (double)(7 - x) * minf;
    v = v < minv ? minv : (v > maxv ? maxv : v);
    nf[x + 1] = x == 7 ? (1u << kFracBits) : (unsigned)(v * one + 0.5);
    prev = (double)nf[x + 1] / one;
  }
  for (int x = 0; x <= 8; ++x) __hip_atomic_store(ctl + kCtlB + x, nf[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(ctl + kCtlR, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------
// Dynamic row queue of the pairwise role (tick_front_dyn_kernel).  Equal static
// shares of rows do not end together: the five pairwise waves of a SIMD are
// all VALU-issue-bound and the issue arbiter favours the oldest, so the
// workgroups dispatched last rank their rows slowest (docs/PERF.md, "Dynamic
// pairwise rows").  A wave therefore takes only `s` rows by the static formula
// (no atomics) and then grabs rows one at a time from the pool [pool0, R),
// which is cut into `q` contiguous ranges with one counter each (one 128-B
// line per counter: pq[x * 32], the word after it counts the workgroups done).
// Pairwise workgroup pb uses range (pb + pb / q) % q, so a range is shared by
// workgroups of every dispatch age and of every XCD (ids are dealt round-robin
// over the XCDs), and a counter sees a few hundred fetch-adds per tick
// (cross-XCD atomics on one address serialise at ~28 ns).
// No wave or workgroup ever waits on another: the only cross-workgroup
// operations are relaxed fetch-adds, there are no flags, spins or fences, and
// a workgroup evaluates the p-values of exactly the rows its own waves
// ranked (their list is kept in LDS), so no `suff` row crosses workgroups
// inside the launch.  The last workgroup of a range to finish zeroes its two
// words for the next launch (every other workgroup of the range has made its
// last grab by then).
// ---------------------------------------------------------------------------
constexpr int kRowCap = 64;   // rows one wave may rank (its LDS list); front_plan keeps 4 nP kRowCap >= R
constexpr int kDynShare = 85; // percent of a wave's even share of the rows it takes statically
struct FrontDyn {
  unsigned* pq;   // q x 32 words, zero between launches
  int q;          // ranges (1 <= q <= nP)
  int s;          // static rows per wave
  int pool0;      // first dynamic row (= 4 nP s)
};

// A wave's request for its next queue index, placed inside the row it is
// ranking (the hook of pw_compute): lane 0's fetch-add is issued once the
// row's loads have been consumed, so no later wait for a load also waits for
// it, and it returns under the row's sorts; the index is read back (wave-
// uniform) after the last reduction, ahead of the row's stores.  The empty asm
// pins that read: without it the compiler hoists the readfirstlane, and with it
// a vmcnt(0), to right behind the fetch-add.
//
// The row's sink (store) keeps the fp64 out of the row: lane 0 puts the 14
// statistics, as the raw integer / float words the reductions left, into the
// row's 64-byte LDS slot (no conversion, no division, no global store), and
// the workgroup turns its slots into the doubles of `suff` one row per thread
// behind its barrier (front_raw_to_suff).  A one-lane instruction costs the
// SIMD a full issue slot, and the conversions with their IEEE division were
// 35-40 of them per row.
constexpr int kRawWords = 16;   // one slot: the 14 words + 2 of padding
struct PwGrab {
  unsigned* ctr;
  bool want;        // wave-uniform
  unsigned& next;   // out (wave-uniform), when want
  unsigned* raw;    // the row's LDS slot (kRawWords words, 16-byte aligned)
  unsigned idx = 0;
  __device__ __forceinline__ void loaded() {
    if (want && lane_id() == 0) idx = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void done() {
    if (want) {
      asm volatile("" : "+v"(idx));
      next = (unsigned)__builtin_amdgcn_readfirstlane((int)idx);
    }
  }
  __device__ __forceinline__ void store(double*, int n1, int n2, int nw, unsigned r1s, unsigned tie, int dnum,
                                        unsigned rps, unsigned tiew, float m1, float m2, float q1, float q2, int npos,
                                        int nzero) const {
    if (lane_id() == 0) {
      uint4* s = reinterpret_cast<uint4*>(raw);
      s[0] = make_uint4((unsigned)n1, (unsigned)n2, (unsigned)nw, r1s);
      s[1] = make_uint4(tie, (unsigned)dnum, rps, tiew);
      s[2] = make_uint4(__float_as_uint(m1), __float_as_uint(m2), __float_as_uint(q1), __float_as_uint(q2));
      *reinterpret_cast<uint2*>(raw + 12) = make_uint2((unsigned)npos, (unsigned)nzero);
    }
  }
};

// One raw slot -> the row's 14 doubles, exactly pw_store_suff's operations.
__device__ __forceinline__ void front_raw_to_suff(const unsigned* __restrict__ raw, double* __restrict__ o) {
  const uint4 a = reinterpret_cast<const uint4*>(raw)[0], b = reinterpret_cast<const uint4*>(raw)[1];
  const uint4 c = reinterpret_cast<const uint4*>(raw)[2];
  const uint2 d = *reinterpret_cast<const uint2*>(raw + 12);
  pw_store_suff(o, (int)a.x, (int)a.y, (int)a.z, a.w, b.x, (int)b.y, b.z, b.w, __uint_as_float(c.x),
                __uint_as_float(c.y), __uint_as_float(c.z), __uint_as_float(c.w), (int)d.x, (int)d.y);
}

// Row `row` of a launch with the baseline cache (the BC = true kernels), with
// the hook of the caller.  The host starts those kernels only for the split
// layout (K = 2, n_cur <= 64, n_base <= 64), so they carry no other form of
// the row, and a launch without a cache runs a kernel without a trace of it.
// The entry's loads are issued with the row's own, ahead of everything
// pw_compute does.  RS: a row without a tie in its pooled sample is ranked by
// searching each current value in the sorted baseline instead of the
// size-128 merge (fm_pairwise.h pw_rank_search); RS = false compiles the row
// without a trace of the search (FM_RANK_SEARCH=0, rank_search() below).
template <bool RS, class Hook>
__device__ __forceinline__ void pw_row_cached(const FrontArgs& a, int64_t row, double* __restrict__ o, Hook hook) {
  const float* __restrict__ c = a.cur + row * a.ld_c;
  const float* __restrict__ b = a.base + row * a.ld_b;
  PwIn<2> in;
  pw_load<2, true>(c, b, a.n_cur, a.n_base, in);
  PwBaseCache bc{a.bc_raw, a.bc_sorted, a.bc_stats, (unsigned)row};
  bc.load(a.n_base);
  pw_compute<2, true, Hook, PwBaseCache, RS>(in, a.n_cur, a.n_base, o, hook, bc);
}

// pw_row with the request for the wave's next row inside it; the row's
// statistics go to its LDS slot `raw`.
template <int K>
__device__ __forceinline__ void pw_row_grab(const float* __restrict__ c, const float* __restrict__ b, int n_cur,
                                            int n_base, unsigned* raw, bool want, unsigned* ctr, unsigned& next) {
  PwIn<K> in;
  if constexpr (K == 2) {
    if (n_cur <= 64 && n_base <= 64) {
      pw_load<K, true>(c, b, n_cur, n_base, in);
      pw_compute<K, true>(in, n_cur, n_base, nullptr, PwGrab{ctr, want, next, raw});
      return;
    }
  }
  pw_load<K>(c, b, n_cur, n_base, in);
  pw_compute<K, false>(in, n_cur, n_base, nullptr, PwGrab{ctr, want, next, raw});
}

// The p-value phase of a pairwise workgroup, after the barrier behind its
// rank-test rows: the six p-values of its nr local rows, one (test, row) pair
// per thread.  rowOf(j), j < nr: the global row of local row j, or negative
// where there is none.
// Wave-sized chunks of (test, 64 rows); the test is wave-uniform so the
// special-function switch stays a scalar branch (a per-lane test index
// made the compiler keep every path live: 256 VGPRs).  Chunks are listed
// costliest test first (Welch's incomplete beta, then the Kolmogorov
// series, then the erfc tests) and dealt to the four waves back and forth
// (0 1 2 3 3 2 1 0 ...), so at one chunk per test the Welch and KS chunks
// have a wave each and the four cheap tests pair up.  Wave w of every
// co-resident workgroup sits on the same SIMD and all of them reach this
// phase together, so the deal is rotated by the workgroup's index (slot =
// (wave + workgroup) & 3): the Welch chains of neighbouring workgroups land
// on different SIMDs.
template <class RowOf>
__device__ __forceinline__ void front_pvalues(const FrontArgs& a, int nr, int slot, RowOf rowOf) {
  // T_T, T_KS, T_MW, T_KRU, T_WIL, T_FRI, one per nibble from the low end
  static_assert(T_T == 4 && T_KS == 3 && T_MW == 0 && T_KRU == 2 && T_WIL == 1 && T_FRI == 5, "kByCost");
  constexpr unsigned kByCost = 0x512034u;
  const int cpt = (nr + 63) >> 6;
  for (int u = 0;; ++u) {
    const int ci = (u >> 1) * 8 + ((u & 1) ? 7 - slot : slot);
    if (ci >= N_TESTS * cpt) break;
    const int tp = ci / cpt;
    const int t = __builtin_amdgcn_readfirstlane((int)((kByCost >> (4 * tp)) & 7u));
    const int j = (ci - tp * cpt) * 64 + lane_id();
    const int64_t row = j < nr ? rowOf(j) : -1;
    if (row >= 0) {
      double pv, sv;
      eval_test_call(t, a.suff + row * kSuff, a.min_mw, a.min_wil, a.min_kru, pv, sv);
      a.pvals[row * N_TESTS + t] = (float)pv;
      a.pstats[row * N_TESTS + t] = (float)sv;
    }
  }
}

// The pairwise role of workgroup pb (0 <= pb < nP) with static rows: a wave
// per row, grid-stride.
template <int K, bool BC, bool RS>
__device__ __forceinline__ void front_pairwise_static(const FrontArgs& a, const int pb) {
  const int64_t R = a.R, first = (int64_t)pb * 4, stride = (int64_t)a.nP * 4;
  for (int64_t row = first + wave_id(); row < R; row += stride) {
    if constexpr (BC) pw_row_cached<RS>(a, row, a.suff + row * kSuff, PwNoHook());
    else pw_row<K>(a.cur + row * a.ld_c, a.base + row * a.ld_b, a.n_cur, a.n_base, a.suff + row * kSuff);
  }
  __syncthreads();   // this workgroup's suff rows are visible to all its waves
  FM_FT_MARK(2);
  // local row j -> global row first + (j & 3) + (j >> 2) * stride
  const int64_t span = R > first ? R - first : 0;
  const int nr = (int)(((span + stride - 1) / stride) * 4);
#ifdef FM_FRONT_TIMING
  {
    int64_t took = 0;
    for (int w = 0; w < 4; ++w) took += span > w ? (span - w + stride - 1) / stride : 0;
    FM_FT_ROWS(took);
  }
#endif
  front_pvalues(a, nr, (wave_id() + pb) & 3, [&](int j) {
    const int64_t row = first + (j & 3) + (int64_t)(j >> 2) * stride;
    return row < R ? row : (int64_t)-1;
  });
}

// The pairwise role of workgroup pb (0 <= pb < nP) with dynamic rows.
template <int K, bool BC, bool RS>
__device__ __forceinline__ void front_pairwise_dyn(const FrontArgs& a, const FrontDyn& dq, const int pb) {
  __shared__ int s_rows[4][kRowCap];
  __shared__ int s_cnt[4];
  __shared__ __attribute__((aligned(16))) unsigned s_raw[4][kRowCap][kRawWords];   // 16 KB: the rows' raw statistics
  const int w = wave_id(), lane = lane_id();
  const int nP = a.nP, W = nP * 4, Q = dq.q;
  const int x = (pb + pb / Q) % Q;
  const int64_t pool = a.R - dq.pool0;
  const int lo = dq.pool0 + (int)(pool * x / Q), hi = dq.pool0 + (int)(pool * (x + 1) / Q);
  const unsigned nx = (unsigned)(hi - lo);       // rows of this range (0: nobody touches its counter)
  unsigned* ctr = dq.pq + x * 32;
  unsigned next = 0;                             // the index drawn last (wave-uniform)
  bool pending = false;                          // an index was drawn and its row is not yet taken
  if (dq.s == 0 && nx != 0u) {                   // no static row to draw it under
    unsigned idx = 0;
    if (lane == 0) idx = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    next = (unsigned)__builtin_amdgcn_readfirstlane((int)idx);
    pending = true;
  }
  const int cls = pb / (nP >= 5 ? nP / 5 : 1);   // dispatch age class: the pairwise ids in fifths
  int i = 0;                                     // rows ranked by this wave
  for (;;) {
    int row;
    if (i < dq.s) {
      row = pb * 4 + w + i * W;                  // (< pool0 <= R)
    } else {
      if (!pending) break;                       // list full (or an empty range)
      if (next >= nx) break;                     // range drained
      row = lo + (int)next;
    }
    // rotating wave priority: VALU issue goes by priority, then age, so left
    // alone the oldest of a SIMD's pairwise waves runs nearly unimpeded and
    // the youngest gets the leftover slots (the static tick's five end times,
    // 52 .. 114 us by dispatch age class).  With (age class + rows done) & 3
    // every wave is the arbitration winner for an equal share of its rows.
    switch ((cls + i) & 3) {
      case 0: __builtin_amdgcn_s_setprio(0); break;
      case 1: __builtin_amdgcn_s_setprio(1); break;
      case 2: __builtin_amdgcn_s_setprio(2); break;
      default: __builtin_amdgcn_s_setprio(3); break;
    }
    // the next index is requested only when the list will have room for its
    // row: every index drawn below nx is ranked by the wave that drew it
    const bool want = nx != 0u && i + 1 >= dq.s && i + 1 < kRowCap;
    if constexpr (BC)
      pw_row_cached<RS>(a, (int64_t)row, nullptr, PwGrab{ctr, want, next, s_raw[w][i]});
    else
      pw_row_grab<K>(a.cur + (int64_t)row * a.ld_c, a.base + (int64_t)row * a.ld_b, a.n_cur, a.n_base, s_raw[w][i],
                     want, ctr, next);
    pending = want;
    if (lane == 0) s_rows[w][i] = row;
    ++i;
  }
  __builtin_amdgcn_s_setprio(0);
  if (lane == 0) s_cnt[w] = i;
  __syncthreads();   // this workgroup's raw rows and row lists are visible to all its waves
  FM_FT_MARK(2);
  // local row j: the four waves' lists, concatenated
  const int c0 = s_cnt[0], c1 = c0 + s_cnt[1], c2 = c1 + s_cnt[2], nr = c2 + s_cnt[3];
  FM_FT_ROWS(nr);
  auto listed = [&](int j, int& ww, int& k) {   // local row j is entry k of wave ww's list
    ww = (j >= c0 ? 1 : 0) + (j >= c1 ? 1 : 0) + (j >= c2 ? 1 : 0);
    k = j - (ww == 0 ? 0 : (ww == 1 ? c0 : (ww == 2 ? c1 : c2)));
  };
  // raw words -> the doubles of suff, one row per thread (nr <= 4 kRowCap = 256)
  if ((int)threadIdx.x < nr) {
    int ww, k;
    listed((int)threadIdx.x, ww, k);
    front_raw_to_suff(s_raw[ww][k], a.suff + (int64_t)s_rows[ww][k] * kSuff);
  }
  __syncthreads();   // this workgroup's suff rows are visible to all its waves
  front_pvalues(a, nr, (w + pb) & 3, [&](int j) {
    int ww, k;
    listed(j, ww, k);
    return (int64_t)s_rows[ww][k];
  });
  // every wave of this workgroup made its last grab before the barrier above
  if (nx != 0u && threadIdx.x == 0) {
    const int full = nP / Q, rem = nP - full * Q;
    const int xr = x - full % Q;                 // range x is range (x - full) mod Q of the partial round
    const unsigned nwg = (unsigned)(full + ((xr < 0 ? xr + Q : xr) < rem ? 1 : 0));
    const unsigned d = __hip_atomic_fetch_add(ctr + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (d == nwg - 1u) {
      __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ctr + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// The three history roles: workgroup hb of nH writes hs[row * 3 ..] of its
// rows (hist_row_emit, fm_row_stats.h; red / redi: its reduction scratch).
//
// Row-statistics cache (fm_row_stats.h).  scan: the host expects (nearly)
// every row to hit -- the history workgroups test their rows one per
// thread, copy the hits and reduce only the misses.  Otherwise (first tick,
// after an invalidation, no cache) every row is taken as a miss without
// looking: the stride or the queue role, plus the cache entry of each row it
// computes.  Either way the device decides what is computed; the host's
// expectation only picks the shape.
template <int NV>
__device__ __forceinline__ void front_hist_scan(const FrontArgs& a, int64_t hb, int nH, double* red, int* redi) {
  __shared__ int s_list[256];
  __shared__ int s_cnt;
  hist_scan_cached<NV>(a.hist, a.ld_h, a.T, a.R, a.hs, a.rowmap, a.cache, a.valid, hb, nH, red, redi, s_list, &s_cnt);
}

// Static grid-stride over the rows (no queue given).  This role and the queue
// role take their pointers as __restrict__ parameters, not as FrontArgs: read
// through the struct their row loops reloaded spilled SGPRs (+34 .. +700
// VALU per kernel; 7 / 27 / 48 more VGPRs at NV = 10 / 12 / 16).
template <int NV>
__device__ __forceinline__ void front_hist_stride(const float* __restrict__ hist, int64_t ld_h, int T, int64_t R,
                                                  float* __restrict__ hs, const int* __restrict__ rowmap,
                                                  float* __restrict__ cache, unsigned* __restrict__ valid, int64_t hb,
                                                  int nH, double* red, int* redi) {
  for (int64_t row = hb; row < R; row += nH)
    hist_row_emit<NV, false>(hist, ld_h, T, hs, rowmap, cache, valid, row, red, redi);
}

// Dynamic history queue: the rows are split into 8 contiguous ranges, one
// per XCD (workgroup ids are dealt round-robin over the XCDs), and the
// history workgroups of a range grab chunks of kHistChunk rows from its
// counter (one 128-B line per counter).  A slot freed by a finished
// pairwise workgroup is then filled by a history workgroup that starts late
// and simply takes what is left, instead of idling (static grid-stride).
// The next chunk index is requested while the current chunk streams.  The
// last workgroup of a range to find it empty resets the counters for the
// next tick (every other workgroup of the range has already exited).
// One row per grab: at the 1,250-service shard (~10 rows per workgroup) the
// tail waits on at most one row instead of two (0.0951/0.0919 -> 0.0937/
// 0.0904 ms per step, interleaved runs); neutral at 10k services.
template <int NV>
__device__ __forceinline__ void front_hist_queue(const float* __restrict__ hist, int64_t ld_h, int T, int64_t R,
                                                 float* __restrict__ hs, const int* __restrict__ rowmap,
                                                 float* __restrict__ cache, unsigned* __restrict__ valid,
                                                 unsigned* __restrict__ queue, int64_t hb, int nH, double* red,
                                                 int* redi) {
  __shared__ unsigned s_next;
  const int xcd = (int)hb & 7;
  const int nwg = (nH >> 3) + ((nH & 7) > xcd ? 1 : 0);   // workgroups sharing this range
  // XCD-balanced ranges: the XCDs do not stream equally fast (per-XCD end
  // times of the history role, tools/front_timing.py: XCDs 3-5 end 30-40 us
  // after XCDs 0-2 at 80k rows, the same XCDs tick after tick), so the range
  // split adapts -- the last range to finish re-divides the rows in
  // proportion to each XCD's measured rows per microsecond for the next tick
  // (1/3 steps, as fractions of the rows, so the split carries over when the
  // fleet's row count changes).  queue[256..320): control block (kXcdCtl).
  unsigned* ctl = queue + kXcdCtl;
  int64_t lo = R * xcd / 8, hi = R * (xcd + 1) / 8;
  auto ld = [](const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  // (agent-scope loads: written by another XCD last tick).  Small fleets keep
  // the even split: at the 1,250-service shard (10k rows) the per-tick
  // durations are too short and noisy to steer by (0.078 -> 0.081 ms measured)
  const bool bal = R >= kXcdMinRows && ld(ctl + kCtlOn) == 1u;
  if (bal && ld(ctl + kCtlR) != 0u) {
    lo = xcd_bound(R, ld(ctl + kCtlB + xcd));
    hi = xcd_bound(R, ld(ctl + kCtlB + xcd + 1));
  }
  unsigned* ctr = queue + xcd * 32;
  if (threadIdx.x == 0) {
    s_next = atomicAdd(ctr, (unsigned)kHistChunk);
    if (bal && s_next == 0u)       // the range's first grab: its start time
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(ctl + kCtlT0) + xcd, __builtin_amdgcn_s_memrealtime(),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  int64_t r0 = lo + (int64_t)s_next;
  while (r0 < hi) {
    unsigned nxt = 0;
    if (threadIdx.x == 0) nxt = atomicAdd(ctr, (unsigned)kHistChunk);
    const int64_t r1 = r0 + kHistChunk < hi ? r0 + kHistChunk : hi;
    for (int64_t row = r0; row < r1; ++row)
      hist_row_emit<NV, false>(hist, ld_h, T, hs, rowmap, cache, valid, row, red, redi);
    __syncthreads();               // everyone is done reading s_next
    if (threadIdx.x == 0) s_next = nxt;
    __syncthreads();
    r0 = lo + (int64_t)s_next;
  }
  if (threadIdx.x == 0) {
    const unsigned d = atomicAdd(ctr + 1, 1u);
    if (d == (unsigned)nwg - 1) {
      __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ctr + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (bal) xcd_rebalance(ctl, xcd, R);
    }
  }
}

// Block id -> role.  Static rows (tick_front_kernel, any history role): the
// pairwise workgroups have the lowest ids (see the top).  DYN
// (tick_front_dyn_kernel, the scan shape only: front_plan): the pairwise role
// takes its rows from the queue above and the (short) history role has the
// lowest block ids: its workgroups are placed first and are gone after a few
// microseconds, and the pairwise workgroups that inherit their slots start
// late and simply grab fewer rows.
template <int NV, int K, bool DYN, bool BC, bool RS>
__device__ __forceinline__ void tick_front_body(const FrontArgs& a, const FrontDyn& dq) {
  __shared__ double red[4];
  __shared__ int redi[4];
  FM_FT_MARK(0);
  const int nH = (int)gridDim.x - a.nP;
  const int pb = DYN ? (int)blockIdx.x - nH : (int)blockIdx.x;                  // pairwise workgroup index
  const int64_t hb = DYN ? (int64_t)blockIdx.x : (int64_t)blockIdx.x - a.nP;   // history workgroup index
  if (pb >= 0 && pb < a.nP) {
    if constexpr (DYN) front_pairwise_dyn<K, BC, RS>(a, dq, pb);
    else front_pairwise_static<K, BC, RS>(a, pb);
  } else if (DYN || a.scan) {
    front_hist_scan<NV>(a, hb, nH, red, redi);
  } else if (a.queue == nullptr) {
    front_hist_stride<NV>(a.hist, a.ld_h, a.T, a.R, a.hs, a.rowmap, a.cache, a.valid, hb, nH, red, redi);
  } else {
    front_hist_queue<NV>(a.hist, a.ld_h, a.T, a.R, a.hs, a.rowmap, a.cache, a.valid, a.queue, hb, nH, red, redi);
  }
  FM_FT_MARK(1);
}

template <int NV, int K, bool BC = false, bool RS = false>
__global__ __launch_bounds__(256) void tick_front_kernel(const FrontArgs a) {
  static_assert(BC || !RS, "the rank search belongs to the kernels with the baseline cache");
  tick_front_body<NV, K, false, BC, RS>(a, FrontDyn{});
}

template <int NV, int K, bool BC = false, bool RS = false>
__global__ __launch_bounds__(256) void tick_front_dyn_kernel(const FrontArgs a, const FrontDyn dq) {
  tick_front_body<NV, K, true, BC, RS>(a, dq);
}

// The host's plan of the pairwise role for R rows, nP requested workgroups
// (<= 0: one per 4 rows) and q_ranges requested ranges.  q == 0: static rows
// (today's kernel).  Otherwise wave w of workgroup pb ranks the s rows
// 4 pb + w + i 4 nP (i < s; together exactly [0, pool0)) and the pool
// [pool0, R) is cut into q ranges, range x = [pool0 + pool x / q,
// pool0 + pool (x + 1) / q).  s is kDynShare percent (FM_FRONT_DYN_SHARE=<percent>
// overrides, read once) of the rows a wave would get statically, rounded down
// (sweep at 80k rows, docs/PERF.md: 66 / 75 / 85 / 95 / 100 % -> 0.1318 /
// 0.1315 / 0.1306 / 0.1336 / 0.1352 ms per step).
// A wave ranks at most kRowCap rows, so the plan keeps 4 nP kRowCap >= R and,
// range by range, the rows of a range within what the lists of its workgroups
// still hold after the static share: no row can be left over; where the
// requested nP is too small for that, nP grows.
// Only the scan shape gets the queue.  A streaming launch keeps static rows
// and its grid: its pairwise workgroups (one per CU) end long before the
// history stream does, and with the queue the tick that recomputes every row
// of the 1,250-service shard measured 0.096-0.097 ms against 0.077-0.078.
struct FrontPlan {
  int nP, s, q;
  int64_t pool0;
};
static FrontPlan front_plan(int64_t R, int nP, int q_ranges, bool scan) {
  static const int share = [] {
    const char* e = getenv("FM_FRONT_DYN_SHARE");
    const int v = e != nullptr ? atoi(e) : -1;
    return v < 0 || v > 100 ? -1 : v;
  }();
  const int64_t pmax = (R + 3) / 4;
  if (nP <= 0 || nP > pmax) nP = (int)pmax;
  const int64_t per0 = R > 0 ? (R + 4 * (int64_t)nP - 1) / (4 * (int64_t)nP) : 0;
  const FrontPlan fixed{nP, (int)(per0 < 0x7fffffff ? per0 : 0x7fffffff), 0, R};
  if (!scan || q_ranges <= 0 || R <= 0 || R > 0x7fffffff) return fixed;
  if ((int64_t)nP * 4 * kRowCap < R) nP = (int)((R + 4 * kRowCap - 1) / (4 * kRowCap));
  for (;;) {
    const int64_t W = 4 * (int64_t)nP, per = R / W;
    const int s = (int)(per * (share >= 0 ? share : kDynShare) / 100);
    const int q = q_ranges < nP ? q_ranges : nP;
    const int64_t pool = R - W * s;
    // the longest range against the fewest workgroups a range can have
    if (s < kRowCap && (pool + q - 1) / q <= (int64_t)(nP / q) * 4 * (kRowCap - s)) return FrontPlan{nP, s, q, W * s};
    if (nP >= pmax) return fixed;   // (not reached: at nP = pmax s <= 1 and pool <= 4 nP, which always fits)
    const int64_t up = (int64_t)nP + nP / 2 + 1;
    nP = (int)(up < pmax ? up : pmax);
  }
}

// out[4]: static rows per wave, first row of the pool, ranges (0 = static
// rows only: the pool is empty), effective nP.  Host only: no device call.
FM_API int fm_front_plan(int64_t R, int nP, int q_ranges, int scan, int64_t* out) {
  if (out == nullptr) return (int)hipErrorInvalidValue;
  const FrontPlan p = front_plan(R, nP, q_ranges, scan != 0);
  out[0] = p.s, out[1] = p.pool0, out[2] = p.q, out[3] = p.nP;
  return 0;
}

// FM_FRONT_LDS=<bytes> (environment, read once): dynamic LDS requested per
// front-kernel workgroup, i.e. a cap on how many of them share a CU (160 KB
// of LDS: 33 KB -> at most four).  Default 33 KB: with the buffer-load history
// role the kernel fits five waves per SIMD, and a fifth concurrent workgroup
// per CU measured slower (more history streams during the pairwise phase).
static unsigned front_lds() {
  static const unsigned b = [] {
    const char* e = getenv("FM_FRONT_LDS");
    return e != nullptr ? (unsigned)atoi(e) : 33u * 1024u;
  }();
  return b;
}

// FM_RANK_SEARCH=0 (environment, read once): the launches with a baseline
// cache start the BC kernels compiled without the search form of the pooled
// ranks (fm_pairwise.h pw_rank_search), i.e. every row takes the size-128
// merge.  The switch is the kernels' template parameter RS, not a branch in
// the row; the outputs are the same words either way.
static bool rank_search() {
  static const bool on = [] {
    const char* e = getenv("FM_RANK_SEARCH");
    return e == nullptr || atoi(e) != 0;
  }();
  return on;
}

// nP / nH: workgroups of each role (0 = one pairwise workgroup per 4 rows /
// one history workgroup per row); queue: dynamic history rows (or nullptr):
// 8 x 32 + 64 zero-initialised uint32 -- the per-XCD counters and the
// XCD-balance control block (kXcdCtl; word kXcdCtl + kCtlOn = 1 enables it).
//
// cache / valid: the row-statistics cache of the history tensor (per physical
// row: float[3] and the validity word, fm_row_stats.h), or both nullptr.
// expect_miss: what the host believes about this tick -- 1: rows were written
// since the last tick (or this is the first): the launch is shaped for
// streaming, exactly as without a cache, and records every row it computes;
// 0: every row should hit: the history workgroups scan the validity words
// (computing whatever does miss), nP / nH are taken as given for that shape
// (nH 0 = one workgroup per 256 rows) and no dynamic LDS caps the pairwise
// workgroups per CU.  A wrong expectation costs time, never correctness.
//
// pqueue / q_ranges (nullptr / 0: static pairwise rows): the pairwise role's
// dynamic row queue, q_ranges x 32 zero-initialised uint32 kept zero between
// launches by the kernel itself (front_plan above; one launch at a time per
// pqueue).  The scan shape uses it: the history workgroups then have the
// lowest block ids, and nP is raised where the wave lists would not hold R
// rows.  A streaming launch keeps static rows.
//
// rowmap: history row of each logical row (fm_row_stats.h hist_row), or
// nullptr for the identity.
//
// bc_raw / bc_sorted / bc_stats (fm_tick_front_bc; all three or none; null:
// no cache, which is what fm_tick_front passes): the baseline cache of the
// pairwise role, one entry per logical row -- bc_raw [R, 64] and bc_sorted
// [R, 64] uint32, bc_stats [R, 4] uint32 (16-byte aligned), zero-initialised
// (fm_pairwise.h PwBaseCache).  Only the split layout uses it (n_cur <= 64,
// n_base <= 64 and more than 64 pooled points); every other shape leaves it
// untouched.  Each row tests its entry against the baseline it loads, on the
// device: an unchanged baseline row skips its half of the sort and its
// moments, a changed or new one computes as without a cache and rewrites
// its entry.  The host expects nothing and tracks nothing; results are the
// same bits either way.  A row's entry is read and written by the one wave
// that ranks the row, with no ordering between launches beyond the
// stream's: launches that share a cache run one at a time (the rule of
// pqueue, which the same callers already keep).
FM_API int fm_tick_front_bc(const float* hist, int64_t ld_h, int T, int64_t R, float* hs, const float* cur,
                            int64_t ld_c, int n_cur, const float* base, int64_t ld_b, int n_base, double* suff, int nP,
                            int nH, int min_mw, int min_wil, int min_kru, float* pvals, float* pstats, unsigned* queue,
                            const int* rowmap, float* cache, unsigned* valid, int expect_miss, unsigned* pqueue,
                            int q_ranges, unsigned* bc_raw, unsigned* bc_sorted, unsigned* bc_stats,
                            hipStream_t stream) {
  if (R <= 0) return 0;
  if ((((uintptr_t)bc_stats) & 15) != 0) return (int)hipErrorInvalidValue;
  // the split layout alone has a kernel with the cache (entries are indexed in 32 bits)
  const bool use_bc = bc_raw != nullptr && bc_sorted != nullptr && bc_stats != nullptr && n_cur <= 64 &&
                      n_base <= 64 && n_cur + n_base > 64 && R <= (int64_t)1 << 25;
  if (!use_bc) bc_raw = bc_sorted = bc_stats = nullptr;
  if ((ld_h & 3) != 0 || (((uintptr_t)hist) & 15) != 0) return (int)hipErrorInvalidValue;
  const int n = n_cur + n_base;
  if (base == nullptr || n_base <= 0 || n > 256) return (int)hipErrorInvalidValue;
  if (cache == nullptr || valid == nullptr || T <= 0) cache = nullptr, valid = nullptr;   // (tag 0 means invalid)
  const int scan = cache != nullptr && expect_miss == 0 ? 1 : 0;
  const FrontPlan plan = front_plan(R, nP, pqueue != nullptr ? q_ranges : 0, scan != 0);
  if (scan && nH <= 0) nH = (int)((R + 255) / 256);
  if (nH <= 0 || nH > R) nH = (int)R;
  // queue: 8 x 32 + 64 zero-initialised uints (the counters are kept zero
  // between launches by the kernel itself); needs at least one history
  // workgroup per XCD range
  if (!scan && queue != nullptr && nH < 8) nH = 8;
  const int nq = (T + 3) / 4;
  const dim3 grid((unsigned)(plan.nP + nH)), block(256);
  const unsigned lds = scan ? 0u : front_lds();
  const FrontArgs a{R, plan.nP, scan, T, hist, ld_h, hs, rowmap, cache, valid, queue, cur, ld_c, base, ld_b, suff,
                    n_cur, n_base, pvals, pstats, min_mw, min_wil, min_kru, bc_raw, bc_sorted,
                    reinterpret_cast<uint4*>(bc_stats)};
  const FrontDyn dq{pqueue, plan.q, plan.s, (int)plan.pool0};
  const int rc = row_stats_dispatch_nv(nq, [&](auto nv) {
    auto launch = [&](auto k, auto bc, auto rs) {
      constexpr int NV = decltype(nv)::value, K = decltype(k)::value;
      constexpr bool BC = decltype(bc)::value, RS = decltype(rs)::value;
      if (plan.q > 0) hipLaunchKernelGGL((tick_front_dyn_kernel<NV, K, BC, RS>), grid, block, lds, stream, a, dq);
      else hipLaunchKernelGGL((tick_front_kernel<NV, K, BC, RS>), grid, block, lds, stream, a);
    };
    if (n <= 64) launch(std::integral_constant<int, 1>{}, std::false_type{}, std::false_type{});
    else if (n > 128) launch(std::integral_constant<int, 4>{}, std::false_type{}, std::false_type{});
    else if (use_bc && rank_search()) launch(std::integral_constant<int, 2>{}, std::true_type{}, std::true_type{});
    else if (use_bc) launch(std::integral_constant<int, 2>{}, std::true_type{}, std::false_type{});
    else launch(std::integral_constant<int, 2>{}, std::false_type{}, std::false_type{});
  });
  if (rc != 0) return rc;
  FM_LAUNCH_CHECK();
  return 0;
}

// The front launch without a baseline cache: fm_tick_front_bc with null cache
// pointers, i.e. the kernels that know nothing of it.
FM_API int fm_tick_front(const float* hist, int64_t ld_h, int T, int64_t R, float* hs, const float* cur, int64_t ld_c,
                         int n_cur, const float* base, int64_t ld_b, int n_base, double* suff, int nP, int nH,
                         int min_mw, int min_wil, int min_kru, float* pvals, float* pstats, unsigned* queue,
                         const int* rowmap, float* cache, unsigned* valid, int expect_miss, unsigned* pqueue,
                         int q_ranges, hipStream_t stream) {
  return fm_tick_front_bc(hist, ld_h, T, R, hs, cur, ld_c, n_cur, base, ld_b, n_base, suff, nP, nH, min_mw, min_wil,
                          min_kru, pvals, pstats, queue, rowmap, cache, valid, expect_miss, pqueue, q_ranges, nullptr,
                          nullptr, nullptr, stream);
}

FM_API int fm_front_timing_read(unsigned long long* host, int n) {
#ifdef FM_FRONT_TIMING
  if (n > kFtMarks * 8192) n = kFtMarks * 8192;
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_front_t), (size_t)n * 8, 0, hipMemcpyDeviceToHost);
#else
  (void)host; (void)n;
  return (int)hipErrorNotSupported;
#endif
}
