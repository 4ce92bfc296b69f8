// fm-hipcc-flags: -mllvm -pragma-unroll-threshold=1000000
// (the 1024-sample pairwise sort, K = 16: past LLVM's default pragma-unroll
// size limit the stage loops stayed rolled -- runtime register indexing
// through scratch (132 B/lane) and s_set_gpr_idx; fully unrolled: 0 scratch)
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
// first and the history workgroups fill the remaining slots.
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
// its p-values (mark 2; a history workgroup leaves that slot alone).
#ifdef FM_FRONT_TIMING
constexpr int kFtMarks = 3;
__device__ unsigned long long g_front_t[kFtMarks * 8192];
#define FM_FT_MARK(k) \
  do { if (threadIdx.x == 0 && blockIdx.x < 8192) g_front_t[kFtMarks * blockIdx.x + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define FM_FT_MARK(k) do {} while (0)
#endif

#define FM_FRONT_PARAMS                                                                                        \
  const float *__restrict__ hist, int64_t ld_h, int T, int64_t R, float *__restrict__ hs /*[R,3]*/,            \
      const float *__restrict__ cur, int64_t ld_c, int n_cur, const float *__restrict__ base, int64_t ld_b,    \
      int n_base, double *__restrict__ suff, int nP, int min_mw, int min_wil, int min_kru,                     \
      float *__restrict__ pvals, float *__restrict__ pstats, unsigned *__restrict__ queue,                    \
      const int *__restrict__ rowmap, float *__restrict__ cache, unsigned *__restrict__ valid, int scan
#define FM_FRONT_ARGS hist, ld_h, T, R, hs, cur, ld_c, n_cur, base, ld_b, n_base, suff, nP, min_mw, min_wil, \
      min_kru, pvals, pstats, queue, rowmap, cache, valid, scan

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
__device__ __attribute__((noinline)) void xcd_rebalance(unsigned* ctl, int xcd, int64_t R, int64_t lo, int64_t hi) {
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

template <int NV, int K>
__device__ __forceinline__ void tick_front_body(FM_FRONT_PARAMS) {
  __shared__ double red[4];
  __shared__ int redi[4];
  FM_FT_MARK(0);
  if ((int)blockIdx.x < nP) {
    const int64_t first = (int64_t)blockIdx.x * 4, stride = (int64_t)nP * 4;
    for (int64_t row = first + wave_id(); row < R; row += stride) {
      pw_row<K>(cur + row * ld_c, base + row * ld_b, n_cur, n_base, suff + row * kSuff);
    }
    __syncthreads();   // this workgroup's suff rows are visible to all its waves
    FM_FT_MARK(2);
    // local row j -> global row first + (j & 3) + (j >> 2) * stride
    const int64_t span = R > first ? R - first : 0;
    const int nr = (int)(((span + stride - 1) / stride) * 4);
    // wave-sized chunks of (test, 64 rows); the test is wave-uniform so the
    // special-function switch stays a scalar branch (a per-lane test index
    // made the compiler keep every path live: 256 VGPRs).  Chunks are listed
    // costliest test first (Welch's incomplete beta, then the Kolmogorov
    // series, then the erfc tests) and dealt to the four waves back and forth
    // (0 1 2 3 3 2 1 0 ...), so at one chunk per test the Welch and KS chunks
    // have a wave each and the four cheap tests pair up.  Wave w of every
    // co-resident workgroup sits on the same SIMD and all of them reach this
    // phase together, so the deal is rotated by blockIdx: the Welch chains of
    // neighbouring workgroups land on different SIMDs.
    // T_T, T_KS, T_MW, T_KRU, T_WIL, T_FRI, one per nibble from the low end
    static_assert(T_T == 4 && T_KS == 3 && T_MW == 0 && T_KRU == 2 && T_WIL == 1 && T_FRI == 5, "kByCost");
    constexpr unsigned kByCost = 0x512034u;
    const int cpt = (nr + 63) >> 6;
    const int slot = (wave_id() + (int)blockIdx.x) & 3;
    for (int u = 0;; ++u) {
      const int ci = (u >> 1) * 8 + ((u & 1) ? 7 - slot : slot);
      if (ci >= N_TESTS * cpt) break;
      const int tp = ci / cpt;
      const int t = __builtin_amdgcn_readfirstlane((int)((kByCost >> (4 * tp)) & 7u));
      const int j = (ci - tp * cpt) * 64 + lane_id();
      const int64_t row = first + (j & 3) + (int64_t)(j >> 2) * stride;
      if (j < nr && row < R) {
        double pv, sv;
        eval_test_call(t, suff + row * kSuff, min_mw, min_wil, min_kru, pv, sv);
        pvals[row * N_TESTS + t] = (float)pv;
        pstats[row * N_TESTS + t] = (float)sv;
      }
    }
    FM_FT_MARK(1);
    return;
  }
  const int nH = (int)gridDim.x - nP;
  // Row-statistics cache (fm_row_stats.h).  scan: the host expects (nearly)
  // every row to hit -- the history workgroups test their rows one per
  // thread, copy the hits and reduce only the misses.  Otherwise (first tick,
  // after an invalidation, no cache) every row is taken as a miss without
  // looking: today's queue, plus the cache entry of each row it computes.
  // Either way the device decides what is computed; the host's expectation
  // only picks the shape.
  if (scan) {
    __shared__ int s_list[256];
    __shared__ int s_cnt;
    hist_scan_cached<NV>(hist, ld_h, T, R, hs, rowmap, cache, valid, (int64_t)blockIdx.x - nP, nH, red, redi, s_list,
                         &s_cnt);
    FM_FT_MARK(1);
    return;
  }
  if (queue == nullptr) {
    for (int64_t row = (int64_t)blockIdx.x - nP; row < R; row += nH) {
      float mf, sd;
      int n;
      const int64_t p = hist_row(rowmap, row);
      block_row_stats<NV>(hist + p * ld_h, T, red, redi, mf, sd, n);
      if (threadIdx.x == 0) {
        hs[row * 3 + 0] = mf;
        hs[row * 3 + 1] = sd;
        hs[row * 3 + 2] = (float)n;
        if (cache != nullptr) row_cache_put<false>(cache, valid, p, (unsigned)T, mf, sd, (float)n);
      }
    }
    FM_FT_MARK(1);
    return;
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
  __shared__ unsigned s_next;
  const int hb = (int)blockIdx.x - nP;
  const int xcd = hb & 7;
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
    for (int64_t row = r0; row < r1; ++row) {
      float mf, sd;
      int n;
      const int64_t p = hist_row(rowmap, row);
      block_row_stats<NV>(hist + p * ld_h, T, red, redi, mf, sd, n);
      if (threadIdx.x == 0) {
        hs[row * 3 + 0] = mf;
        hs[row * 3 + 1] = sd;
        hs[row * 3 + 2] = (float)n;
        if (cache != nullptr) row_cache_put<false>(cache, valid, p, (unsigned)T, mf, sd, (float)n);
      }
    }
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
      if (bal) xcd_rebalance(ctl, xcd, R, lo, hi);
    }
  }
  FM_FT_MARK(1);
}

template <int NV, int K>
__global__ __launch_bounds__(256) void tick_front_kernel(FM_FRONT_PARAMS) {
  tick_front_body<NV, K>(FM_FRONT_ARGS);
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
FM_API int fm_tick_front_cached(const float* hist, int64_t ld_h, int T, int64_t R, float* hs, const float* cur,
                                int64_t ld_c, int n_cur, const float* base, int64_t ld_b, int n_base, double* suff,
                                int nP, int nH, int min_mw, int min_wil, int min_kru, float* pvals, float* pstats,
                                unsigned* queue, const int* rowmap, float* cache, unsigned* valid, int expect_miss,
                                hipStream_t stream) {
  if (R <= 0) return 0;
  if ((ld_h & 3) != 0 || (((uintptr_t)hist) & 15) != 0) return (int)hipErrorInvalidValue;
  const int n = n_cur + n_base;
  if (base == nullptr || n_base <= 0 || n > 256) return (int)hipErrorInvalidValue;
  if (cache == nullptr || valid == nullptr || T <= 0) cache = nullptr, valid = nullptr;   // (tag 0 means invalid)
  const int scan = cache != nullptr && expect_miss == 0 ? 1 : 0;
  const int64_t pmax = (R + 3) / 4;
  if (nP <= 0 || nP > pmax) nP = (int)pmax;
  if (scan && nH <= 0) nH = (int)((R + 255) / 256);
  if (nH <= 0 || nH > R) nH = (int)R;
  // queue: 8 x 32 + 64 zero-initialised uints (the counters are kept zero
  // between launches by the kernel itself); needs at least one history
  // workgroup per XCD range
  if (!scan && queue != nullptr && nH < 8) nH = 8;
  const int nq = (T + 3) / 4;
  const dim3 grid((unsigned)(nP + nH)), block(256);
  const unsigned lds = scan ? 0u : front_lds();
#define FM_TF(KK) hipLaunchKernelGGL((tick_front_kernel<NV, KK>), grid, block, lds, stream, FM_FRONT_ARGS)
  const int rc = row_stats_dispatch_nv(nq, [&](auto nv) {
    constexpr int NV = decltype(nv)::value;
    if (n <= 64) FM_TF(1);
    else if (n <= 128) FM_TF(2);
    else FM_TF(4);
  });
#undef FM_TF
  if (rc != 0) return rc;
  FM_LAUNCH_CHECK();
  return 0;
}

FM_API int fm_tick_front_rm(const float* hist, int64_t ld_h, int T, int64_t R, float* hs, const float* cur,
                            int64_t ld_c, int n_cur, const float* base, int64_t ld_b, int n_base, double* suff, int nP,
                            int nH, int min_mw, int min_wil, int min_kru, float* pvals, float* pstats,
                            unsigned* queue, const int* rowmap, hipStream_t stream) {
  return fm_tick_front_cached(hist, ld_h, T, R, hs, cur, ld_c, n_cur, base, ld_b, n_base, suff, nP, nH, min_mw,
                              min_wil, min_kru, pvals, pstats, queue, rowmap, nullptr, nullptr, 1, stream);
}

FM_API int fm_tick_front(const float* hist, int64_t ld_h, int T, int64_t R, float* hs, const float* cur, int64_t ld_c,
                         int n_cur, const float* base, int64_t ld_b, int n_base, double* suff, int nP, int nH,
                         int min_mw, int min_wil, int min_kru, float* pvals, float* pstats, unsigned* queue,
                         hipStream_t stream) {
  return fm_tick_front_rm(hist, ld_h, T, R, hs, cur, ld_c, n_cur, base, ld_b, n_base, suff, nP, nH, min_mw, min_wil,
                          min_kru, pvals, pstats, queue, nullptr, stream);
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
