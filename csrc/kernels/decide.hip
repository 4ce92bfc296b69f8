// K7: the anomaly decision per service, the stand-alone service reduce and
// the compaction of anomalous points.
#include "fm_lane_fold.h"  // lane_put, max_fold, fold_metric_max
#include "fm_pairwise.h"   // N_TESTS

// ---------------------------------------------------------------------------
// Decision + pairwise combine + service reduce in ONE launch: one WAVE per
// service, looping over its M <= 16 metric rows.  All global loads of the
// service (current window, p-values) are issued before any arithmetic, so a
// wave pays one memory latency; with 4 services per workgroup a CU keeps up to
// 32 services in flight (a workgroup-per-service layout with a wave per metric
// kept only 4, and the kernel was latency-bound at ~30 us for 10k services).
// Per row: p-values fold into "distribution differs" (lanes 0..N_TESTS-1 +
// two ballots), the threshold is lowered accordingly, the current window is
// flagged against the history band (anomalous / observed counts from ballot
// popcounts), and the service verdict is reduced in registers.  Replaces
// pcombine + a per-row window-decide kernel + service_reduce.
// ---------------------------------------------------------------------------
// MAXM: metric slots in registers; EXACT: M == MAXM (no per-metric guards);
// ONE: n_cur <= 64 (the current window is one wave-wide chunk).  The
// specialised forms (EXACT and ONE, M = 8 or 4) take decide_service_lanes
// below, the generic ones the loop in the kernel.

// The specialised decision (M metrics exactly, n_cur <= 64).  Everything that
// is one value per metric lives in lane m and is computed there once for all
// metrics: the band (up, lo, inv, has_hist) from lane m's own loads, the
// "distribution differs" bit from one scalar mask.  The per-metric loop only
// broadcasts what the per-point compare needs (up, lo, inv and three
// condition bits: four readlanes), its counts and flag ballots are scalars
// written into lane m (v_writelane), and the M per-lane maxima are reduced
// together (max_fold) instead of by M butterflies.  The expressions are those
// of the generic loop, term for term: the outputs are the same bits.
template <int M>
__device__ __forceinline__ void decide_service_lanes(
    const int64_t svc, const float* __restrict__ hs, const float* __restrict__ cur, int64_t ld_c, int n_cur,
    const float* __restrict__ thr, const int* __restrict__ bound, const float* __restrict__ minlb, float pair_factor,
    const float* __restrict__ pvals, int test_mask, int combine_any, float p_thr, int min_hist,
    float* __restrict__ out_stats, unsigned long long* __restrict__ out_flags, int NW, int* __restrict__ out_count,
    float* __restrict__ out_score, int* __restrict__ out_valid, int8_t* __restrict__ out_diff,
    float* __restrict__ packed) {
  static_assert(M == 8 || M == 4, "the reduction below folds 8 or 4 registers");
  const int lane = lane_id();
  const float NaNf = __builtin_nanf("");
  // every load of the service up front (clamped, unpredicated)
  const int li = lane < n_cur ? lane : n_cur - 1;
  const int lp = lane < N_TESTS ? lane : N_TESTS - 1;
  const int lm = lane < M ? lane : M - 1;
  float xs[M], pv[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int64_t row = svc * M + m;
    xs[m] = cur[row * ld_c + li];
    pv[m] = pvals != nullptr ? pvals[row * N_TESTS + lp] : NaNf;
  }
  const float* h = hs + (svc * M + lm) * 3;
  const float mf = h[0], sd = h[1];
  const int n = (int)h[2];
  float th = thr[lm];
  const int bd = bound[lm];
  const float mlb = minlb[lm];
  // bit m: the p-values of metric m say "differs"
  unsigned dmask = 0u;
  if (pvals != nullptr) {
    const bool use = lane < N_TESTS && ((test_mask >> lane) & 1);
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const bool sel = use && !isnan(pv[m]);
      const unsigned long long app = __builtin_amdgcn_ballot_w64(sel), sig = __builtin_amdgcn_ballot_w64(sel && pv[m] < p_thr);
      const bool differs = app != 0ull && (combine_any ? sig != 0ull : sig == app);
      dmask |= (differs ? 1u : 0u) << m;
    }
  }
  // lane m: the band of metric m
  const bool differs = (dmask >> lm) & 1u;
  if (differs) th *= pair_factor;
  const float up = mf + th * sd;
  float lo = mf - th * sd;
  if (lo < mlb) lo = mlb;
  const bool has_hist = n >= min_hist && n > 0;
  const float inv = sd > 0.f ? __builtin_amdgcn_rcpf(sd) : 0.f;   // z-score scale, 1-ulp rcp
  const int cfg = (has_hist ? (bd & 3) : 0) | (sd > 0.f ? 4 : 0) | (has_hist ? 8 : 0);

  int tot = 0, mask = 0, o_cnt = 0, f_lo = 0, f_hi = 0;
  unsigned seen = 0u;   // bit m: metric m has an observed point
  bool unknown = false;
  float bestm[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const float up_m = lane_bcast(up, m), lo_m = lane_bcast(lo, m), inv_m = lane_bcast(inv, m);
    const int cfg_m = lane_bcast(cfg, m);
    const float x = xs[m];
    const bool obs = lane < n_cur && isfinite(x);
    const bool hi = (cfg_m & 1) && obs && x > up_m;
    const bool lw = (cfg_m & 2) && obs && x < lo_m;
    const bool f = hi || lw;
    const float z = (cfg_m & 4) ? (hi ? x - up_m : lo_m - x) * inv_m : 1e30f;
    bestm[m] = f && z > 0.f ? z : 0.f;
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(f);
    const int acnt = __popcll(bal);
    const bool any_obs = __builtin_amdgcn_ballot_w64(obs) != 0ull;
    o_cnt = lane_put(o_cnt, m, acnt);
    f_lo = lane_put(f_lo, m, (int)(unsigned)bal);
    f_hi = lane_put(f_hi, m, (int)(unsigned)(bal >> 32));
    seen |= (any_obs ? 1u : 0u) << m;
    tot += acnt;
    if (acnt > 0) mask |= 1 << m;
    if (!((cfg_m & 8) && any_obs)) unknown = true;
  }
  // lane m: metric m's maximum; sbest: the service's, in lane 0
  float o_score, sbest;
  fold_metric_max<M>(bestm, lane, lm, o_score, sbest);
  if (lane < M) {
    const int64_t row = svc * M + lane;
    reinterpret_cast<float4*>(out_stats)[row] = make_float4(mf, sd, up, lo);
    out_count[row] = o_cnt;
    out_valid[row] = (has_hist ? 1 : 0) | (((seen >> lane) & 1u) ? 2 : 0);
    out_score[row] = o_score;
    out_flags[row * NW] = ((unsigned long long)(unsigned)f_hi << 32) | (unsigned)f_lo;
    if (out_diff != nullptr && pvals != nullptr) out_diff[row] = (int8_t)(differs ? 1 : 0);
  }
  if (lane == 0) {
    packed[svc * 4 + 0] = (float)(tot > 0 ? 1 : (unknown ? 2 : 0));
    packed[svc * 4 + 1] = sbest;
    packed[svc * 4 + 2] = (float)mask;
    packed[svc * 4 + 3] = (float)tot;
  }
}

template <int MAXM, bool EXACT, bool ONE>
__global__ __launch_bounds__(256) void decide_service_kernel(
    const float* __restrict__ hs, const float* __restrict__ cur, int64_t ld_c, int n_cur, int64_t S, int M,
    const float* __restrict__ thr, const int* __restrict__ bound, const float* __restrict__ minlb, float pair_factor,
    const float* __restrict__ pvals, int test_mask, int combine_any, float p_thr, int min_hist,
    float* __restrict__ out_stats, unsigned long long* __restrict__ out_flags, int NW, int* __restrict__ out_count,
    float* __restrict__ out_score, int* __restrict__ out_valid, int8_t* __restrict__ out_diff,
    float* __restrict__ packed) {
  if (EXACT) M = MAXM;
  const int64_t svc = (int64_t)blockIdx.x * 4 + wave_id();
  if (svc >= S) return;
  if constexpr (EXACT && ONE && (MAXM == 8 || MAXM == 4)) {
    decide_service_lanes<MAXM>(svc, hs, cur, ld_c, n_cur, thr, bound, minlb, pair_factor, pvals, test_mask,
                               combine_any, p_thr, min_hist, out_stats, out_flags, NW, out_count, out_score,
                               out_valid, out_diff, packed);
    return;
  }
  const int lane = lane_id();
  const float NaNf = __builtin_nanf("");
  // phase 1: every load of the service up front (clamped, unpredicated)
  const int li = lane < n_cur ? lane : n_cur - 1;
  const int lp = lane < N_TESTS ? lane : N_TESTS - 1;
  float xs[MAXM], pv[MAXM];
#pragma unroll
  for (int m = 0; m < MAXM; ++m) {
    const int64_t row = svc * M + ((EXACT || m < M) ? m : M - 1);
    xs[m] = cur[row * ld_c + li];
    pv[m] = pvals != nullptr ? pvals[row * N_TESTS + lp] : NaNf;
  }
  // the service's [M, 3] history stats (3M <= 48 floats) as one vector
  // load, lane j holding element j, broadcast per metric with readlane
  const int nh = 3 * M;
  const float hsv = hs[svc * nh + (lane < nh ? lane : nh - 1)];
  int tot = 0, mask = 0;
  bool unknown = false;
  float bestm[MAXM];
  // per-row outputs are collected in lane m (values are wave-uniform per
  // metric) and stored once by lanes 0..M-1: 7 store instructions per
  // service instead of 7 per metric from lane 0
  float4 o_st = make_float4(0.f, 0.f, 0.f, 0.f);
  int o_cnt = 0, o_valid = 0, o_diff = 0;
  unsigned long long o_flag = 0ull;
#pragma unroll
  for (int m = 0; m < MAXM; ++m) {
    bestm[m] = 0.f;
    if (!EXACT && m >= M) continue;
    const int64_t row = svc * M + m;
    bool differs = false;
    if (pvals != nullptr) {
      const bool sel = lane < N_TESTS && ((test_mask >> lane) & 1) && !isnan(pv[m]);
      const unsigned long long app = __ballot(sel), sig = __ballot(sel && pv[m] < p_thr);
      differs = app != 0ull && (combine_any ? sig != 0ull : sig == app);
    }
    const float mf = lane_bcast(hsv, 3 * m);
    const float sd = lane_bcast(hsv, 3 * m + 1);
    const int n = (int)lane_bcast(hsv, 3 * m + 2);
    float th = thr[m];
    if (differs) th *= pair_factor;
    const int bd = bound[m];
    const float up = mf + th * sd;
    float lo = mf - th * sd;
    if (lo < minlb[m]) lo = minlb[m];
    const bool has_hist = n >= min_hist && n > 0;
    const float inv = sd > 0.f ? __builtin_amdgcn_rcpf(sd) : 0.f;   // z-score scale, 1-ulp rcp
    int acnt = 0, ccnt = 0;
    float best = 0.f;
    for (int i0 = 0; i0 < (ONE ? 64 : n_cur); i0 += 64) {
      const int i = i0 + lane;
      const float x = (ONE || i0 == 0) ? xs[m] : cur[row * ld_c + (i < n_cur ? i : n_cur - 1)];
      const bool obs = i < n_cur && isfinite(x);
      const bool hi = has_hist && obs && (bd & 1) && x > up;
      const bool lw = has_hist && obs && (bd & 2) && x < lo;
      const bool f = hi || lw;
      const float z = sd > 0.f ? (hi ? x - up : lo - x) * inv : 1e30f;
      best = f && z > best ? z : best;
      const unsigned long long bal = __ballot(f);
      acnt += __popcll(bal);
      ccnt += __popcll(__ballot(obs));
      if (i0 == 0) {
        if (lane == m) o_flag = bal;
      } else if (lane == 0 && i0 / 64 < NW) {
        out_flags[row * NW + i0 / 64] = bal;
      }
    }
    bestm[m] = best;
    const int valid = (has_hist ? 1 : 0) | (ccnt > 0 ? 2 : 0);
    if (lane == m) {
      o_st = make_float4(mf, sd, up, lo);
      o_cnt = acnt;
      o_valid = valid;
      o_diff = differs ? 1 : 0;
    }
    tot += acnt;
    if (acnt > 0) mask |= 1 << m;
    if ((valid & 3) != 3) unknown = true;
  }
  // the M max-reductions are independent: issued together they overlap
  float sbest = 0.f, o_score = 0.f;
#pragma unroll
  for (int m = 0; m < MAXM; ++m) bestm[m] = wave_max(bestm[m]);
#pragma unroll
  for (int m = 0; m < MAXM; ++m) {
    if (!EXACT && m >= M) break;
    if (lane == m) o_score = bestm[m];
    sbest = bestm[m] > sbest ? bestm[m] : sbest;
  }
  if (lane < M) {
    const int64_t row = svc * M + lane;
    reinterpret_cast<float4*>(out_stats)[row] = o_st;
    out_count[row] = o_cnt;
    out_valid[row] = o_valid;
    out_score[row] = o_score;
    out_flags[row * NW] = o_flag;
    if (out_diff != nullptr && pvals != nullptr) out_diff[row] = (int8_t)o_diff;
  }
  if (lane == 0) {
    packed[svc * 4 + 0] = (float)(tot > 0 ? 1 : (unknown ? 2 : 0));
    packed[svc * 4 + 1] = sbest;
    packed[svc * 4 + 2] = (float)mask;
    packed[svc * 4 + 3] = (float)tot;
  }
}

FM_API int fm_decide_services(const float* hs, const float* cur, int64_t ld_c, int n_cur, int64_t S, int M,
                              const float* thr, const int* bound, const float* minlb, float pair_factor,
                              const float* pvals, int test_mask, int combine_any, float p_thr, int min_hist,
                              float* out_stats, unsigned long long* out_flags, int NW, int* out_count,
                              float* out_score, int* out_valid, int8_t* out_diff, float* packed,
                              hipStream_t stream) {
  if (S <= 0) return 0;
  if (M < 1 || M > 16 || n_cur < 1 || NW * 64 < n_cur) return (int)hipErrorInvalidValue;
  if ((((uintptr_t)out_stats) & 15) != 0) return (int)hipErrorInvalidValue;   // float4 row stores
  const dim3 grid((unsigned)((S + 3) / 4)), block(256);
#define FM_DS(MM, EX, ONE)                                                                                            \
  hipLaunchKernelGGL((decide_service_kernel<MM, EX, ONE>), grid, block, 0, stream, hs, cur, ld_c, n_cur, S, M, thr,    \
                     bound, minlb, pair_factor, pvals, test_mask, combine_any, p_thr, min_hist, out_stats, out_flags,  \
                     NW, out_count, out_score, out_valid, out_diff, packed)
  if (M == 8 && n_cur <= 64) FM_DS(8, true, true);
  else if (M == 4 && n_cur <= 64) FM_DS(4, true, true);
  else if (M <= 8) FM_DS(8, false, false);
  else FM_DS(16, false, false);
#undef FM_DS
  FM_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// Service reduce: per service, fold its M metric rows into the packed result
// row [status, score, anomalous-metric mask, anomalous point count] that is
// all-gathered across ranks.  status: 0 = no anomaly, 1 = anomaly, 2 = unknown
// (missing current data or not enough history).
// ---------------------------------------------------------------------------
__global__ void service_reduce_kernel(const int* __restrict__ count, const float* __restrict__ score,
                                      const int* __restrict__ valid, int64_t S, int M, float* __restrict__ packed) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  int tot = 0, mask = 0;
  bool unknown = false;
  float best = 0.f;
  for (int m = 0; m < M; ++m) {
    const int64_t r = s * M + m;
    const int c = count[r];
    tot += c;
    if (c > 0) mask |= 1 << m;
    if ((valid[r] & 3) != 3) unknown = true;
    best = score[r] > best ? score[r] : best;
  }
  const int status = tot > 0 ? 1 : (unknown ? 2 : 0);
  packed[s * 4 + 0] = (float)status;
  packed[s * 4 + 1] = best;
  packed[s * 4 + 2] = (float)mask;
  packed[s * 4 + 3] = (float)tot;
}

FM_API int fm_service_reduce(const int* count, const float* score, const int* valid, int64_t S, int M, float* packed,
                             hipStream_t stream) {
  if (S <= 0) return 0;
  if (M > 24) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(service_reduce_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, stream, count, score,
                     valid, S, M, packed);
  FM_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// Stream compaction of anomalous points: one wave per row, entries
// (row, index, value) appended through one atomic per row with anomalies.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void compact_kernel(const unsigned long long* __restrict__ flags, int NW,
                                                      const float* __restrict__ cur, int64_t ld_c, int n_cur,
                                                      const int* __restrict__ count, int64_t R, int cap,
                                                      int* __restrict__ counter, int* __restrict__ out_idx,
                                                      float* __restrict__ out_val) {
  const int64_t row = (int64_t)blockIdx.x * 4 + wave_id();
  if (row >= R) return;
  const int c = count[row];
  if (c == 0) return;
  const int lane = lane_id();
  int base = 0;
  if (lane == 0) base = atomicAdd(counter, c);
  base = __shfl(base, 0);
  int written = 0;
  for (int w = 0; w < NW; ++w) {
    const unsigned long long word = flags[row * NW + w];
    if (!word) continue;
    const bool mine = (word >> lane) & 1ull;
    const unsigned long long below = lane == 0 ? 0ull : (word & ((1ull << lane) - 1ull));
    const int pos = written + __popcll(below);
    if (mine) {
      const int slot = base + pos;
      const int i = w * 64 + lane;
      if (slot < cap) {
        out_idx[2 * slot + 0] = (int)row;
        out_idx[2 * slot + 1] = i;
        out_val[slot] = cur[row * ld_c + i];
      }
    }
    written += __popcll(word);
  }
}

FM_API int fm_compact_anomalies(const unsigned long long* flags, int NW, const float* cur, int64_t ld_c, int n_cur,
                                const int* count, int64_t R, int cap, int* counter, int* out_idx, float* out_val,
                                hipStream_t stream) {
  if (R <= 0) return 0;
  hipLaunchKernelGGL(compact_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, stream, flags, NW, cur, ld_c, n_cur,
                     count, R, cap, counter, out_idx, out_val);
  FM_LAUNCH_CHECK();
  return 0;
}
