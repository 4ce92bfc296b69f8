// The service decision over band records: fm_decide_services (decide.hip)
// with bs [R,4] = (centre, sigma_lo, sigma_up, n) in place of hs [R,3], for
// the static band models' resident tick (K25, band_stats.hip).  One wave per
// service and every load up front, as there: the p-value combine, the pairwise
// threshold factor, the history gate, the min_lower_bound clamp, flags,
// counts, score, valid, out_diff and the packed service row.  Per side:
// up = c + th * sigma_up, lo = c - th * sigma_lo (clamped); a point above up
// scores (x - up) * rcp(sigma_up), one below lo (lo - x) * rcp(sigma_lo), 1e30
// where that side's sigma is not positive.  The expressions of a side are
// decide_service_kernel's, term for term, and the file is built with its
// flags: a row with sigma_lo == sigma_up comes out as fm_decide_services makes
// it, bit for bit.  out_stats [R,4] = (centre, sigma_up, up, lo).
// LANES (M == MAXM == 8 or 4 and n_cur <= 64) is decide_service_lanes' form,
// everything per metric in lane m; the others take the generic loop.
#include "fm_lane_fold.h"  // lane_put, fold_metric_max
#include "fm_pairwise.h"   // N_TESTS

// decide_service_lanes (decide.hip) over band records: lane m loads its
// metric's record as one float4 and keeps a reciprocal and a "sigma > 0" bit
// per side; the per-metric loop broadcasts one value more.  The expressions
// are the generic loop's, term for term.
template <int M>
__device__ __forceinline__ void decide_service_lanes_2s(
    const int64_t svc, const float* __restrict__ bs, const float* __restrict__ cur, int64_t ld_c, int n_cur,
    const float* __restrict__ thr, const int* __restrict__ bound, const float* __restrict__ minlb, float pair_factor,
    const float* __restrict__ pvals, int test_mask, int combine_any, float p_thr, int min_hist,
    float* __restrict__ out_stats, unsigned long long* __restrict__ out_flags, int NW, int* __restrict__ out_count,
    float* __restrict__ out_score, int* __restrict__ out_valid, int8_t* __restrict__ out_diff,
    float* __restrict__ packed) {
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
  const float4 b = reinterpret_cast<const float4*>(bs)[svc * M + lm];
  const float mf = b.x, sd_lo = b.y, sd_up = b.z;
  const int n = (int)b.w;
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
  const float up = mf + th * sd_up;
  float lo = mf - th * sd_lo;
  if (lo < mlb) lo = mlb;
  const bool has_hist = n >= min_hist && n > 0;
  const float inv_up = sd_up > 0.f ? __builtin_amdgcn_rcpf(sd_up) : 0.f;   // z-score scale, 1-ulp rcp
  const float inv_lo = sd_lo > 0.f ? __builtin_amdgcn_rcpf(sd_lo) : 0.f;
  const int cfg = (has_hist ? (bd & 3) : 0) | (sd_up > 0.f ? 4 : 0) | (has_hist ? 8 : 0) | (sd_lo > 0.f ? 16 : 0);

  int tot = 0, mask = 0, o_cnt = 0, f_lo = 0, f_hi = 0;
  unsigned seen = 0u;   // bit m: metric m has an observed point
  bool unknown = false;
  float bestm[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const float up_m = lane_bcast(up, m), lo_m = lane_bcast(lo, m);
    const float inv_up_m = lane_bcast(inv_up, m), inv_lo_m = lane_bcast(inv_lo, m);
    const int cfg_m = lane_bcast(cfg, m);
    const float x = xs[m];
    const bool obs = lane < n_cur && isfinite(x);
    const bool hi = (cfg_m & 1) && obs && x > up_m;
    const bool lw = (cfg_m & 2) && obs && x < lo_m;
    const bool f = hi || lw;
    const float z = hi ? ((cfg_m & 4) ? (x - up_m) * inv_up_m : 1e30f) : ((cfg_m & 16) ? (lo_m - x) * inv_lo_m : 1e30f);
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
    reinterpret_cast<float4*>(out_stats)[row] = make_float4(mf, sd_up, up, lo);
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

template <int MAXM, bool LANES>
__global__ __launch_bounds__(256) void decide_service_2s_kernel(
    const float* __restrict__ bs, const float* __restrict__ cur, int64_t ld_c, int n_cur, int64_t S, int M,
    const float* __restrict__ thr, const int* __restrict__ bound, const float* __restrict__ minlb, float pair_factor,
    const float* __restrict__ pvals, int test_mask, int combine_any, float p_thr, int min_hist,
    float* __restrict__ out_stats, unsigned long long* __restrict__ out_flags, int NW, int* __restrict__ out_count,
    float* __restrict__ out_score, int* __restrict__ out_valid, int8_t* __restrict__ out_diff,
    float* __restrict__ packed) {
  const int64_t svc = (int64_t)blockIdx.x * 4 + wave_id();
  if (svc >= S) return;
  if constexpr (LANES) {
    decide_service_lanes_2s<MAXM>(svc, bs, cur, ld_c, n_cur, thr, bound, minlb, pair_factor, pvals, test_mask,
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
    const int64_t row = svc * M + (m < M ? m : M - 1);
    xs[m] = cur[row * ld_c + li];
    pv[m] = pvals != nullptr ? pvals[row * N_TESTS + lp] : NaNf;
  }
  // the service's [M, 4] band records (4M <= 64 floats) as one vector load,
  // lane j holding element j, broadcast per metric with readlane
  const int nh = 4 * M;
  const float bsv = bs[svc * nh + (lane < nh ? lane : nh - 1)];
  int tot = 0, mask = 0;
  bool unknown = false;
  float bestm[MAXM];
  // per-row outputs are collected in lane m (values are wave-uniform per
  // metric) and stored once by lanes 0..M-1
  float4 o_st = make_float4(0.f, 0.f, 0.f, 0.f);
  int o_cnt = 0, o_valid = 0, o_diff = 0;
  unsigned long long o_flag = 0ull;
#pragma unroll
  for (int m = 0; m < MAXM; ++m) {
    bestm[m] = 0.f;
    if (m >= M) continue;
    const int64_t row = svc * M + m;
    bool differs = false;
    if (pvals != nullptr) {
      const bool sel = lane < N_TESTS && ((test_mask >> lane) & 1) && !isnan(pv[m]);
      const unsigned long long app = __ballot(sel), sig = __ballot(sel && pv[m] < p_thr);
      differs = app != 0ull && (combine_any ? sig != 0ull : sig == app);
    }
    const float mf = lane_bcast(bsv, 4 * m);
    const float sd_lo = lane_bcast(bsv, 4 * m + 1);
    const float sd_up = lane_bcast(bsv, 4 * m + 2);
    const int n = (int)lane_bcast(bsv, 4 * m + 3);
    float th = thr[m];
    if (differs) th *= pair_factor;
    const int bd = bound[m];
    const float up = mf + th * sd_up;
    float lo = mf - th * sd_lo;
    if (lo < minlb[m]) lo = minlb[m];
    const bool has_hist = n >= min_hist && n > 0;
    const float inv_up = sd_up > 0.f ? __builtin_amdgcn_rcpf(sd_up) : 0.f;   // z-score scale, 1-ulp rcp
    const float inv_lo = sd_lo > 0.f ? __builtin_amdgcn_rcpf(sd_lo) : 0.f;
    int acnt = 0, ccnt = 0;
    float best = 0.f;
    for (int i0 = 0; i0 < n_cur; i0 += 64) {
      const int i = i0 + lane;
      const float x = i0 == 0 ? xs[m] : cur[row * ld_c + (i < n_cur ? i : n_cur - 1)];
      const bool obs = i < n_cur && isfinite(x);
      const bool hi = has_hist && obs && (bd & 1) && x > up;
      const bool lw = has_hist && obs && (bd & 2) && x < lo;
      const bool f = hi || lw;
      const float z = hi ? (sd_up > 0.f ? (x - up) * inv_up : 1e30f) : (sd_lo > 0.f ? (lo - x) * inv_lo : 1e30f);
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
      o_st = make_float4(mf, sd_up, up, lo);
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
    if (m >= M) break;
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

// fm_decide_services' arguments with bs [R,4] band records for hs [R,3].
FM_API int fm_decide_services_2s(const float* bs, const float* cur, int64_t ld_c, int n_cur, int64_t S, int M,
                                 const float* thr, const int* bound, const float* minlb, float pair_factor,
                                 const float* pvals, int test_mask, int combine_any, float p_thr, int min_hist,
                                 float* out_stats, unsigned long long* out_flags, int NW, int* out_count,
                                 float* out_score, int* out_valid, int8_t* out_diff, float* packed,
                                 hipStream_t stream) {
  if (S <= 0) return 0;
  if (M < 1 || M > 16 || n_cur < 1 || NW * 64 < n_cur) return (int)hipErrorInvalidValue;
  if (((((uintptr_t)out_stats) | ((uintptr_t)bs)) & 15) != 0) return (int)hipErrorInvalidValue;   // float4 rows
  const dim3 grid((unsigned)((S + 3) / 4)), block(256);
#define FM_DS2(MM, LANES)                                                                                             \
  hipLaunchKernelGGL((decide_service_2s_kernel<MM, LANES>), grid, block, 0, stream, bs, cur, ld_c, n_cur, S, M, thr,   \
                     bound, minlb, pair_factor, pvals, test_mask, combine_any, p_thr, min_hist, out_stats, out_flags,  \
                     NW, out_count, out_score, out_valid, out_diff, packed)
  if (M == 8 && n_cur <= 64) FM_DS2(8, true);
  else if (M == 4 && n_cur <= 64) FM_DS2(4, true);
  else if (M <= 8) FM_DS2(8, false);
  else FM_DS2(16, false);
#undef FM_DS2
  FM_LAUNCH_CHECK();
  return 0;
}
