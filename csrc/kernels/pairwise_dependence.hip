// fm-hipcc-flags: -mllvm -pragma-unroll-threshold=1000000 -ffp-contract=off -Xclang -target-feature -Xclang -packed-fp32-ops
// (pairwise_tail.hip's line, for the same reasons: the K = 16 bitonic network
// must unroll fully to stay in registers, the fp64 sums are defined op by op as
// the numpy reference evaluates them, and the device code uses no packed fp32
// instructions.)
//
// K33: the dependence gate of the pairwise verdict (docs/BRAIN_SPEC.md 4.7):
// the rank-sum z of current against baseline with each side's sample size
// deflated by a variance-inflation factor, estimated from the autocorrelation
// of the pooled midranks along time inside each pod.  The contract is
// foremast_amd/ops/reference.py pairwise_dependence / dependence_verdict.
//
// cur [R, n_cur] is pod-major with seg_end [R, G] as in K29 / K31, the samples
// of a pod in time order, one column per time step; the baseline is one
// segment.  NaN / +-inf are missing.  Over the N pooled finite values rank2 =
// 2 lt + t + 1 and a = rank2 - (N + 1), |a| <= N - 1 <= 8,191: an int16, and
// -32,768 marks a column without a sample.  a sits in LDS AT ITS COLUMN -- a
// lag is a column distance, a missing sample is a gap in time, nothing is
// compacted -- with 16 marker columns behind the row, so that a read of
// a[c + k], k <= 16, needs no bound of its own.  T = sum of a over the current
// side and A = sum of a^2 are exact integers; so are the per-segment sum of a
// and finite count n_s, in LDS bins (bin 0 the baseline, bin g + 1 pod g)
// filled by integer atomics.
//
// Once the bins are complete, a kept segment's mean goes to LDS in fp64, and
// every column gets one word beside a (col_word): its bin, and 1 + the largest
// lag at which it still opens a pair -- min(L, n_s / 4, columns left in its
// segment) -- or 0 for a column that counts nowhere (no sample, no segment, a
// segment below the gate).  The lag pass (lag_sums) then runs lag by lag, k =
// 0 .. L, lag 0 being c0: the thread that owns column c reads its word, a[c]
// and a[c + k] -- neighbouring threads read neighbouring int16, no bank
// conflict -- and adds e_c e_(c+k) in fp64 and 1 to the sums of its side.  A
// lag holds four accumulators, so the pass needs no register array; the sums
// of a lag are reduced over the wave or the workgroup and lane k - 1 keeps
// them.  (All lags in one sweep, 2 x 17 fp64 sums and their butterflies in
// registers, took over 200 VGPRs: docs/PERF.md K33.)
//
// Wave tier (n_cur + n_base <= 1024): one wave per row, four rows per
// workgroup.  The pooled row sits in registers with the column as the tag;
// bitonic_sort<K, TAGGED> and avg_ranks (fm_pairwise.h) give every value its
// rank2, and the value writes a to LDS at its tag.
//
// Workgroup tier (<= kPairwiseWideMax): one 256-thread workgroup per row in
// K21's counting form: the finite keys of the pooled row are sorted as one
// side in LDS (fm_lds_sort.h), every sample is read again from global memory
// and ranked by count_lt / count_le, and a goes to a second LDS array at its
// column (32 KiB + 16 KiB plus the bins); the sorted keys are dead after that
// and their array takes the columns' words.
//
// dep_finish (both tiers, one whole wave): lane k - 1 owns lag k of both sides
// (rho_k and its taper weight), the VIFs are wave sums, lane 0 evaluates z,
// z_adj, erfc and the verdict and does the row's stores.
//
// Whatever seg_end holds, the staged ends lie in [0, n_cur] and never decrease
// (stage_ends), a group index lies in [0, G] and only ever picks a bin, a
// column's reach is held to [0, 16], and a column is read only below the row's
// width plus the marker columns: no input makes an access leave its array.
#include "fm_pairwise.h"
#include "fm_segments.h"

namespace {

constexpr int kDepPodMax = FM_WAVE;          // pods per row (POD_MAX in ops/canary.py)
constexpr int kDepWaveMax = 1024;            // pooled columns, wave tier (PAIRWISE_MAX in ops/canary.py)
constexpr int kDepBins = 68;                 // the baseline + kDepPodMax pods, padded to whole uint4
constexpr int kDepLagMax = 16;               // lags per row, at most (ACF_MAX_LAG in ops/reference.py)
constexpr short kGap = -32768;               // a column without a sample

struct DepBins {
  unsigned seg[kDepPodMax];
  int sum[kDepBins];                         // sum of a over the group's finite samples (< 2^26)
  unsigned cnt[kDepBins];                    // n_s
  double mean[kDepBins];                     // sum / n_s of a kept segment
};

struct DepCfg {
  int L, need;
  float p_thr;
};

struct DepOut {
  float* __restrict__ dep;                   // [R, 6]
  float* __restrict__ rho;                   // [R, 2, 16]
  int* __restrict__ n;                       // [R, 2]
  long long* __restrict__ TA;                // [R, 2]
  int* __restrict__ kept;                    // [R, 2]
  int* __restrict__ pairs;                   // [R, 2, 16]
  int8_t* __restrict__ dep_keep;             // [R]
};

struct DepWideShared {
  alignas(16) unsigned keys[kWideWords];
  alignas(16) short a[kPairwiseWideMax + kDepLagMax];
  DepBins bins;
  double redd[2][kWideWaves];
  long long redl[2][kWideWaves];
  int redi[2][kWideWaves];
};
// 49.7 KiB: within the plain launch limit, three workgroups per CU by LDS
static_assert(sizeof(DepWideShared) <= kLaunchLds && 3 * sizeof(DepWideShared) <= 160 * 1024, "LDS of a workgroup");

// The row's segment ends into LDS, by one whole wave: every end clamped to
// [0, n_cur] and raised to the largest end before it, so that the staged ends
// never decrease whatever seg_end holds (an end below its predecessor's is an
// empty pod, as the definition has it) and the search of group_of is exact.
__device__ __forceinline__ void stage_ends(DepBins* bins, const int* __restrict__ ends, int G, int n_cur) {
  const int lane = lane_id();
  int e = lane < G ? ends[lane] : 0;
  e = e < 0 ? 0 : (e > n_cur ? n_cur : e);
  e = wave_incl_max(e, 0);
  if (lane < G) bins->seg[lane] = (unsigned)e;
}

// The segments' means, by the threads tid < kDepBins (the bins are complete and visible).
__device__ __forceinline__ void bin_means(DepBins* bins, int need, int tid) {
  if (tid < kDepBins) {
    const int ns = (int)bins->cnt[tid];
    bins->mean[tid] = ns >= need ? (double)bins->sum[tid] / (double)ns : 0.0;
  }
}

// The word of column i: bin << 8 | 1 + the largest lag at which the column
// opens a pair, or 0 for a column that counts nowhere.
__device__ __forceinline__ unsigned col_word(const short* a, const DepBins* bins, int G, int n_cur, int n_pooled,
                                             const DepCfg& cfg, int i) {
  const int grp = group_of(bins->seg, G, i, n_cur, n_pooled);
  if (grp < 0 || a[i] == kGap) return 0u;
  const int ns = (int)bins->cnt[grp];
  if (ns < cfg.need) return 0u;
  int end = n_pooled;
  if (grp > 0) {
    const unsigned e = bins->seg[grp - 1];
    end = (int)(e < (unsigned)n_cur ? e : (unsigned)n_cur);
  }
  int reach = cfg.L < (ns >> 2) ? cfg.L : (ns >> 2);
  reach = reach < end - 1 - i ? reach : end - 1 - i;
  reach = reach > 0 ? reach : 0;
  return (unsigned)grp << 8 | (unsigned)(reach + 1);
}

// What lane k - 1 keeps of the complete sums: C0 of both sides and its own lag
// k's c_k and pair counts.
struct DepLag {
  double C0[2], ck[2];
  int mk[2];
};

// The lag pass over the columns tid, tid + NT, ... (NT = 64: a wave, else the
// workgroup, whose every thread calls it; red: its scratch).  a, the words and
// the means are complete and visible.
template <int NT>
__device__ __forceinline__ DepLag lag_sums(const short* a, const unsigned* word, const DepBins* bins, int n_cur,
                                           int n_pooled, int L, int tid, DepWideShared* red) {
  DepLag r{{0.0, 0.0}, {0.0, 0.0}, {0, 0}};
#pragma nounroll
  for (int k = 0; k <= L; ++k) {
    double c[2] = {0.0, 0.0};
    int m[2] = {0, 0};
    for (int i = tid; i < n_pooled; i += NT) {
      const unsigned w = word[i];
      const int aj = a[i + k];                                 // (i + k < n_pooled + kDepLagMax)
      if ((int)(w & 0xFFu) <= k || aj == kGap) continue;
      const double mean = bins->mean[w >> 8];
      const double p = ((double)a[i] - mean) * ((double)aj - mean);
      if (i < n_cur) { c[0] += p; m[0] += 1; }
      else { c[1] += p; m[1] += 1; }
    }
    if constexpr (NT == FM_WAVE) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        c[s] = wave_sum(c[s]);
        m[s] = (int)wave_sum_uniform((unsigned)m[s]);
      }
    } else {
      block_sums(c, red->redd);
      block_sums(m, red->redi);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (k == 0) r.C0[s] = c[s];
      else if (lane_id() == k - 1) { r.ck[s] = c[s]; r.mk[s] = m[s]; }
    }
  }
  return r;
}

// The finishing pass of a row, run by one whole wave: lane k - 1 holds lag k of
// both sides (lag_sums), the bins are complete and visible.
__device__ __forceinline__ void dep_finish(const DepLag& lag, const DepBins* bins, int G, int n1, int n2,
                                           long long T, long long A, const DepCfg& cfg, int64_t row,
                                           const DepOut& out) {
  const int lane = lane_id();
  const int L = cfg.L;
  const int kept_c = __popcll(__ballot(lane < G && (int)bins->cnt[lane + 1] >= cfg.need));
  const int kept_b = (int)bins->cnt[0] >= cfg.need ? 1 : 0;
  double vif[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const double ck = lag.ck[s];
    const int mk = lag.mk[s];
    const double C0 = lag.C0[s];
    const double rho = (lane < L && C0 > 0.0) ? ck / C0 : 0.0;
    const double w = 1.0 - (double)(lane + 1) / ((double)L + 1.0);
    const double sum = wave_sum(lane < L ? w * rho : 0.0);
    const double cap = 0.5 * (double)(s == 0 ? n1 : n2);
    double v = 1.0 + 2.0 * sum;
    v = v > 1.0 ? v : 1.0;
    vif[s] = v < (cap > 1.0 ? cap : 1.0) ? v : (cap > 1.0 ? cap : 1.0);
    if (lane < kDepLagMax) {
      out.rho[(row * 2 + s) * kDepLagMax + lane] = (float)rho;
      out.pairs[(row * 2 + s) * kDepLagMax + lane] = mk;
    }
  }
  if (lane == 0) {
    const double NaN = __builtin_nan("");
    double z = NaN, za = NaN, p = NaN;
    const bool applies = n1 >= 2 && n2 >= 2 && A != 0;
    const double d1 = (double)n1, d2 = (double)n2, dN = (double)(n1 + n2);
    if (applies) {
      z = (double)T / sqrt(d1 * d2 / (dN * (dN - 1.0)) * (double)A);
      za = z * sqrt((1.0 / d1 + 1.0 / d2) / (vif[0] / d1 + vif[1] / d2));
      p = erfc(fabs(za) / 1.41421356237309504880);
    }
    const float pf = (float)p;
    float* o = out.dep + row * 6;
    o[0] = pf; o[1] = (float)za; o[2] = (float)z; o[3] = (float)vif[0]; o[4] = (float)vif[1]; o[5] = (float)(n1 + n2);
    out.n[row * 2] = n1;
    out.n[row * 2 + 1] = n2;
    out.TA[row * 2] = T;
    out.TA[row * 2 + 1] = A;
    out.kept[row * 2] = kept_c;
    out.kept[row * 2 + 1] = kept_b;
    out.dep_keep[row] = (!applies || pf < cfg.p_thr) ? 1 : 0;
  }
}

}  // namespace

template <int K>
__global__ __launch_bounds__(256) void dep_wave_kernel(const float* __restrict__ cur, int64_t ld_c, int n_cur,
                                                       const int* __restrict__ seg_end, int G,
                                                       const float* __restrict__ base, int64_t ld_b, int n_base,
                                                       int64_t R, DepCfg cfg, DepOut out) {
  constexpr int W = 64 * K + kDepLagMax;
  __shared__ DepBins s_bins[4];
  __shared__ unsigned s_word[4][64 * K];
  __shared__ short s_a[4][W];
  DepBins* bins = &s_bins[wave_id()];
  unsigned* word = s_word[wave_id()];
  short* a = s_a[wave_id()];
  const int lane = lane_id();
  const int n_pooled = n_cur + n_base;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave_id(); row < R; row += (int64_t)gridDim.x * 4) {
    const float* c = cur + row * ld_c;
    const float* b = base + row * ld_b;
    stage_ends(bins, seg_end + row * G, G, n_cur);
    for (int j = lane; j < kDepBins; j += FM_WAVE) { bins->sum[j] = 0; bins->cnt[j] = 0u; }
    for (int j = lane; j < W; j += FM_WAVE) a[j] = kGap;
    // ---- load: the value and its column
    float v[K];
    int tag[K];
    int n1 = 0, n2 = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = k * 64 + lane;
      float x = i < n_cur ? c[i] : (i < n_pooled ? b[i - n_cur] : kPad);
      int t = i < n_pooled ? i : -1;
      if (!isfinite(x)) { x = kPad; t = -1; }
      v[k] = x; tag[k] = t;
      n1 += __popcll(__ballot(t >= 0 && i < n_cur));
      n2 += __popcll(__ballot(t >= 0 && i >= n_cur));
    }
    const int N = n1 + n2;
    wave_lds_sync();
    // ---- ranks; a to its column, the integers, the bins
    bitonic_sort<K, false, true>(v, tag);
    int rk2[K];
    bool en[K];
    avg_ranks<K, true>(v, N, rk2, en);
    unsigned Tl = 0u, Al = 0u;                                 // (N <= 1024: sum of a^2 < 2^30)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (tag[k] >= 0) {
        const int av = rk2[k] - (N + 1);
        a[tag[k]] = (short)av;
        Tl += tag[k] < n_cur ? (unsigned)av : 0u;
        Al += (unsigned)(av * av);
        const int grp = group_of(bins->seg, G, tag[k], n_cur, n_pooled);
        if (grp >= 0) {
          atomicAdd(&bins->sum[grp], av);
          atomicAdd(&bins->cnt[grp], 1u);
        }
      }
    }
    const long long T = (long long)(int)wave_sum_uniform(Tl), A = (long long)wave_sum_uniform(Al);
    wave_lds_sync();
    // ---- the means and the columns' words, then the lag pass
    bin_means(bins, cfg.need, lane);
    bin_means(bins, cfg.need, lane + FM_WAVE);
    for (int i = lane; i < n_pooled; i += FM_WAVE) word[i] = col_word(a, bins, G, n_cur, n_pooled, cfg, i);
    wave_lds_sync();
    const DepLag lag = lag_sums<FM_WAVE>(a, word, bins, n_cur, n_pooled, cfg.L, lane, nullptr);
    dep_finish(lag, bins, G, n1, n2, T, A, cfg, row, out);
    wave_lds_sync();                                          // a, the words and the bins are reused by the next row
  }
}

__global__ __launch_bounds__(kWideNT) void dep_wide_kernel(const float* __restrict__ cur, int64_t ld_c, int n_cur,
                                                           const int* __restrict__ seg_end, int G,
                                                           const float* __restrict__ base, int64_t ld_b, int n_base,
                                                           int64_t R, DepCfg cfg, DepOut out) {
  __shared__ DepWideShared sh;
  DepBins* bins = &sh.bins;
  const int tid = threadIdx.x;
  const int n_pooled = n_cur + n_base;
  const Side pooled{sh.keys, chunks_up(n_pooled), pow2_up(chunks_up(n_pooled))};
  const Side none{sh.keys + pooled.n16, 0, 0};
  for (int64_t row = blockIdx.x; row < R; row += gridDim.x) {
    const float* c = cur + row * ld_c;
    const float* b = base + row * ld_b;
    if (tid < FM_WAVE) stage_ends(bins, seg_end + row * G, G, n_cur);
    if (tid < kDepBins) { bins->sum[tid] = 0; bins->cnt[tid] = 0u; }
    if (tid < kDepLagMax) sh.a[n_pooled + tid] = kGap;
    // ---- the finite keys of the pooled row, sorted as one side; both finite counts packed into one sum
    int packed = 0;
    for (int i = tid; i < pooled.n16; i += kWideNT) {
      unsigned key = kMissing;
      if (i < n_pooled) {
        key = sample_key(i < n_cur ? c[i] : b[i - n_cur]);
        if (key != kMissing) packed += i < n_cur ? 1 : 1 << 16;
      }
      sh.keys[i] = key;
    }
    packed = uniform(block_sum<kWideNT>(packed, sh.redi[0]));   // (barriers: keys, bins and seg visible)
    const int n1 = packed & 0xFFFF, n2 = packed >> 16, N = n1 + n2;
    sort_sides(pooled, none);
    // ---- every sample again: its rank by search, a to its column, the integers, the bins
    long long ta[2] = {0ll, 0ll};
    for (int i = tid; i < n_pooled; i += kWideNT) {
      const unsigned x = sample_key(i < n_cur ? c[i] : b[i - n_cur]);
      short av16 = kGap;
      if (x != kMissing) {
        const int lt = count_lt(sh.keys, N, x), le = count_le(sh.keys, N, x);
        const int av = 2 * lt + (le - lt) + 1 - (N + 1);
        av16 = (short)av;
        ta[0] += i < n_cur ? av : 0;
        ta[1] += (long long)av * av;
        const int grp = group_of(bins->seg, G, i, n_cur, n_pooled);
        if (grp >= 0) {
          atomicAdd(&bins->sum[grp], av);
          atomicAdd(&bins->cnt[grp], 1u);
        }
      }
      sh.a[i] = av16;
    }
    block_sums(ta, sh.redl);                                    // (barriers: a and the bins are complete, the keys dead)
    // ---- the means and the columns' words (in the keys' array), then the lag pass
    bin_means(bins, cfg.need, tid);
    for (int i = tid; i < n_pooled; i += kWideNT) sh.keys[i] = col_word(sh.a, bins, G, n_cur, n_pooled, cfg, i);
    __syncthreads();
    const DepLag lag = lag_sums<kWideNT>(sh.a, sh.keys, bins, n_cur, n_pooled, cfg.L, tid, &sh);
    if (tid < FM_WAVE) dep_finish(lag, bins, G, n1, n2, ta[0], ta[1], cfg, row, out);
    __syncthreads();                                          // the keys, a and the bins are reused by the next row
  }
}

// Per row: dep [R, 6] fp32 = (p_adj, z_adj, z, VIF_c, VIF_b, N), rho [R, 2, 16]
// fp32 and pairs [R, 2, 16] int32 (entry j: lag j + 1; 0 beyond max_lag), n
// [R, 2] int32, TA [R, 2] int64 = (T, A), kept [R, 2] int32, dep_keep [R]
// int8; every output of every row is written (NaN where the gate does not
// apply).  seg_end [R, G] int32 (may be null with G == 0).  tier 0: the wave
// tier up to 1024 pooled columns, else the wide tier; tier 2: the wide tier.
// G <= 64, n_cur + n_base <= 8192, 1 <= max_lag <= 16.
FM_API int fm_pairwise_dependence(const float* cur, int64_t ld_c, int n_cur, const int* seg_end, int G,
                                  const float* base, int64_t ld_b, int n_base, int64_t R, int max_lag, int min_points,
                                  float p_thr, int tier, float* dep, float* rho, int* n, long long* TA, int* kept,
                                  int* pairs, int8_t* dep_keep, hipStream_t stream) {
  if (n_cur < 0 || n_base < 0 || R < 0 || G < 0 || G > kDepPodMax || (int64_t)n_cur + n_base > kPairwiseWideMax ||
      (tier != 0 && tier != 2) || max_lag < 1 || max_lag > kDepLagMax)
    return (int)hipErrorInvalidValue;
  if (R == 0) return 0;
  if (dep == nullptr || rho == nullptr || n == nullptr || TA == nullptr || kept == nullptr || pairs == nullptr ||
      dep_keep == nullptr || (G > 0 && seg_end == nullptr))
    return (int)hipErrorInvalidValue;
  const DepOut out{dep, rho, n, TA, kept, pairs, dep_keep};
  const DepCfg cfg{max_lag, min_points > 1 ? min_points : 1, p_thr};
  const int np = n_cur + n_base;
  if (tier == 0 && np <= kDepWaveMax) {
    const dim3 grid((unsigned)((R + 3) / 4 < 0x7FFFFFFF ? (R + 3) / 4 : 0x7FFFFFFF)), block(256);
#define FM_DEP(KK)                                                                                                   \
  hipLaunchKernelGGL(dep_wave_kernel<KK>, grid, block, 0, stream, cur, ld_c, n_cur, seg_end, G, base, ld_b, n_base,  \
                     R, cfg, out)
    if (np <= 64) FM_DEP(1);
    else if (np <= 128) FM_DEP(2);
    else if (np <= 256) FM_DEP(4);
    else if (np <= 512) FM_DEP(8);
    else FM_DEP(16);
#undef FM_DEP
  } else {
    constexpr int64_t kMaxBlocks = 4096;     // beyond what the CUs hold at once the rows are strided
    hipLaunchKernelGGL(dep_wide_kernel, dim3((unsigned)(R < kMaxBlocks ? R : kMaxBlocks)), dim3(kWideNT), 0, stream,
                       cur, ld_c, n_cur, seg_end, G, base, ld_b, n_base, R, cfg, out);
  }
  FM_LAUNCH_CHECK();
  return 0;
}
