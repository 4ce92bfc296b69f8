// fm-hipcc-flags: -mllvm -pragma-unroll-threshold=1000000 -ffp-contract=off -Xclang -target-feature -Xclang -packed-fp32-ops
// (the unroll threshold as in pairwise.hip: the K = 16 bitonic network must
// unroll fully to stay in registers.  Contraction is off because the fp64
// statistics are defined as plain products, quotients and sums, each rounded
// once, as the numpy reference evaluates them; for the same contract the
// device code uses no packed fp32 instructions.)
//
// K29: the per-pod canary test (docs/BRAIN_SPEC.md 4.3): Kruskal-Wallis H over
// the baseline and the canary's pods as k + 1 groups, then Dunn's contrast of
// every pod against the baseline, Bonferroni over the k pods.  The contract is
// foremast_amd/ops/reference.py pairwise_pods / pods_verdict.
//
// cur [R, n_cur] is pod-major; seg_end [R, G] holds the column at which pod
// g's segment ends, so pod g owns [seg_end[g - 1], seg_end[g]) and columns
// past the last end belong to no pod.  NaN / +-inf are missing; a pod with
// fewer than `need` finite samples is dropped from the pooled sample.  Over
// the N pooled values (baseline = group 0, kept pods after it), exact
// integers: the doubled rank sum of every group and the tie term; from them in
// fp64, the same way in both tiers (pods_finish): H, its chi-square tail at k
// degrees of freedom, the k contrasts z_g and the largest one's p-value.
//
// A group is a tag, and what a tag collects is a bin: kPodBins words of LDS per
// row hold the groups' finite counts, kPodBins more their doubled rank sums (bin
// 0 the baseline, bin g + 1 pod g), both filled by ds_add_u32.  A doubled rank
// sum is at most 8192 * 16385 < 2^32.  The pod of a column is the number of
// segment ends at or below it: a search of the row's seg_end, staged in LDS.
// Whatever seg_end holds, a pod index lies in [0, G] and only ever picks a
// bin, and a column is read only below n_cur: no input makes an access leave
// its array.
//
// Wave tier (n_cur + n_base <= 1024): one wave per row, four rows per
// workgroup, the bins private to the wave (no barrier).  The pooled sample
// sits in registers with the group as the tag, the dropped pods' samples are
// re-tagged as missing once the counts are known, bitonic_sort<K, TAGGED> and
// avg_ranks (fm_pairwise.h) give every element its doubled rank and the tie
// term, and each element adds its rank to its group's bin.
//
// Wide tier (n_cur + n_base <= kPairwiseWideMax, any split): one 256-thread
// workgroup per row, grid-stride over rows, tag-free in K21's counting form.
// Pass 1 counts the pods' finite samples; pass 2 writes the keys of the kept
// samples into ONE LDS array (the missing key elsewhere), which
// fm_lds_sort.h sorts as a single side; pass 3 reads every sample again from
// global memory -- its group follows from its column -- and takes lt / le on
// the pooled sorted array: t = le - lt, 2 rank = 2 lt + t + 1 into the group's
// bin, t^2 - 1 into the 64-bit tie sum (sum over samples of t^2 - 1 = sum over
// runs of t^3 - t).
//
// Finish (both tiers, one wave): lane g owns pod g.  It reads n_g and rank2_g
// from the bins and evaluates z_g in fp64; H's sum is a wave_sum, the largest
// |z| a wave arg-max that prefers the lower lane on ties, lgamma(k / 2) of the
// chi-square tail a wave_sum of one log per lane; lane 0 evaluates the two
// tails and the verdict.  kPodMax is the wave width, so no pass loops over
// pods.
#include "fm_pairwise.h"
#include "fm_segments.h"

namespace {

constexpr int kPodMax = FM_WAVE;             // pods per row (POD_MAX in ops/canary.py)
constexpr int kPodWaveMax = 1024;            // pooled columns, wave tier (PAIRWISE_MAX in ops/canary.py)
constexpr int kPodBins = 68;                    // the baseline + kPodMax pods, padded to whole uint4

// One row's group bins and staged segment ends
struct PodBins {
  unsigned seg[kPodMax];
  unsigned cnt[kPodBins];
  unsigned r2[kPodBins];
};

struct PodOut {
  float* __restrict__ pods;                  // [R, 6]
  float* __restrict__ pod_z;                 // [R, G]
  int* __restrict__ pod_n;                   // [R, G]
  long long* __restrict__ pod_rank2;         // [R, G]
  long long* __restrict__ base_rank2;        // [R]
  long long* __restrict__ tie;               // [R]
  int8_t* __restrict__ pod_diff;             // [R]
};

struct PodWideShared {
  alignas(16) unsigned keys[kWideWords];
  PodBins bins;
  unsigned long long redu[1][kWideWaves];
};
// 32.9 KiB: within the plain launch limit, four workgroups per CU by LDS (three by registers: 145 VGPRs,
// profiles/pod_test_resources.txt; held to 128 the finishing pass spills)
static_assert(sizeof(PodWideShared) <= kLaunchLds && 4 * sizeof(PodWideShared) <= 160 * 1024, "LDS of a workgroup");

__device__ __forceinline__ double lane_bcast_f64(double v, int lane) {
  return __hiloint2double(lane_bcast(__double2hiint(v), lane), lane_bcast(__double2loint(v), lane));
}

// The finishing pass of a row, run by one whole wave once the bins are
// complete and visible: lane g owns pod g.
__device__ __forceinline__ void pods_finish(const PodBins* bins, int G, unsigned long long tie, int need, float p_thr,
                                            int64_t row, const PodOut& out) {
  const int lane = lane_id();
  const double NaN = __builtin_nan("");
  const int n0 = uniform((int)bins->cnt[0]);
  const unsigned r0 = uniform(bins->r2[0]);
  const int ng_raw = lane < G ? (int)bins->cnt[lane + 1] : 0;
  const bool kept = ng_raw >= need;
  const int ng = kept ? ng_raw : 0;
  const unsigned rg = kept ? bins->r2[lane + 1] : 0u;
  const int k = __popcll(__ballot(kept));
  const int N = n0 + (int)wave_sum_uniform((unsigned)ng);
  const double dN = (double)N, d0 = (double)n0, dg = (double)ng, dtie = (double)tie;
  const double C = 1.0 - dtie / (dN * dN * dN - dN);
  const bool applies = uniform((int)(k >= 2 && n0 >= need && C > 0.0)) != 0;

  double z = NaN, az = -1.0, hterm = 0.0;
  if (applies && kept) {
    const double var = dN * (dN + 1.0) / 12.0 - dtie / (12.0 * (dN - 1.0));
    z = ((double)rg / (2.0 * dg) - (double)r0 / (2.0 * d0)) / sqrt(var * (1.0 / dg + 1.0 / d0));
    az = fabs(z);
    const double half = (double)rg / 2.0;
    hterm = half * half / dg;
  }
  // arg-max of |z| over the kept pods, the lower lane on ties; every lane ends with the same pair
  int worst = kept ? lane : kPodMax + lane;
  {
    double a = az;
#define FM_POD_ARGMAX(S)                                                     \
    {                                                                        \
      const double oa = xor_lane<S>(a);                                      \
      const int ow = xor_lane<S>(worst);                                     \
      const bool take = oa > a || (oa == a && ow < worst);                   \
      a = take ? oa : a;                                                     \
      worst = take ? ow : worst;                                             \
    }
    FM_POD_ARGMAX(1) FM_POD_ARGMAX(2) FM_POD_ARGMAX(4) FM_POD_ARGMAX(8) FM_POD_ARGMAX(16) FM_POD_ARGMAX(32)
#undef FM_POD_ARGMAX
  }
  const double hsum = wave_sum(hterm);
  // lgamma(k / 2) = sum over j = 1 .. m of log(k / 2 - j) + lgamma(k / 2 - m) with m = (k - 1) / 2, which
  // leaves lgamma(1) = 0 or lgamma(1 / 2) = log(sqrt(pi)): one log per lane (k <= 64) instead of the general
  // function on lane 0, whose constants alone would take over a hundred registers
  const double gln = wave_sum(applies && lane < ((k - 1) >> 1) ? log(0.5 * (double)k - (double)(lane + 1)) : 0.0) +
                     ((k & 1) ? 0.57236494292470008707 : 0.0);
  const int wl = uniform(worst) & (FM_WAVE - 1);             // (no kept pod: any lane, unused)
  const double zw = applies ? lane_bcast_f64(z, wl) : NaN;
  worst = applies ? wl : -1;

  if (lane < G) {
    out.pod_z[row * G + lane] = (float)z;
    out.pod_n[row * G + lane] = ng;
    out.pod_rank2[row * G + lane] = (long long)rg;
  }
  if (lane == 0) {
    double H = NaN, pH = NaN, pw = NaN;
    if (applies) {
      const double h0 = (double)r0 / 2.0;
      H = (12.0 / (dN * (dN + 1.0)) * (h0 * h0 / d0 + hsum) - 3.0 * (dN + 1.0)) / C;
      pH = chi2_sf(H, (double)k, gln);
      pw = (double)k * erfc(fabs(zw) / 1.41421356237309504880);
      pw = pw > 1.0 ? 1.0 : pw;
    }
    float* o = out.pods + row * 6;
    const float pHf = (float)pH, pwf = (float)pw;
    o[0] = (float)H; o[1] = pHf; o[2] = (float)zw; o[3] = pwf; o[4] = (float)worst; o[5] = (float)k;
    out.base_rank2[row] = (long long)r0;
    out.tie[row] = (long long)tie;
    out.pod_diff[row] = (applies && pHf < p_thr && pwf < p_thr) ? 1 : 0;
  }
}

}  // namespace

template <int K>
__global__ __launch_bounds__(256) void pods_wave_kernel(const float* __restrict__ cur, int64_t ld_c, int n_cur,
                                                        const int* __restrict__ seg_end, int G,
                                                        const float* __restrict__ base, int64_t ld_b, int n_base,
                                                        int64_t R, int need, float p_thr, PodOut out) {
  __shared__ PodBins s_bins[4];
  PodBins* bins = &s_bins[wave_id()];
  const int lane = lane_id();
  const int n_pooled = n_cur + n_base;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave_id(); row < R; row += (int64_t)gridDim.x * 4) {
    const float* c = cur + row * ld_c;
    const float* b = base + row * ld_b;
    if (lane < G) bins->seg[lane] = (unsigned)seg_end[row * G + lane];
    for (int j = lane; j < kPodBins; j += FM_WAVE) { bins->cnt[j] = 0u; bins->r2[j] = 0u; }
    wave_lds_sync();
    // ---- load: the value and its group; finite counts into the bins
    float v[K];
    int tag[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = k * 64 + lane;
      float x = i < n_cur ? c[i] : (i < n_pooled ? b[i - n_cur] : kPad);
      int t = group_of(bins->seg, G, i, n_cur, n_pooled);
      if (!isfinite(x) || t < 0) { x = kPad; t = -1; }      // (a column past the last segment end is no sample)
      v[k] = x; tag[k] = t;
      if (t >= 0) atomicAdd(&bins->cnt[t], 1u);
    }
    wave_lds_sync();
    // ---- the samples of a pod below the gate are missing
    int n = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (tag[k] > 0 && (int)bins->cnt[tag[k]] < need) { v[k] = kPad; tag[k] = -1; }
      n += __popcll(__ballot(tag[k] >= 0));
    }
    bitonic_sort<K, false, true>(v, tag);
    int rk2[K];
    bool en[K];
    const int tie = avg_ranks<K, true>(v, n, rk2, en);
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (tag[k] >= 0) atomicAdd(&bins->r2[tag[k]], (unsigned)rk2[k]);
    wave_lds_sync();
    pods_finish(bins, G, (unsigned long long)(unsigned)tie, need, p_thr, row, out);
    wave_lds_sync();                                          // the bins are reused by the next row
  }
}

__global__ __launch_bounds__(kWideNT) void pods_wide_kernel(const float* __restrict__ cur, int64_t ld_c, int n_cur,
                                                            const int* __restrict__ seg_end, int G,
                                                            const float* __restrict__ base, int64_t ld_b, int n_base,
                                                            int64_t R, int need, float p_thr, PodOut out) {
  __shared__ PodWideShared sh;
  PodBins* bins = &sh.bins;
  const int tid = threadIdx.x;
  const int n_pooled = n_cur + n_base;
  const Side pooled{sh.keys, chunks_up(n_pooled), pow2_up(chunks_up(n_pooled))};
  const Side none{sh.keys + pooled.n16, 0, 0};
  for (int64_t row = blockIdx.x; row < R; row += gridDim.x) {
    const float* c = cur + row * ld_c;
    const float* b = base + row * ld_b;
    if (tid < G) bins->seg[tid] = (unsigned)seg_end[row * G + tid];
    if (tid < kPodBins) { bins->cnt[tid] = 0u; bins->r2[tid] = 0u; }
    __syncthreads();
    // ---- pass 1: finite counts per group
    for (int i = tid; i < n_pooled; i += kWideNT) {
      const float x = i < n_cur ? c[i] : b[i - n_cur];
      const int t = group_of(bins->seg, G, i, n_cur, n_pooled);
      if (t >= 0 && sample_key(x) != kMissing) atomicAdd(&bins->cnt[t], 1u);
    }
    __syncthreads();
    // ---- pass 2: the keys of the baseline and of the kept pods, sorted as one side
    int N = (int)bins->cnt[0];
    for (int g = 0; g < G; ++g) {
      const int ng = (int)bins->cnt[g + 1];
      N += ng >= need ? ng : 0;
    }
    for (int i = tid; i < pooled.n16; i += kWideNT) {
      unsigned key = kMissing;
      if (i < n_pooled) {
        const int t = group_of(bins->seg, G, i, n_cur, n_pooled);
        if (t == 0 || (t > 0 && (int)bins->cnt[t] >= need)) key = sample_key(i < n_cur ? c[i] : b[i - n_cur]);
      }
      sh.keys[i] = key;
    }
    __syncthreads();
    sort_sides(pooled, none);
    // ---- pass 3: every kept sample's doubled rank into its group's bin
    unsigned long long tie[1] = {0ull};
    for (int i = tid; i < n_pooled; i += kWideNT) {
      const int t = group_of(bins->seg, G, i, n_cur, n_pooled);
      if (t < 0 || (t > 0 && (int)bins->cnt[t] < need)) continue;
      const unsigned x = sample_key(i < n_cur ? c[i] : b[i - n_cur]);
      if (x == kMissing) continue;
      const int lt = count_lt(sh.keys, N, x), le = count_le(sh.keys, N, x);
      const int run = le - lt;
      atomicAdd(&bins->r2[t], (unsigned)(2 * lt + run + 1));
      tie[0] += (unsigned long long)((long long)run * run - 1);
    }
    block_sums(tie, sh.redu);                                 // (barriers: the bins are complete)
    if (tid < FM_WAVE) pods_finish(bins, G, tie[0], need, p_thr, row, out);
    __syncthreads();                                          // the keys and the bins are reused by the next row
  }
}

// Per row: pods [R, 6] fp32 = (H, p_H, z_worst, p_worst, worst, k), pod_z [R, G]
// fp32, pod_n [R, G] int32, pod_rank2 [R, G] int64, base_rank2 [R] int64, tie
// [R] int64, pod_diff [R] int8; every output of every row is written (NaN /
// -1 / 0 where the test does not apply).  seg_end [R, G] int32 (may be null
// with G == 0).  tier 0: the wave tier up to 1024 pooled columns, else the
// wide tier; tier 2: the wide tier.  G <= 64, n_cur + n_base <= 8192.
FM_API int fm_pairwise_pods(const float* cur, int64_t ld_c, int n_cur, const int* seg_end, int G, const float* base,
                            int64_t ld_b, int n_base, int64_t R, int min_points, float p_thr, int tier, float* pods,
                            float* pod_z, int* pod_n, long long* pod_rank2, long long* base_rank2, long long* tie,
                            int8_t* pod_diff, hipStream_t stream) {
  if (n_cur < 0 || n_base < 0 || R < 0 || G < 0 || G > kPodMax || (int64_t)n_cur + n_base > kPairwiseWideMax ||
      (tier != 0 && tier != 2))
    return (int)hipErrorInvalidValue;
  if (R == 0) return 0;
  if (pods == nullptr || base_rank2 == nullptr || tie == nullptr || pod_diff == nullptr ||
      (G > 0 && (seg_end == nullptr || pod_z == nullptr || pod_n == nullptr || pod_rank2 == nullptr)))
    return (int)hipErrorInvalidValue;
  const PodOut out{pods, pod_z, pod_n, pod_rank2, base_rank2, tie, pod_diff};
  const int need = min_points > 1 ? min_points : 1;
  const int n = n_cur + n_base;
  if (tier == 0 && n <= kPodWaveMax) {
    const dim3 grid((unsigned)((R + 3) / 4 < 0x7FFFFFFF ? (R + 3) / 4 : 0x7FFFFFFF)), block(256);
#define FM_PODS(KK)                                                                                                   \
  hipLaunchKernelGGL(pods_wave_kernel<KK>, grid, block, 0, stream, cur, ld_c, n_cur, seg_end, G, base, ld_b, n_base, \
                     R, need, p_thr, out)
    if (n <= 64) FM_PODS(1);
    else if (n <= 128) FM_PODS(2);
    else if (n <= 256) FM_PODS(4);
    else if (n <= 512) FM_PODS(8);
    else FM_PODS(16);
#undef FM_PODS
  } else {
    constexpr int64_t kMaxBlocks = 4096;     // beyond what the CUs hold at once the rows are strided
    hipLaunchKernelGGL(pods_wide_kernel, dim3((unsigned)(R < kMaxBlocks ? R : kMaxBlocks)), dim3(kWideNT), 0, stream,
                       cur, ld_c, n_cur, seg_end, G, base, ld_b, n_base, R, need, p_thr, out);
  }
  FM_LAUNCH_CHECK();
  return 0;
}
