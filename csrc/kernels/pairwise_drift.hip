// fm-hipcc-flags: -ffp-contract=off -Xclang -target-feature -Xclang -packed-fp32-ops
// (contraction is off because the fp64 statistics are defined as plain
// products, quotients and sums, each rounded once, as the numpy reference
// evaluates them; for the same contract the device code uses no packed fp32
// instructions.)
//
// K31: the drift canary test (docs/BRAIN_SPEC.md 4.5): a stratified
// Mann-Kendall trend test of the canary's pods against the baseline's own
// trend.  The contract is foremast_amd/ops/reference.py pairwise_drift /
// drift_verdict.
//
// cur [R, n_cur] is pod-major with seg_end [R, G] as in K29; the baseline is
// one segment.  NaN / +-inf are missing, the rest keep their column order as
// time.  Per segment, over its finite samples x_1..x_n, with g_j / l_j / c_j
// the earlier samples of the segment below / above / equal to x_j: S = sum
// g_j - l_j, n, sum c_j and sum c_j^2; from them per side the exact integers
// S, P, Tx2, V18 and, in fp64, z and tau (drift_finish).  No sort, no ranks:
// the kernel counts pairs.
//
// The pooled row goes to LDS once with every missing sample, and every column
// of no segment, turned into NaN: an ordered IEEE compare with a NaN is false,
// so missing samples drop out of every count, and -0.0 == 0.0.  Beside it
// sits, per tile of 64 columns, the ballot of its finite columns and their
// running count, from which the number of finite columns below any column
// follows in two reads (finite_below); c_j is that number over the segment's
// earlier columns less g_j and l_j, so the pair loop keeps two counters.
//
// The pair loop (pair_tile): a lane holds K samples x_j in registers, register
// k of lane l the column j0 + 64 k + l.  A tile of 64 earlier columns is read
// from LDS four at a time at an address all lanes share (a broadcast), and
// every word read meets all K registers: two compares and two add-with-carry
// per pair.  Once per tile every register gets one of three wave-uniform
// modes: skip (no finite lane's segment reaches into the tile, or no column
// of the register lies after it), full (every finite lane's segment covers
// the tile and the register lies wholly after it: no predicate) or cut (the
// diagonal and the tiles a segment edge falls into: lo_j <= i < j per pair).
//
// Wave tier (n_cur + n_base <= 1024): one wave per row, four rows per
// workgroup, K = the row's tiles, j0 = 0: the tiles before a register's own
// are full or skipped, its own is the diagonal.
//
// Wide tier (<= kPairwiseWideMax): one 512-thread workgroup per row.  The row
// is cut into at most 32 blocks of 64 K columns (K = 1, 2, 4 by the row's
// width).  A block is owned by one wave from its segment's first tile to its
// own, because c_j enters squared and must be whole in one lane.  The blocks'
// pair counts differ (the pair matrix is block-triangular per segment), so
// every wave ranks the blocks by the columns they have to meet and takes them
// in boustrophedon order of that rank (0..7, 7..0, ...): the waves' pair
// counts balance whether the row is one long pod or many short ones.
//
// Both tiers add S_j, c_j and c_j^2 into per-segment LDS bins (bin 0 the
// baseline, bin g + 1 pod g) by integer LDS atomics; drift_finish, one wave,
// lane g owning pod g (so G <= 64), forms the integers, the statistics, the
// verdict and all stores.  Whatever seg_end holds, a segment index lies in
// [0, G] and only ever picks a bin, and a column is read only below the row's
// width: no input makes an access leave its array.
#include "fm_segments.h"

using namespace fm;

namespace {

constexpr int kDriftPodMax = FM_WAVE;        // pods per row (POD_MAX in ops/canary.py)
constexpr int kDriftWaveMax = 1024;          // pooled columns, wave tier (PAIRWISE_MAX in ops/canary.py)
constexpr int kDriftBins = 68;               // the baseline + kDriftPodMax pods, padded to whole uint4
constexpr int kDriftNT = 512;                // threads of a wide-tier workgroup
constexpr int kDriftWaves = kDriftNT / FM_WAVE;
constexpr int kDriftBlocks = 32;             // blocks a wide row is cut into, at most
constexpr int kTile = FM_WAVE;

struct DriftBins {
  unsigned seg[kDriftPodMax];
  int S[kDriftBins];
  unsigned c1[kDriftBins];
  unsigned long long c2[kDriftBins];
};

// A pooled row in LDS: the samples (NaN = no sample), per tile the ballot of
// the finite columns and the count of finite columns before the tile; entry
// [tiles] closes the row (no column, the row's total).
template <int TILES>
struct DriftRow {
  alignas(16) float x[TILES * kTile];
  unsigned long long fin[TILES + 1];
  unsigned pre[TILES + 1];
};

struct DriftOut {
  float* __restrict__ drift;                 // [R, 6]
  long long* __restrict__ counts;            // [R, 2, 4]
  int* __restrict__ pod_S;                   // [R, G]
  int* __restrict__ pod_n;                   // [R, G]
  int* __restrict__ k;                       // [R]
  int8_t* __restrict__ drift_diff;           // [R]
};

struct DriftWideShared {
  DriftRow<kPairwiseWideMax / kTile> row;
  DriftBins bins;
};
static_assert(sizeof(DriftWideShared) <= kLaunchLds && 4 * sizeof(DriftWideShared) <= 160 * 1024, "LDS of a workgroup");

// finite columns of the row below column p (p <= 64 tiles)
__device__ __forceinline__ int finite_below(const unsigned long long* fin, const unsigned* pre, int p) {
  return (int)pre[p >> 6] + __popcll(fin[p >> 6] & ((1ull << (p & 63)) - 1ull));
}

// Tiles wave, wave + NW, ... of the row into LDS.
template <int NW>
__device__ __forceinline__ void load_tiles(float* x, unsigned long long* fin, unsigned* pre, const unsigned* seg, int G,
                                           const float* __restrict__ c, const float* __restrict__ b, int n_cur,
                                           int n_pooled, int tiles, int wave) {
  const int lane = lane_id();
  for (int t = wave; t < tiles; t += NW) {
    const int i = t * kTile + lane;
    const float v = i < n_cur ? c[i] : (i < n_pooled ? b[i - n_cur] : 0.f);
    const bool ok = group_of(seg, G, i, n_cur, n_pooled) >= 0 && fabsf(v) < __builtin_inff();
    x[i] = ok ? v : __builtin_nanf("");
    const unsigned long long m = __ballot(ok);
    if (lane == 0) { fin[t] = m; pre[t] = (unsigned)__popcll(m); }
  }
}

// pre[] from per-tile counts to counts before the tile, by one wave; closes the row.
__device__ __forceinline__ void scan_tiles(unsigned long long* fin, unsigned* pre, int tiles) {
  const int lane = lane_id();
  unsigned carry = 0;
  for (int t0 = 0; t0 <= tiles; t0 += FM_WAVE) {
    const int t = t0 + lane;
    const unsigned v = t < tiles ? pre[t] : 0u;
    const unsigned inc = wave_incl_sum(v);
    if (t <= tiles) pre[t] = carry + inc - v;
    carry += lane_bcast(inc, FM_WAVE - 1);
  }
  if (lane == 0) fin[tiles] = 0ull;
}

// The columns [i0, i0 + 64) of the row against the K registers of every lane:
// register k holds the sample of column j0 + 64 k + lane, whose segment starts
// at lo[k]; gt / lt count the earlier columns of the segment below / above it.
template <int K>
__device__ __forceinline__ void pair_tile(const float* xs, int i0, int j0, const float (&x)[K], const int (&lo)[K],
                                          int (&gt)[K], int (&lt)[K]) {
  const int lane = lane_id();
  unsigned full = 0u, cut = 0u;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int jk = j0 + k * kTile;
    if (jk + kTile - 1 <= i0) continue;                       // no column of the register lies after the tile's first
    const bool fin = x[k] == x[k];
    if (__ballot(fin && lo[k] < i0 + kTile) == 0ull) continue;  // no segment reaches into the tile
    if (jk >= i0 + kTile && __ballot(fin && lo[k] > i0) == 0ull) full |= 1u << k;
    else cut |= 1u << k;
  }
  if ((full | cut) == 0u) return;
  const float4* x4 = reinterpret_cast<const float4*>(xs + i0);
  for (int q = 0; q < kTile / 4; ++q) {
    const float4 v = x4[q];                                   // (one address for the wave: a broadcast)
    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (full >> k & 1u) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          gt[k] += e[u] < x[k];
          lt[k] += e[u] > x[k];
        }
      } else if (cut >> k & 1u) {
        const unsigned span = (unsigned)(j0 + k * kTile + lane - lo[k]);   // lo <= i < j as one unsigned compare
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float ev = (unsigned)(i0 + 4 * q + u - lo[k]) < span ? e[u] : __builtin_nanf("");
          gt[k] += ev < x[k];
          lt[k] += ev > x[k];
        }
      }
    }
  }
}

// The K registers of a lane from the row in LDS (tiles past the row's: NaN).
template <int K>
__device__ __forceinline__ void load_block(const float* xs, const unsigned* seg, int G, int n_cur, int n_pooled,
                                           int tiles, int j0, float (&x)[K], int (&lo)[K], int (&grp)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int j = j0 + k * kTile + lane_id();
    x[k] = j < tiles * kTile ? xs[j] : __builtin_nanf("");
    grp[k] = segment_of(seg, G, j, n_cur, n_pooled, lo[k]);
  }
}

// S_j, c_j and c_j^2 of the lane's finite samples into their segments' bins.
template <int K>
__device__ __forceinline__ void bin_block(DriftBins* bins, const unsigned long long* fin, const unsigned* pre, int j0,
                                          const float (&x)[K], const int (&lo)[K], const int (&grp)[K],
                                          const int (&gt)[K], const int (&lt)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (!(x[k] == x[k])) continue;                            // (a finite sample has a group)
    const int j = j0 + k * kTile + lane_id();
    const unsigned c = (unsigned)(finite_below(fin, pre, j) - finite_below(fin, pre, lo[k]) - gt[k] - lt[k]);
    atomicAdd(&bins->S[grp[k]], gt[k] - lt[k]);
    if (c) {
      atomicAdd(&bins->c1[grp[k]], c);
      atomicAdd(&bins->c2[grp[k]], (unsigned long long)c * c);
    }
  }
}

// z and tau of one side from its integers (V18 > 0)
__device__ __forceinline__ void side_stats(long long S, long long P, long long T2, long long V, double& z, double& tau) {
  z = tau = 0.0;
  if (V > 0) {
    const long long sg = (S > 0) - (S < 0);
    z = (double)(S - sg) / sqrt((double)V / 18.0);
    tau = (double)S / sqrt((double)P * ((double)P - (double)T2 / 2.0));
  }
}

// The finishing pass of a row, run by one whole wave once the bins are
// complete and visible: lane g owns pod g.
__device__ __forceinline__ void drift_finish(const DriftBins* bins, const unsigned long long* fin, const unsigned* pre,
                                             int G, int n_cur, int n_pooled, int need, float p_thr, float min_tau,
                                             int64_t row, const DriftOut& out) {
  const int lane = lane_id();
  const unsigned ucur = (unsigned)n_cur;
  unsigned lo = lane > 0 && lane < G ? bins->seg[lane - 1] : 0u, hi = lane < G ? bins->seg[lane] : 0u;
  lo = lo < ucur ? lo : ucur;
  hi = hi < ucur ? hi : ucur;
  hi = hi > lo ? hi : lo;
  const int n_raw = lane < G ? finite_below(fin, pre, (int)hi) - finite_below(fin, pre, (int)lo) : 0;
  const bool kept = n_raw >= need;
  const int k = __popcll(__ballot(kept));
  // the integers of segment `bin` with n finite samples
  auto ints = [&](int bin, long long n, long long (&v)[4]) {
    const long long c1 = (long long)bins->c1[bin], c2 = (long long)bins->c2[bin];
    v[0] = (long long)bins->S[bin];
    v[1] = n * (n - 1) / 2;
    v[2] = 2 * c1;
    v[3] = n * (n - 1) * (2 * n + 5) - (6 * c2 + 12 * c1);
  };
  long long cu[4] = {0, 0, 0, 0}, ba[4];
  if (kept) ints(lane + 1, (long long)n_raw, cu);
  const int Sg = (int)cu[0];
#pragma unroll
  for (int q = 0; q < 4; ++q) cu[q] = wave_sum(cu[q]);
  const int n0 = finite_below(fin, pre, n_pooled) - finite_below(fin, pre, n_cur);
  ints(0, (long long)n0, ba);

  if (lane < G) {
    out.pod_S[row * G + lane] = Sg;
    out.pod_n[row * G + lane] = kept ? n_raw : 0;
  }
  if (lane == 0) {
    const double NaN = __builtin_nan("");
    double z = NaN, p = NaN, zc = NaN, tc = NaN, zb = NaN, tb = NaN;
    const bool applies = k >= 1 && n0 >= need && cu[3] > 0;
    if (applies) {
      side_stats(cu[0], cu[1], cu[2], cu[3], zc, tc);
      side_stats(ba[0], ba[1], ba[2], ba[3], zb, tb);
      z = (zc - zb) / sqrt(1.0 + (ba[3] > 0 ? 1.0 : 0.0));
      p = erfc(fabs(z) / 1.41421356237309504880);
    }
    float* o = out.drift + row * 6;
    const float pf = (float)p, tf = (float)tc;
    o[0] = (float)z; o[1] = pf; o[2] = (float)zc; o[3] = tf; o[4] = (float)zb; o[5] = (float)tb;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      out.counts[row * 8 + q] = cu[q];
      out.counts[row * 8 + 4 + q] = ba[q];
    }
    out.k[row] = k;
    out.drift_diff[row] = (applies && pf < p_thr && fabsf(tf) >= min_tau) ? 1 : 0;
  }
}

}  // namespace

template <int K>
__global__ __launch_bounds__(256) void drift_wave_kernel(const float* __restrict__ cur, int64_t ld_c, int n_cur,
                                                         const int* __restrict__ seg_end, int G,
                                                         const float* __restrict__ base, int64_t ld_b, int n_base,
                                                         int64_t R, int need, float p_thr, float min_tau,
                                                         DriftOut out) {
  __shared__ DriftRow<K> s_row[4];
  __shared__ DriftBins s_bins[4];
  DriftRow<K>* rw = &s_row[wave_id()];
  DriftBins* bins = &s_bins[wave_id()];
  const int lane = lane_id();
  const int n_pooled = n_cur + n_base;
  const int tiles = (n_pooled + kTile - 1) / kTile;           // <= K
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave_id(); row < R; row += (int64_t)gridDim.x * 4) {
    if (lane < G) bins->seg[lane] = (unsigned)seg_end[row * G + lane];
    for (int j = lane; j < kDriftBins; j += FM_WAVE) { bins->S[j] = 0; bins->c1[j] = 0u; bins->c2[j] = 0ull; }
    wave_lds_sync();
    load_tiles<1>(rw->x, rw->fin, rw->pre, bins->seg, G, cur + row * ld_c, base + row * ld_b, n_cur, n_pooled, tiles, 0);
    wave_lds_sync();
    scan_tiles(rw->fin, rw->pre, tiles);
    wave_lds_sync();
    float x[K];
    int lo[K], grp[K], gt[K], lt[K];
    load_block<K>(rw->x, bins->seg, G, n_cur, n_pooled, tiles, 0, x, lo, grp);
#pragma unroll
    for (int k = 0; k < K; ++k) gt[k] = lt[k] = 0;
    for (int t = 0; t < tiles; ++t) pair_tile<K>(rw->x, t * kTile, 0, x, lo, gt, lt);
    bin_block<K>(bins, rw->fin, rw->pre, 0, x, lo, grp, gt, lt);
    wave_lds_sync();
    drift_finish(bins, rw->fin, rw->pre, G, n_cur, n_pooled, need, p_thr, min_tau, row, out);
    wave_lds_sync();                                          // the row and the bins are reused by the next row
  }
}

template <int K>
__global__ __launch_bounds__(kDriftNT) void drift_wide_kernel(const float* __restrict__ cur, int64_t ld_c, int n_cur,
                                                              const int* __restrict__ seg_end, int G,
                                                              const float* __restrict__ base, int64_t ld_b, int n_base,
                                                              int64_t R, int need, float p_thr, float min_tau,
                                                              DriftOut out) {
  __shared__ DriftWideShared sh;
  DriftBins* bins = &sh.bins;
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
  const int n_pooled = n_cur + n_base;
  const int tiles = (n_pooled + kTile - 1) / kTile;
  constexpr int kBlock = K * kTile;
  const int blocks = (n_pooled + kBlock - 1) / kBlock;        // <= kDriftBlocks
  for (int64_t row = blockIdx.x; row < R; row += gridDim.x) {
    if (tid < G) bins->seg[tid] = (unsigned)seg_end[row * G + tid];
    if (tid < kDriftBins) { bins->S[tid] = 0; bins->c1[tid] = 0u; bins->c2[tid] = 0ull; }
    __syncthreads();
    load_tiles<kDriftWaves>(sh.row.x, sh.row.fin, sh.row.pre, bins->seg, G, cur + row * ld_c, base + row * ld_b, n_cur,
                            n_pooled, tiles, wave);
    __syncthreads();
    if (wave == 0) scan_tiles(sh.row.fin, sh.row.pre, tiles);
    __syncthreads();
    // ---- deal the blocks: lane b weighs block b by the columns its samples have to meet (its end less its
    // first segment's start), ranks it among the blocks (ties: the lower block first) and maps rank to wave
    int work = -1;
    if (lane < blocks) {
      int lo0;
      segment_of(bins->seg, G, lane * kBlock, n_cur, n_pooled, lo0);
      work = (lane + 1) * kBlock - lo0;
    }
    int rank = 0;
    for (int b = 0; b < kDriftBlocks; ++b) {
      const int w = lane_bcast(work, b);
      rank += (w > work || (w == work && b < lane)) ? 1 : 0;
    }
    const int turn = rank & (kDriftWaves - 1);
    const int owner = (rank / kDriftWaves & 1) ? kDriftWaves - 1 - turn : turn;
    unsigned mine = (unsigned)__ballot(lane < blocks && owner == wave);
    // ---- every block of this wave from its first segment's tile to its own last
    while (mine) {
      const int j0 = (__ffs(mine) - 1) * kBlock;
      mine &= mine - 1u;
      float x[K];
      int lo[K], grp[K], gt[K], lt[K];
      load_block<K>(sh.row.x, bins->seg, G, n_cur, n_pooled, tiles, j0, x, lo, grp);
#pragma unroll
      for (int k = 0; k < K; ++k) gt[k] = lt[k] = 0;
      const int t0 = uniform(lo[0]) / kTile;                  // (segment starts do not decrease along the row)
      const int t1 = min(tiles, (j0 + kBlock) / kTile);
      for (int t = t0; t < t1; ++t) pair_tile<K>(sh.row.x, t * kTile, j0, x, lo, gt, lt);
      bin_block<K>(bins, sh.row.fin, sh.row.pre, j0, x, lo, grp, gt, lt);
    }
    __syncthreads();
    if (wave == 0) drift_finish(bins, sh.row.fin, sh.row.pre, G, n_cur, n_pooled, need, p_thr, min_tau, row, out);
    __syncthreads();                                          // the row and the bins are reused by the next row
  }
}

// Per row: drift [R, 6] fp32 = (z, p, z_c, tau_c, z_b, tau_b), counts [R, 2, 4]
// int64 = (S, P, Tx2, V18) of the current side and the baseline, pod_S / pod_n
// [R, G] int32, k [R] int32, drift_diff [R] int8; every output of every row is
// written (NaN / 0 where the test does not apply).  seg_end [R, G] int32 (may
// be null with G == 0).  tier 0: the wave tier up to 1024 pooled columns, else
// the wide tier; tier 2: the wide tier.  G <= 64, n_cur + n_base <= 8192.
FM_API int fm_pairwise_drift(const float* cur, int64_t ld_c, int n_cur, const int* seg_end, int G, const float* base,
                             int64_t ld_b, int n_base, int64_t R, int min_points, float p_thr, float min_tau, int tier,
                             float* drift, long long* counts, int* pod_S, int* pod_n, int* k, int8_t* drift_diff,
                             hipStream_t stream) {
  if (n_cur < 0 || n_base < 0 || R < 0 || G < 0 || G > kDriftPodMax || (int64_t)n_cur + n_base > kPairwiseWideMax ||
      (tier != 0 && tier != 2))
    return (int)hipErrorInvalidValue;
  if (R == 0) return 0;
  if (drift == nullptr || counts == nullptr || k == nullptr || drift_diff == nullptr ||
      (G > 0 && (seg_end == nullptr || pod_S == nullptr || pod_n == nullptr)))
    return (int)hipErrorInvalidValue;
  const DriftOut out{drift, counts, pod_S, pod_n, k, drift_diff};
  const int need = min_points > 1 ? min_points : 1;
  const int n = n_cur + n_base;
#define FM_DRIFT(KERNEL, KK, GRID, NT)                                                                               \
  hipLaunchKernelGGL(KERNEL<KK>, GRID, dim3(NT), 0, stream, cur, ld_c, n_cur, seg_end, G, base, ld_b, n_base, R,     \
                     need, p_thr, min_tau, out)
  if (tier == 0 && n <= kDriftWaveMax) {
    const dim3 grid((unsigned)((R + 3) / 4 < 0x7FFFFFFF ? (R + 3) / 4 : 0x7FFFFFFF));
    if (n <= 64) FM_DRIFT(drift_wave_kernel, 1, grid, 256);
    else if (n <= 128) FM_DRIFT(drift_wave_kernel, 2, grid, 256);
    else if (n <= 256) FM_DRIFT(drift_wave_kernel, 4, grid, 256);
    else if (n <= 512) FM_DRIFT(drift_wave_kernel, 8, grid, 256);
    else FM_DRIFT(drift_wave_kernel, 16, grid, 256);
  } else {
    constexpr int64_t kMaxBlocks = 4096;     // beyond what the CUs hold at once the rows are strided
    const dim3 grid((unsigned)(R < kMaxBlocks ? R : kMaxBlocks));
    if (n <= kDriftBlocks * kTile) FM_DRIFT(drift_wide_kernel, 1, grid, kDriftNT);
    else if (n <= kDriftBlocks * kTile * 2) FM_DRIFT(drift_wide_kernel, 2, grid, kDriftNT);
    else FM_DRIFT(drift_wide_kernel, 4, grid, kDriftNT);
  }
#undef FM_DRIFT
  FM_LAUNCH_CHECK();
  return 0;
}
