// fm-hipcc-flags: -mllvm -pragma-unroll-threshold=1000000 -ffp-contract=off -Xclang -target-feature -Xclang -packed-fp32-ops
// (the unroll threshold as in pairwise.hip: the K = 16 bitonic network must
// unroll fully to stay in registers.  Contraction is off because the fp64
// finish is defined as plain products, quotients and sums, each rounded once,
// as the numpy reference evaluates them; for the same contract the device code
// uses no packed fp32 instructions.)
//
// K30: the joint multi-metric canary test (docs/BRAIN_SPEC.md 4.4): the
// Puri-Sen multivariate rank-sum statistic over the up to 8 metrics of a job.
// The contract is foremast_amd/ops/reference.py pairwise_joint / joint_verdict.
//
// A group is up to 8 member rows of cur [R, n_cur] / base [R, n_base] (rows
// [G, 8] int32, -1 padded; members [G] their number).  Column c of every
// member is the same sample, so a column counts only where every member is
// finite (listwise deletion).  Per member the midranks over its N kept pooled
// values, doubled and centred: a = rank2 - (N + 1), an integer below 1,024 in
// magnitude.  T_j = the sum of a_j over the kept current columns, A = a a^T
// over all kept columns, both exact; then in fp64 the elimination of A in
// member order (a constant or rank-collinear member is dropped), L = N (N - 1)
// / (n1 n2) * sum y_j^2 / d_j and its chi-square tail at dof = members kept.
//
// One workgroup of 8 waves per group, wave j owns member j; n_cur + n_base <=
// 1024, the pooled row in 64 K <= 1024 register slots per wave.
//
//   mask   every wave loads its member's pooled row and ballots finiteness
//          per register into fin[j][k] (a wave without a member: all ones);
//          after ONE barrier lane k < K of every wave ANDs the eight words
//          of register k: the keep mask, read out per register as a scalar.
//   rank   dropped columns become +inf, every value is tagged with its column,
//          bitonic_sort / avg_ranks (fm_pairwise.h, the wave tier's texts)
//          give the doubled midranks, and the centred a goes as int16 to LDS
//          a[j][column]: each of the 64 K slots is written exactly once (0 by
//          the pads, which carry the dropped columns' tags), a wave without a
//          member zeroes its row, so dropped columns, unused members and the
//          padding add nothing to T or A and nothing is compacted.
//   gram   A = a a^T on v_mfma_f64_16x16x4_f64: members are rows 0..7 of the
//          16 x 4 operand, rows 8..15 zero, and the same register serves as
//          both operands (B = a^T has a's own lane layout).  A chunk is 16
//          columns: lane (m, q) reads the four int16 a[m][16 u + 4 q ..] as
//          one 8-byte word and feeds them to four matrix instructions; which
//          column sits at which k index of which instruction is free, every
//          column is used once.  The 4 K chunks are dealt round robin to the 8
//          waves, the eight partial accumulators are summed through LDS in
//          wave order.  Every value is an integer below 2^31: fp64 holds them
//          exactly whatever the order, and A is written as int64.  The member
//          rows are 1,040 int16 apart (520 words = 8 mod 64), so the 32 lanes
//          that read (8 members x 4 k indices x 2 words) touch 64 banks once.
//   finish wave 0, every lane the same arithmetic: the elimination with its
//          factors in LDS, the statistic, chi2_sf (fm_common.h, the tail
//          K29's finish uses) with lgamma(dof / 2) as at most three logarithms;
//          lane j < 8 evaluates member j's marginal z, and the largest |z| is
//          an arg-max over those eight lanes that prefers the lower one.
//
// Whatever rows and members hold, a member index outside [0, R) reads nothing
// (the member is then missing everywhere, and no column is kept), members is
// clamped to 0..8, and a tag is a slot number below 64 K: no input makes an
// access leave its array.
#include "fm_pairwise.h"

namespace {

constexpr int kJointMembers = 8;             // members per group (JOINT_MAX_K in ops/canary.py, zoo.MVN_MAX_K)
constexpr int kJointMax = 1024;              // pooled columns (PAIRWISE_MAX in ops/canary.py)
constexpr int kJointWaves = 8;
constexpr int kJointNT = kJointWaves * FM_WAVE;
constexpr int kJointLd = kJointMax + 16;     // int16 per member row of a: 520 words, 8 mod 64

typedef double joint_acc_t __attribute__((ext_vector_type(4)));
typedef short joint_a4_t __attribute__((ext_vector_type(4)));

struct JointShared {
  unsigned long long fin[kJointMembers][kJointMax / FM_WAVE];   // finite lanes of register k of member j
  alignas(16) short a[kJointMembers][kJointLd];                 // centred doubled midranks by column
  double part[kJointWaves][4][FM_WAVE];                         // the waves' accumulators as the lanes hold them
  double A[kJointMembers * kJointMembers];
  double l[kJointMembers][kJointMembers], d[kJointMembers], y[kJointMembers];   // the finish's factors
  int T[kJointMembers];
};
// 34.9 KiB: four workgroups per CU by LDS, which is also all the 2,048 threads of a CU hold
static_assert(sizeof(JointShared) <= 40 * 1024 && 4 * sizeof(JointShared) <= 160 * 1024, "LDS of a workgroup");

struct JointOut {
  float* __restrict__ joint;                 // [G, 6]
  int* __restrict__ n12;                     // [G, 2]
  long long* __restrict__ T;                 // [G, 8]
  long long* __restrict__ A;                 // [G, 8, 8]
  float* __restrict__ member_z;              // [G, 8]
  int8_t* __restrict__ joint_diff;           // [G]
};

// Where the 16 x 16 fp64 accumulator keeps D[i][j]: register i / 4 of lane
// 16 (i % 4) + j.  (A is symmetric, so the transposed reading gives the same
// numbers.)
__device__ __forceinline__ int gram_reg(int i) { return i >> 2; }
__device__ __forceinline__ int gram_lane(int i, int j) { return 16 * (i & 3) + j; }

// The finishing pass of a group, run by one whole wave once sh.A and sh.T are
// complete and visible.  Uniform but for the marginal z of lane j < 8.
__device__ __forceinline__ void joint_finish(JointShared& sh, int n1, int n2, int need, float p_thr, int64_t g,
                                             const JointOut& out) {
  constexpr int M = kJointMembers;
  const int lane = lane_id();
  const double NaN = __builtin_nan("");
  // l, d and y live in LDS and the loops stay rolled: unrolled into registers the factors cost the whole kernel
  // a hundred VGPRs.  Every lane stores the same numbers and reads back its own stores.
  int dof = 0;
  double q = 0.0;                            // sum over the kept members of y^2 / d
#pragma unroll 1
  for (int j = 0; j < M; ++j) {
    const double ajj = sh.A[j * M + j];
#pragma unroll 1
    for (int k = 0; k < j; ++k) {
      double s = 0.0;
#pragma unroll 1
      for (int m = 0; m < k; ++m) s += sh.l[j][m] * sh.l[k][m] * sh.d[m];
      const double dk = sh.d[k];             // (0 marks a dropped member: its factors are zeros, its terms add 0.0)
      sh.l[j][k] = dk != 0.0 ? (sh.A[j * M + k] - s) / dk : 0.0;
    }
    double s = 0.0, t = 0.0;
#pragma unroll 1
    for (int k = 0; k < j; ++k) s += sh.l[j][k] * sh.l[j][k] * sh.d[k];
#pragma unroll 1
    for (int k = 0; k < j; ++k) t += sh.l[j][k] * sh.y[k];
    const double dj = ajj - s, yj = (double)sh.T[j] - t;
    const bool kept = !(ajj == 0.0 || dj <= 1e-9 * ajj);
    sh.d[j] = kept ? dj : 0.0;
    sh.y[j] = kept ? yj : 0.0;
    dof += kept ? 1 : 0;
    q += kept ? yj * yj / dj : 0.0;
  }
  const int N = n1 + n2;
  const bool applies = n1 >= need && n2 >= need && dof > 0;
  const double dN = (double)N, d12 = (double)n1 * (double)n2;

  // the marginals: lane j owns member j; arg-max of |z| over lanes 0..7, the lower lane on ties
  const int j = lane & (M - 1);
  const double ajj = sh.A[j * M + j];
  double z = NaN, az = -1.0;
  if (applies && ajj != 0.0) {
    z = (double)sh.T[j] / sqrt(d12 / (dN * (dN - 1.0)) * ajj);
    az = fabs(z);
  }
  int worst = j;
  double zw = z;
#define FM_JOINT_ARGMAX(S)                                                   \
  {                                                                          \
    const double oa = xor_lane<S>(az), oz = xor_lane<S>(zw);                 \
    const int ow = xor_lane<S>(worst);                                       \
    const bool take = oa > az || (oa == az && ow < worst);                   \
    az = take ? oa : az;                                                     \
    zw = take ? oz : zw;                                                     \
    worst = take ? ow : worst;                                               \
  }
  FM_JOINT_ARGMAX(1) FM_JOINT_ARGMAX(2) FM_JOINT_ARGMAX(4)
#undef FM_JOINT_ARGMAX

  if (lane < M) {
    out.T[g * M + lane] = (long long)sh.T[lane];
    out.member_z[g * M + lane] = (float)z;
  }
  if (lane == 0) {
    double L = NaN, p = NaN;
    if (applies) {
      L = dN * (dN - 1.0) / d12 * q;
      // lgamma(dof / 2) as in K29's finish: logarithms down to lgamma(1) = 0 or lgamma(1 / 2) = log(sqrt(pi))
      double gln = (dof & 1) ? 0.57236494292470008707 : 0.0;
      for (int m = 1; m <= ((dof - 1) >> 1); ++m) gln += log(0.5 * (double)dof - (double)m);
      p = chi2_sf(L, (double)dof, gln);
    }
    const float pf = (float)p;
    float* o = out.joint + g * 6;
    o[0] = (float)L; o[1] = pf; o[2] = (float)dof; o[3] = applies ? (float)zw : (float)NaN;
    o[4] = applies ? (float)worst : -1.f; o[5] = (float)N;
    out.n12[g * 2] = n1; out.n12[g * 2 + 1] = n2;
    out.joint_diff[g] = (applies && pf < p_thr) ? 1 : 0;
  }
}

}  // namespace

template <int K>
__global__ __launch_bounds__(kJointNT) void joint_kernel(const float* __restrict__ cur, int64_t ld_c, int n_cur,
                                                         const float* __restrict__ base, int64_t ld_b, int n_base,
                                                         int64_t R, const int* __restrict__ rows,
                                                         const int* __restrict__ members, int64_t G, int need,
                                                         float p_thr, JointOut out) {
  __shared__ JointShared sh;
  const int lane = lane_id(), w = wave_id();
  const int n_pooled = n_cur + n_base;
  for (int64_t g = blockIdx.x; g < G; g += gridDim.x) {
    int kg = members[g];
    kg = kg < 0 ? 0 : (kg > kJointMembers ? kJointMembers : kg);
    const bool has_member = w < kg;          // wave-uniform
    // ---- mask: the member's pooled row, its finite lanes per register
    float v[K];
    if (has_member) {
      const int64_t row = rows[g * kJointMembers + w];
      const bool ok = row >= 0 && row < R;   // (a member that is no row is missing everywhere)
      const float* c = cur + (ok ? row : 0) * ld_c;
      const float* b = base + (ok ? row : 0) * ld_b;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int i = k * 64 + lane;
        v[k] = !ok ? kPad : (i < n_cur ? c[i] : (i < n_pooled ? b[i - n_cur] : kPad));
      }
    } else {
#pragma unroll
      for (int k = 0; k < K; ++k) v[k] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const unsigned long long f = __ballot(isfinite(v[k]));
      if (lane == 0) sh.fin[w][k] = f;
    }
    __syncthreads();
    unsigned long long mine = ~0ull;         // lane k: the columns of register k that every member has
    if (lane < K) {
#pragma unroll
      for (int j = 0; j < kJointMembers; ++j) mine &= sh.fin[j][lane];
    }
    int n1 = 0, n2 = 0;
    bool keep[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)mine, k);
      const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(mine >> 32), k);
      const int i = k * 64 + lane;
      keep[k] = ((((unsigned long long)hi << 32) | lo) >> lane & 1ull) != 0ull && i < n_pooled;
      n1 += __popcll(__ballot(keep[k] && i < n_cur));
      n2 += __popcll(__ballot(keep[k] && i >= n_cur));
    }
    const int N = n1 + n2;
    // ---- rank: the centred doubled midrank of every kept value, to its own column
    if (has_member) {
      int tag[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        v[k] = keep[k] ? v[k] : kPad;
        tag[k] = k * 64 + lane;
      }
      bitonic_sort<K, false, true>(v, tag);
      int rk2[K];
      bool en[K];
      avg_ranks<K, true>(v, N, rk2, en);
      int t = 0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int a = k * 64 + lane < N ? rk2[k] - (N + 1) : 0;     // (the pads sort behind the N kept values)
        sh.a[w][tag[k]] = (short)a;
        t += tag[k] < n_cur ? a : 0;
      }
      t = (int)wave_sum_uniform((unsigned)t);
      if (lane == 0) sh.T[w] = t;
    } else {
      int* z = reinterpret_cast<int*>(sh.a[w]);
      for (int i = lane; i < 32 * K; i += FM_WAVE) z[i] = 0;
      if (lane == 0) sh.T[w] = 0;
    }
    __syncthreads();
    // ---- gram: this wave's chunks of 16 columns through the matrix unit
    {
      joint_acc_t acc = {0.0, 0.0, 0.0, 0.0};
      const int m = lane & 15, q = lane >> 4;
      for (int u = w; u < 4 * K; u += kJointWaves) {
        joint_a4_t s = {0, 0, 0, 0};
        if (m < kJointMembers) s = *reinterpret_cast<const joint_a4_t*>(&sh.a[m][16 * u + 4 * q]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const double x = (double)s[t];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) sh.part[w][r][lane] = acc[r];
    }
    __syncthreads();
    if (w == 0) {
      const int i = lane >> 3, j = lane & 7;
      double s = 0.0;
#pragma unroll
      for (int p = 0; p < kJointWaves; ++p) s += sh.part[p][gram_reg(i)][gram_lane(i, j)];
      sh.A[lane] = s;
      out.A[g * (kJointMembers * kJointMembers) + lane] = (long long)s;
      // the wave's own LDS stores, read back by all of its lanes
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      joint_finish(sh, n1, n2, need, p_thr, g, out);
    }
    // (no barrier here: the next group's stores before its first barrier go to fin, which nothing above reads after
    // the first barrier of this group; a, T, part and A are written again only behind a barrier wave 0 has to reach)
  }
}

// Per group: joint [G, 6] fp32 = (L, p, dof, z_worst, worst, N), n12 [G, 2]
// int32, T [G, 8] int64, A [G, 8, 8] int64, member_z [G, 8] fp32, joint_diff
// [G] int8; every output of every group is written (NaN / -1 / 0 where the
// test does not apply).  rows [G, 8] int32 member rows (-1 padded), members
// [G] int32.  n_cur + n_base <= 1024.
FM_API int fm_pairwise_joint(const float* cur, int64_t ld_c, int n_cur, const float* base, int64_t ld_b, int n_base,
                             int64_t R, const int* rows, const int* members, int64_t G, int min_points, float p_thr,
                             float* joint, int* n12, long long* T, long long* A, float* member_z, int8_t* joint_diff,
                             hipStream_t stream) {
  if (n_cur < 0 || n_base < 0 || R < 0 || G < 0 || (int64_t)n_cur + n_base > kJointMax) return (int)hipErrorInvalidValue;
  if (G == 0) return 0;
  if (rows == nullptr || members == nullptr || joint == nullptr || n12 == nullptr || T == nullptr || A == nullptr ||
      member_z == nullptr || joint_diff == nullptr || (R > 0 && (n_cur > 0 && cur == nullptr)) ||
      (R > 0 && (n_base > 0 && base == nullptr)))
    return (int)hipErrorInvalidValue;
  const JointOut out{joint, n12, T, A, member_z, joint_diff};
  const int need = min_points > 1 ? min_points : 1;
  const int n = n_cur + n_base;
  constexpr int64_t kMaxBlocks = 4096;       // beyond what the CUs hold at once the groups are strided
  const dim3 grid((unsigned)(G < kMaxBlocks ? G : kMaxBlocks)), block(kJointNT);
#define FM_JOINT(KK)                                                                                                 \
  hipLaunchKernelGGL(joint_kernel<KK>, grid, block, 0, stream, cur, ld_c, n_cur, base, ld_b, n_base, R, rows, members, \
                     G, need, p_thr, out)
  if (n <= 64) FM_JOINT(1);
  else if (n <= 128) FM_JOINT(2);
  else if (n <= 256) FM_JOINT(4);
  else if (n <= 512) FM_JOINT(8);
  else FM_JOINT(16);
#undef FM_JOINT
  FM_LAUNCH_CHECK();
  return 0;
}
