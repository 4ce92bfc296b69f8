// K37: the joint multivariate-normal detector for groups of 9 to 32 member
// rows, plain (`multivariate_normal`) and robust (`robust_multivariate`).  The
// definition is K12's and K17's (foremast_amd/ops/misc.py ref_mvn and
// ref_mvn_robust, docs/BRAIN_SPEC.md §3); what differs is how the moments are
// taken.  K12 keeps K + K(K+1)/2 running sums a thread in registers (44 at
// K = 8, 560 at K = 32) and spends 5.5 VALU FMAs a loaded float; at K = 32 the
// Gram matrix D W D^T wants 33 products a loaded float, which is the shape of
// v_mfma_f32_32x32x2_f32.
//
// One 256-thread workgroup per group; rows are addressed in place through
// rows[G, 32] (int32 row ids, -1 padding) into hist[R, ld] / cur[R, ld_c]: no
// gathered copy of the history is made and T is unbounded.
//
//   stage   a wave owns the column tiles wv, wv + 4, ... of 64 columns.  Lane l
//           loads 16 B of member (l >> 4) + 4 i at quad l & 15, i = 0 .. 7: four
//           whole 256-B row segments an instruction, the next tile's loads in
//           flight while this one is multiplied.  A 4-bit mask a lane says
//           which of its columns are finite in all of its members (and, robust
//           form, in none further than its limit from its centre); two lane
//           swaps combine the four row groups into the column weight.  The
//           weight is 0 or 1, so w d_a d_b = (w d_a)(w d_b): the column is
//           zeroed as it is written to LDS and the A and B operands are the
//           same register.  Non-finite samples and the members K .. 31 are 0.
//           The tile is 32 rows of 65 floats: the odd stride spreads both the
//           stores (bank = row group + 4 quad + e) and the operand reads over
//           all banks.
//   gram    lane l reads member l & 31 at column c + 32 (l >> 5), c = 0 .. 31
//           (bank = member + c + 32 half: conflict-free on 64 banks and, half a
//           wave at a time, on 32), one MFMA a read into a 16-register fp32
//           tile; the member sums S_a ride on the VALU (one add a read) and the
//           column count N on the masks.  Every kFlush tiles (512 columns a
//           wave) the fp32 tile is added to an fp64 one in registers and
//           cleared, so no fp32 sum is longer than 512 products.
//   reduce  the waves' fp64 tiles meet in LDS; mu = s + S / N, M_ab = P_ab -
//           S_a S_b / N, C = M / max(N - 1, 1), all fp64.
//   solve   live members have diag(C) > 1e-12 mu^2 + 1e-30; the others (and
//           the padding) keep a unit diagonal and zero couplings, which leaves
//           the distance that of the live members alone.  Wave 0 factors
//           R + 1e-6 I in registers, lane j column j (fm_chol_regs.h, K36's
//           factorisation); L and 1 / diag(L) go to LDS.
//   score   one current point a lane: column-oriented forward substitution
//           L y = z, d = |y|, the dead-member and present rules, the cut
//           cuts[lowered][k]; flags by ballot.
//
// The shift s of the plain form is K12's form 1: the mean of the complete
// columns among the last 16 tiles (1,024 columns), a mean sweep when that tail
// holds none.  The robust form shifts by the member's median, and a counting
// sweep (loads and masks only, nothing staged) gives `complete` and `rejected`
// before the Gram sweep, so that the breakdown guard (2 rejected > complete:
// nothing is rejected) is known when the columns are weighted.
#include "fm_chol_regs.h"
#include "fm_common.h"

using namespace fm;

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int kNT = 256;
constexpr int kWaves = kNT / FM_WAVE;
constexpr int kM = 32;                 // members of the operand (the group's K, zero padded)
constexpr int kC = 64;                 // columns of a tile
constexpr int kStride = kC + 1;
constexpr int kFlush = 8;              // tiles between two fp64 flushes of a wave's fp32 tile (docs/PERF.md)
constexpr int kTailTiles = 16;         // the shift's tail: the last 1,024 columns
constexpr double kRidge = 1e-6;        // foremast_amd/ops/misc.py MVN_RIDGE

enum Mode { kCount, kMean, kGram };

struct WideShared {
  float tile[kWaves][kM * kStride];
  double P[kM * kM];                   // Gram, then the covariance (full, symmetric)
  double L[kM * kM];                   // the factor below the diagonal, 1 / diag(L) on it
  double part[kWaves][kM];             // the waves' member sums
  double sum[kM], mu[kM], isd[kM];
  float shift[kM];
  int rid[kM];
  int cnt[kWaves], rej[kWaves];
  int redi[kWaves];
  float cut;
  int ok, rows_ok;
};

// LDS written by some lanes of this wave is read by others: the wave's LDS
// operations complete in order; this keeps the compiler from moving them
// across and waits for the stores.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// This lane's share of tile t: d = x - s of members (lane >> 4) + 4 i at quad
// lane & 15 (0 for a non-finite sample, a member >= K and a column >= T), and
// the wave-combined masks of its four columns: okm = finite in every member,
// outm = some member beyond its limit.
template <bool ROBUST>
__device__ __forceinline__ void load_tile(const float4* const (&rp)[8], const float (&sh)[8], const float (&lim)[8],
                                          int K, int t, int T, int nq, float4 (&v)[8], unsigned& okm, unsigned& outm) {
  const int lane = lane_id(), r0 = lane >> 4;
  const int qi = t * (kC / 4) + (lane & 15);
  const bool inq = qi < nq;
  unsigned ok = 0, out = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) ok |= (qi * 4 + e < T ? 1u : 0u) << e;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + 4 * i < K && inq) {
      const float4 x = rp[i][qi];
      const float xe[4] = {x.x, x.y, x.z, x.w};
      float d[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool fin = isfinite(xe[e]);
        const float de = __fsub_rn(xe[e], sh[i]);
        if (!fin) ok &= ~(1u << e);
        if (ROBUST && fabsf(de) > lim[i]) out |= 1u << e;
        d[e] = fin ? de : 0.f;
      }
      v[i] = make_float4(d[0], d[1], d[2], d[3]);
    }
  }
  ok &= xor_lane<16>(ok);
  ok &= xor_lane<32>(ok);
  if (ROBUST) {
    out |= xor_lane<16>(out);
    out |= xor_lane<32>(out);
  }
  okm = ok;
  outm = out;
}

// The rows < K of the wave's tile, the columns outside `use` zeroed.
__device__ __forceinline__ void store_tile(float* tile, const float4 (&v)[8], unsigned use, int K) {
  const int lane = lane_id(), r0 = lane >> 4;
  float* base = tile + r0 * kStride + 4 * (lane & 15);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (r0 + 4 * i < K) {
      float* p = base + 4 * i * kStride;
      p[0] = (use & 1u) ? v[i].x : 0.f;
      p[1] = (use & 2u) ? v[i].y : 0.f;
      p[2] = (use & 4u) ? v[i].z : 0.f;
      p[3] = (use & 8u) ? v[i].w : 0.f;
    }
  }
}

// One wave over its tiles t_first, t_first + kWaves, ... < t_end.  Every mode
// tallies the columns used (cnt) and, robust form, those complete but rejected
// (rej), on the lanes < 16.  kMean and kGram stage the tile and add this lane's
// member (lane & 31) over its 32 columns into srow; kGram also accumulates the
// Gram tile: acc[e] = row (e & 3) + 8 (e >> 2) + 4 (lane >> 5), column lane & 31.
template <bool ROBUST, Mode MODE, int FLUSH>
__device__ __forceinline__ void sweep(float* tile, const float4* const (&rp)[8], const float (&sh)[8],
                                      const float (&lim)[8], int K, int T, int nq, int t_first, int t_end,
                                      double (&acc64)[16], double& srow64, int& cnt, int& rej) {
  const int lane = lane_id();
  const float* tp = tile + (lane & 31) * kStride + 32 * (lane >> 5);
  f32x16 acc = f32x16{};
  float srow = 0.f;
  int since = 0;
  float4 v[8];
  unsigned okm = 0, outm = 0;
  int t = t_first;
  if (t < t_end) load_tile<ROBUST>(rp, sh, lim, K, t, T, nq, v, okm, outm);
  while (t < t_end) {                                         // (t is wave-uniform)
    const unsigned use = okm & ~outm;
    if (lane < 16) {
      cnt += __popc(use);
      rej += __popc(okm & outm);
    }
    if (MODE != kCount) {
      store_tile(tile, v, use, K);
      wave_lds_sync();
    }
    t += kWaves;
    if (t < t_end) load_tile<ROBUST>(rp, sh, lim, K, t, T, nq, v, okm, outm);
    if (MODE != kCount) {
#pragma unroll
      for (int c = 0; c < 32; ++c) {
        const float a = tp[c];
        if (MODE == kGram) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, a, acc, 0, 0, 0);
        srow += a;
      }
      wave_lds_sync();                                        // the tile is rewritten by the next store
      if (++since == FLUSH) {
        since = 0;
        if (MODE == kGram) {
#pragma unroll
          for (int e = 0; e < 16; ++e) acc64[e] += (double)acc[e];
          acc = f32x16{};
        }
        srow64 += (double)srow;
        srow = 0.f;
      }
    }
  }
  if (MODE == kGram) {
#pragma unroll
    for (int e = 0; e < 16; ++e) acc64[e] += (double)acc[e];
  }
  srow64 += (double)srow;
}

// The waves' member sums and column tallies -> S.sum[0 .. 32) and the block's
// (cnt, rej).  Called by every thread.
__device__ __forceinline__ void reduce_sums(WideShared& S, double srow64, int cnt, int rej, int& tot_cnt, int& tot_rej) {
  const int lane = lane_id(), wv = wave_id();
  const double sr = srow64 + xor_lane<32>(srow64);
  cnt = wave_sum(cnt);
  rej = wave_sum(rej);
  if (lane < kM) S.part[wv][lane] = sr;
  if (lane == 0) {
    S.cnt[wv] = cnt;
    S.rej[wv] = rej;
  }
  __syncthreads();
  tot_cnt = tot_rej = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    tot_cnt += S.cnt[w];
    tot_rej += S.rej[w];
  }
  if (threadIdx.x < kM) S.sum[threadIdx.x] = (S.part[0][threadIdx.x] + S.part[1][threadIdx.x]) +
                                             (S.part[2][threadIdx.x] + S.part[3][threadIdx.x]);
  __syncthreads();
}

// (the second launch bound: three workgroups share a CU's 160 KB of LDS, so the registers are held to three
// waves a SIMD)
template <bool ROBUST, int FLUSH>
__global__ __launch_bounds__(kNT, 3) void mvn_wide_kernel(const float* __restrict__ hist, int64_t ld, int T, int64_t R,
                                                       const float* __restrict__ cur, int64_t ld_c, int n,
                                                       const int* __restrict__ rows /*[G,32]*/, int K,
                                                       const float* __restrict__ cuts /*[2,33]*/,
                                                       const unsigned char* __restrict__ lowered /*[G]*/, int min_n,
                                                       const float* __restrict__ stats /*[R,3]*/, float reject,
                                                       float* __restrict__ params /*[G,2+K+NP]*/,
                                                       float* __restrict__ dist /*[G,n]*/,
                                                       unsigned long long* __restrict__ flags, int NW,
                                                       int* __restrict__ count, int* __restrict__ valid,
                                                       int* __restrict__ rejected) {
  __shared__ WideShared S;
  const int64_t g = blockIdx.x;
  const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
  const int NA = K + K * (K + 1) / 2;

  // ---- the member rows; a group with a row id outside the buffer reads nothing and comes out invalid
  if (wv == 0) {
    const int id = lane < K ? rows[g * kM + lane] : 0;
    const bool bad = id < 0 || id >= R;
    if (lane < kM) S.rid[lane] = bad ? 0 : id;
    const unsigned long long any_bad = __ballot(bad);
    if (lane == 0) S.rows_ok = any_bad == 0ull;
  }
  float* tile = S.tile[wv];
  for (int i = lane; i < kM * kStride; i += FM_WAVE) tile[i] = 0.f;     // the members >= K stay 0
  __syncthreads();
  const bool rows_ok = S.rows_ok != 0;
  const int nq = rows_ok ? (T + 3) >> 2 : 0;
  const int nt = rows_ok ? (T + kC - 1) / kC : 0;

  // ---- this lane's staging rows (lane >> 4) + 4 i: pointer, shift and limit
  const float4* rp[8];
  float sh[8], lim[8];
  const bool rejecting = ROBUST && reject > 0.f && !isinf(reject);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = (lane >> 4) + 4 * i;
    const int64_t id = S.rid[r];                              // (0 for the padding: never read)
    rp[i] = reinterpret_cast<const float4*>(hist + id * ld);
    sh[i] = 0.f;
    lim[i] = INFINITY;
    if (ROBUST && r < K && rows_ok) {
      // a member without a finite sample has NaN statistics: its shift is 0 (the group has no complete
      // column anyway) and its NaN limit compares false, as in the oracle
      const float med = stats[id * 3], sg = stats[id * 3 + 1];
      sh[i] = isfinite(med) ? med : 0.f;
      lim[i] = rejecting ? __fmul_rn(reject, sg) : INFINITY;
    }
  }

  double acc64[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc64[e] = 0.0;
  int nrej = 0;
  if (ROBUST) {
    // (sixteen lanes stage each member; those of quad 0 publish its shift, 0 for the padding)
    if (wv == 0 && (lane & 15) == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) S.shift[(lane >> 4) + 4 * i] = sh[i];
    }
    // ---- counting sweep: the breakdown guard is known before the columns are weighted
    double unused = 0.0;
    int cnt = 0, rej = 0, complete;
    sweep<true, kCount, FLUSH>(tile, rp, sh, lim, K, T, nq, wv, nt, acc64, unused, cnt, rej);
    reduce_sums(S, 0.0, cnt, rej, complete, nrej);
    complete += nrej;
    if (2 * nrej > complete) {                                // (block-uniform)
      nrej = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) lim[i] = INFINITY;
    }
  } else {
    // ---- the shift: the mean of the complete columns of the tail, else of all columns
    const int t_tail = nt > kTailTiles ? nt - kTailTiles : 0;
    double srow64 = 0.0;
    int cnt = 0, rej = 0, c0, r0;
    sweep<false, kMean, FLUSH>(tile, rp, sh, lim, K, T, nq, t_tail + wv, nt, acc64, srow64, cnt, rej);
    reduce_sums(S, srow64, cnt, rej, c0, r0);
    if (c0 == 0 && t_tail > 0) {                              // (block-uniform)
      srow64 = 0.0;
      cnt = 0;
      sweep<false, kMean, FLUSH>(tile, rp, sh, lim, K, T, nq, wv, t_tail, acc64, srow64, cnt, rej);
      reduce_sums(S, srow64, cnt, rej, c0, r0);
    }
    if (tid < kM) S.shift[tid] = c0 > 0 ? (float)(S.sum[tid] / (double)c0) : 0.f;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) sh[i] = S.shift[(lane >> 4) + 4 * i];
  }

  // ---- the Gram sweep
  int Ni;
  {
    double srow64 = 0.0;
    int cnt = 0, rej = 0, r0;
    sweep<ROBUST, kGram, FLUSH>(tile, rp, sh, lim, K, T, nq, wv, nt, acc64, srow64, cnt, rej);
#pragma unroll 1
    for (int w = 0; w < kWaves; ++w) {
      if (wv == w) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int idx = ((e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)) * kM + (lane & 31);
          S.P[idx] = (w ? S.P[idx] : 0.0) + acc64[e];
        }
      }
      __syncthreads();
    }
    reduce_sums(S, srow64, cnt, rej, Ni, r0);
  }
  if (ROBUST && tid == 0) rejected[g] = nrej;

  // ---- moments: mu, the live test, the cut (wave 0), then the covariance in place (all threads)
  const double N = (double)Ni;
  const double inv_n = Ni > 0 ? 1.0 / N : 0.0, den = Ni > 1 ? N - 1.0 : 1.0;
  float* pr = params + g * (2 + NA);
  if (wv == 0) {
    bool live = false;
    if (lane < kM) {
      const double Sa = S.sum[lane];
      const double mu = (double)S.shift[lane] + Sa * inv_n;
      // one column has no spread: exactly 0, where a shift that is not the column itself (the robust
      // form's median) would leave the rounding of the fp32 products
      const double caa = Ni > 1 ? (S.P[lane * kM + lane] - Sa * Sa * inv_n) / den : 0.0;
      live = lane < K && caa > 1e-12 * mu * mu + 1e-30;
      S.mu[lane] = mu;
      S.isd[lane] = live ? 1.0 / sqrt(caa) : 0.0;
      if (lane < K) pr[2 + lane] = (float)mu;
    }
    const int k = __popcll(__ballot(live));
    if (lane == 0) {
      const int need = min_n > K + 2 ? min_n : K + 2;
      pr[0] = (float)Ni;
      pr[1] = (float)k;
      S.cut = cuts[(lowered[g] ? kM + 1 : 0) + k];
      S.ok = Ni >= need ? 1 : 0;
    }
  }
  __syncthreads();                                            // (the diagonal of P was read above)
  for (int idx = tid; idx < kM * kM; idx += kNT) {
    const int a = idx >> 5, b = idx & 31;
    if (a <= b) {                                             // (the lower triangle is written, never read)
      const double c = Ni > 1 ? (S.P[idx] - S.sum[a] * S.sum[b] * inv_n) / den : 0.0;
      S.P[idx] = c;
      S.P[b * kM + a] = c;
      if (b < K) pr[2 + K + a * K - a * (a - 1) / 2 + (b - a)] = (float)c;
    }
  }
  __syncthreads();

  // ---- solve: R + ridge over the live members, a unit diagonal and zero couplings elsewhere
  if (wv == 0) {
    const int j = lane & 31;
    const double isdj = S.isd[j];
    double a[kM];
#pragma unroll
    for (int i = 0; i < kM; ++i) a[i] = i == j ? 1.0 + kRidge : S.P[i * kM + j] * S.isd[i] * isdj;
    chol_columns<kM, kM>(a, j);
    // L[i][j] below the diagonal, 1 / L[j][j] on it (what is left above it is never read)
    if (lane < kM) {
#pragma unroll
      for (int i = 0; i < kM; ++i) S.L[i * kM + j] = a[i];
    }
  }
  __syncthreads();

  // ---- current points, one per thread
  const bool okg = S.ok != 0;
  const float cut = S.cut;
  int nflag = 0, npres = 0;
#pragma unroll 1
  for (int i0 = 0; i0 < n; i0 += kNT) {
    asm volatile("" ::: "memory");                            // L is read where it is used, not hoisted into registers
    const int i = i0 + tid;
    bool f = false;
    if (i < n) {
      float d = NAN;
      if (rows_ok) {
        bool present = true, moved = false;
        double z[kM];
#pragma unroll
        for (int a = 0; a < kM; ++a) {
          z[a] = 0.0;
          if (a < K) {
            const float x = cur[(int64_t)S.rid[a] * ld_c + i];
            present = present && isfinite(x);
            const double mu = S.mu[a], isd = S.isd[a], dx = (double)x - mu;
            moved = moved || (isd == 0.0 && fabs(dx) > 1e-6 * fabs(mu) + 1e-12);
            z[a] = dx * isd;
          }
        }
        npres += present;
        if (present && okg) {
          // L y = z by columns: y_b is final once the columns before it are taken off
          double q = 0.0;
#pragma unroll
          for (int b = 0; b < kM; ++b) {
            if (b < K) {
              const double y = z[b] * S.L[b * kM + b];
              q = fma(y, y, q);
#pragma unroll
              for (int a = b + 1; a < kM; ++a) z[a] = fma(-S.L[a * kM + b], y, z[a]);
            }
          }
          d = moved ? INFINITY : (float)sqrt(q);
          f = d > cut;
          nflag += f;
        }
      }
      dist[g * n + i] = d;
    }
    const unsigned long long bal = __ballot(f);
    const int w = i0 / 64 + wv;
    if (lane == 0 && w < NW) flags[g * NW + w] = bal;
  }
  nflag = block_sum<kNT>(nflag, S.redi);
  npres = block_sum<kNT>(npres, S.redi);
  if (tid == 0) {
    count[g] = nflag;
    valid[g] = (okg ? 1 : 0) | (npres > 0 ? 2 : 0);
  }
}

template <bool ROBUST, int FLUSH = kFlush>
int launch(const float* hist, int64_t ld, int T, int64_t R, const float* cur, int64_t ld_c, int n, const int* rows,
           int64_t G, int K, const float* cuts, const unsigned char* lowered, int min_n, const float* stats,
           float reject, float* params, float* dist, unsigned long long* flags, int NW, int* count, int* valid,
           int* rejected, hipStream_t stream) {
  if (G <= 0) return 0;
  if (K < 9 || K > kM || T <= 0 || n <= 0 || R <= 0 || (ld & 3) || ld < T || ld_c < n || (((uintptr_t)hist) & 15) ||
      NW * 64 < n || G > 0x7fffffffLL || (ROBUST && (stats == nullptr || rejected == nullptr)))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL((mvn_wide_kernel<ROBUST, FLUSH>), dim3((unsigned)G), dim3(kNT), 0, stream, hist, ld, T, R, cur, ld_c, n,
                     rows, K, cuts, lowered, min_n, stats, reject, params, dist, flags, NW, count, valid, rejected);
  FM_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// hist [R, ld], cur [R, ld_c], rows [G, 32] int32 (first K entries of each
// group used, 9 <= K <= 32), cuts [2, 33], lowered [G] bytes.  Outputs as
// fm_mvn: params [G, 2 + K + K(K+1)/2], dist [G, n], flags [G, NW], count,
// valid [G].
FM_API int fm_mvn_wide(const float* hist, int64_t ld, int T, int64_t R, const float* cur, int64_t ld_c, int n,
                       const int* rows, int64_t G, int K, const float* cuts, const unsigned char* lowered, int min_n,
                       float* params, float* dist, unsigned long long* flags, int NW, int* count, int* valid,
                       hipStream_t stream) {
  return launch<false>(hist, ld, T, R, cur, ld_c, n, rows, G, K, cuts, lowered, min_n, nullptr, 0.f, params, dist,
                       flags, NW, count, valid, nullptr, stream);
}

// fm_mvn_wide with the incident columns set aside: stats [R, 3] as
// fm_robust_stats writes them over the same T columns (only the member rows
// are read), reject <= 0, NaN or +inf: nothing is rejected; rejected [G].
FM_API int fm_mvn_wide_robust(const float* hist, int64_t ld, int T, int64_t R, const float* cur, int64_t ld_c, int n,
                              const int* rows, int64_t G, int K, const float* cuts, const unsigned char* lowered,
                              int min_n, const float* stats, float reject, float* params, float* dist,
                              unsigned long long* flags, int NW, int* count, int* valid, int* rejected,
                              hipStream_t stream) {
  return launch<true>(hist, ld, T, R, cur, ld_c, n, rows, G, K, cuts, lowered, min_n, stats, reject, params, dist,
                      flags, NW, count, valid, rejected, stream);
}

// fm_mvn_wide with another flush interval (2 or 32 tiles; anything else is the
// default): for benchmarks/bench_mvn_wide.py, which measures whether the
// interval matters.
FM_API int fm_mvn_wide_flush(const float* hist, int64_t ld, int T, int64_t R, const float* cur, int64_t ld_c, int n,
                             const int* rows, int64_t G, int K, const float* cuts, const unsigned char* lowered,
                             int min_n, int flush, float* params, float* dist, unsigned long long* flags, int NW,
                             int* count, int* valid, hipStream_t stream) {
  if (flush == 2)
    return launch<false, 2>(hist, ld, T, R, cur, ld_c, n, rows, G, K, cuts, lowered, min_n, nullptr, 0.f, params,
                            dist, flags, NW, count, valid, nullptr, stream);
  if (flush == 32)
    return launch<false, 32>(hist, ld, T, R, cur, ld_c, n, rows, G, K, cuts, lowered, min_n, nullptr, 0.f, params,
                             dist, flags, NW, count, valid, nullptr, stream);
  return fm_mvn_wide(hist, ld, T, R, cur, ld_c, n, rows, G, K, cuts, lowered, min_n, params, dist, flags, NW, count,
                     valid, stream);
}
