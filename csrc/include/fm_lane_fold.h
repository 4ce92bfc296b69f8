// Lane-level pieces of the lane-per-metric service decision, shared by
// decide.hip (fm_decide_services) and decide_2s.hip (fm_decide_services_2s).
#pragma once
#include "fm_common.h"

using namespace fm;

// v with lane `l` (a constant) replaced by the wave-uniform s: v_writelane_b32.
// This toolchain has no clang builtin for it, so the LLVM intrinsic is
// declared by name; the compiler then sees a real VALU instruction and places
// the wait states an SGPR written by a v_cmp needs before it.
extern "C" __device__ int fm_llvm_writelane_i32(int s, int l, int v) __asm("llvm.amdgcn.writelane.i32");
__device__ __forceinline__ int lane_put(int v, int l, int s) { return fm_llvm_writelane_i32(s, l, v); }

// One level of a transposing max-reduction: a and b each hold 64 per-lane
// candidates of their own metric; afterwards the lower lanes of every swapped
// span hold a's pairwise maxima and the upper lanes b's (v_permlane32_swap:
// halves of the wave, v_permlane16_swap: rows 0/1 and 2/3), so two registers
// become one per swap + max.
template <int S>
__device__ __forceinline__ float max_fold(float a, float b) {
  float lo, hi;
  const unsigned ua = __float_as_uint(a), ub = __float_as_uint(b);
  if constexpr (S == 32) {
    const auto r = __builtin_amdgcn_permlane32_swap(ua, ub, false, false);
    lo = __uint_as_float((unsigned)r[0]); hi = __uint_as_float((unsigned)r[1]);
  } else {
    static_assert(S == 16, "permlane swap strides");
    const auto r = __builtin_amdgcn_permlane16_swap(ua, ub, false, false);
    lo = __uint_as_float((unsigned)r[0]); hi = __uint_as_float((unsigned)r[1]);
  }
  return lo > hi ? lo : hi;
}

// The per-metric maxima of M registers of 64 per-lane candidates each (M = 8 or
// 4): lane m < M gets metric m's maximum in o_score (the other lanes 0), lane 0
// the service's in sbest.  lm = min(lane, M - 1).
template <int M>
__device__ __forceinline__ void fold_metric_max(const float (&bestm)[M], int lane, int lm, float& o_score,
                                                float& sbest) {
  static_assert(M == 8 || M == 4, "the reduction folds 8 or 4 registers");
  // fold the M registers into one whose 64 / M-lane groups each hold one
  // metric's candidates: group g = 2 r + h (M = 8: row r, half-row h) or row r
  // (M = 4) holds metric 4 h + rev(r), rev = {0, 2, 1, 3}
  float e;
  if constexpr (M == 8) {
    const float d0 = max_fold<16>(max_fold<32>(bestm[0], bestm[1]), max_fold<32>(bestm[2], bestm[3]));
    const float d1 = max_fold<16>(max_fold<32>(bestm[4], bestm[5]), max_fold<32>(bestm[6], bestm[7]));
    const bool upper = (lane & 8) != 0;
    const float keep = upper ? d1 : d0, send = upper ? d0 : d1;
    const float got = dpp_mov_all<0x128>(send);   // row_ror:8: the other half-row
    e = keep > got ? keep : got;
  } else {
    e = max_fold<16>(max_fold<32>(bestm[0], bestm[1]), max_fold<32>(bestm[2], bestm[3]));
    const float got = dpp_mov<0x118>(e, e);       // row_shr:8 (lanes 0-7 of a row keep their own)
    e = e > got ? e : got;
  }
  // inside a group: after row_shr 4, 2, 1 its last lane holds the maximum
  { const float g = dpp_mov<0x114>(e, e); e = e > g ? e : g; }
  { const float g = dpp_mov<0x112>(e, e); e = e > g ? e : g; }
  { const float g = dpp_mov<0x111>(e, e); e = e > g ? e : g; }
  // lane m fetches metric m's maximum from the last lane of its group
  const int q = lm & 3, rev = ((q & 1) << 1) | (q >> 1);
  const int src = M == 8 ? ((2 * rev + (lm >> 2)) * 8 + 7) : (rev * 16 + 15);
  o_score = __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(e)));
  if (lane >= M) o_score = 0.f;
  // the service maximum, into lane 0 (row_shl 4, 2, 1 over lanes 0 .. M-1)
  sbest = o_score;
  if constexpr (M == 8) { const float g = dpp_mov<0x104>(sbest, sbest); sbest = sbest > g ? sbest : g; }
  { const float g = dpp_mov<0x102>(sbest, sbest); sbest = sbest > g ? sbest : g; }
  { const float g = dpp_mov<0x101>(sbest, sbest); sbest = sbest > g ? sbest : g; }
}
