// Pod-major rows of the per-pod (K29) and drift (K31) canary tests: the pooled
// row is the current window's columns [0, n_cur), cut into pods by the row's
// cumulative segment ends (staged in LDS), and the baseline's columns after it.
#pragma once
#include "fm_lds_sort.h"

namespace fm {

// LDS written by some lanes of this wave is read by others (wave tier): the
// wave's LDS operations complete in order; this keeps the compiler from moving
// them across and waits for the stores.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The group of column i of the pooled row (0 = baseline, g + 1 = pod g, -1 =
// none): columns [0, n_cur) are the current window's, the baseline follows.
__device__ __forceinline__ int group_of(const unsigned* seg, int G, int i, int n_cur, int n_pooled) {
  if (i >= n_cur) return i < n_pooled ? 0 : -1;
  const int pod = count_le(seg, G, (unsigned)i);
  return pod < G ? pod + 1 : -1;
}

// group_of, and the column at which that group's segment starts (i itself for
// a column of no group, so that no earlier column counts as its segment's);
// whatever seg holds, 0 <= lo <= i.
__device__ __forceinline__ int segment_of(const unsigned* seg, int G, int i, int n_cur, int n_pooled, int& lo) {
  lo = i;
  if (i >= n_cur) {
    if (i >= n_pooled) return -1;
    lo = n_cur;
    return 0;
  }
  const int pod = count_le(seg, G, (unsigned)i);
  if (pod >= G) return -1;
  const unsigned s = pod ? seg[pod - 1] : 0u;
  lo = (int)(s < (unsigned)i ? s : (unsigned)i);
  return pod + 1;
}

}  // namespace fm
