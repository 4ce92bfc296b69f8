// Right-looking Cholesky of a matrix of up to 32 columns held in registers, one
// column a lane, in fp64.  Shared by K36 (lsq_robust.hip: the 32 x 32 Gram of a
// row's fit with its right-hand side as a 33rd row) and K37 (mvn_wide.hip: the
// correlation matrix of a group's members).
#pragma once
#include "fm_common.h"

namespace fm {

__device__ __forceinline__ double bcast_f64(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                          __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// Lane j (and lane j + 32, which holds the same column) carries column j of a
// symmetric positive definite N x N matrix in a[0 .. N) and NR - N further rows
// below it (an augmented right-hand side g turns into y = L^-1 g).  Step k:
// lane k scales its column to L[:, k] and keeps 1 / L[k][k] in a[k]; lane j > k
// subtracts L[i][k] L[j][k] from all of its column (the full symmetric matrix
// is carried, so L[j][k] is its own a[k]).  The pivot column is broadcast by
// readlane.  On return a[i] = L[i][j] for i > j and a[j] = 1 / L[j][j]; a pivot
// that is not positive gives a zero column.
template <int N, int NR>
__device__ __forceinline__ void chol_columns(double (&a)[NR], int j) {
  static_assert(N <= 32 && NR >= N, "one column a lane of a half wave");
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double pk = bcast_f64(a[k], k);
    const double inv = pk > 0.0 ? 1.0 / sqrt(pk) : 0.0;
    const double cj = j > k ? a[k] * inv : 0.0;
    const double scl = j == k ? inv : 1.0;
    a[k] = j == k ? inv : a[k];
#pragma unroll
    for (int i = k + 1; i < NR; ++i) {
      a[i] *= scl;
      const double ci = bcast_f64(a[i], k);
      a[i] = fma(-ci, cj, a[i]);
    }
  }
}

}  // namespace fm
