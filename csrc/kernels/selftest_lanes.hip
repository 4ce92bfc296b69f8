#include "fm_common.h"

using namespace fm;

// ---------------------------------------------------------------------------
// Self-test of the cross-lane primitives (one wave): the DPP / permlane-swap
// encodings are checked against their definitions by tests/test_canary_ops.py.
// out [12][64]: xor 1,2,4,8,16,32 | incl sum | incl max | suffix min | prev |
// next | wave sum
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void selftest_lanes_kernel(const int* __restrict__ in, int* __restrict__ out) {
  const int l = lane_id();
  const int v = in[l];
  out[0 * 64 + l] = xor_lane<1>(v);
  out[1 * 64 + l] = xor_lane<2>(v);
  out[2 * 64 + l] = xor_lane<4>(v);
  out[3 * 64 + l] = xor_lane<8>(v);
  out[4 * 64 + l] = xor_lane<16>(v);
  out[5 * 64 + l] = xor_lane<32>(v);
  out[6 * 64 + l] = wave_incl_sum(v);
  out[7 * 64 + l] = wave_incl_max(v, (int)0x80000000);
  out[8 * 64 + l] = wave_incl_suffix_min(v, 0x7fffffff);
  out[9 * 64 + l] = lane_prev(v, -1);
  out[10 * 64 + l] = lane_next(v, -2);
  out[11 * 64 + l] = wave_sum(v);
}

FM_API int fm_selftest_lanes(const int* in, int* out, hipStream_t stream) {
  hipLaunchKernelGGL(selftest_lanes_kernel, dim3(1), dim3(64), 0, stream, in, out);
  FM_LAUNCH_CHECK();
  return 0;
}
