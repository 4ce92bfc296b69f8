#include "fm_common.h"

using namespace fm;

// ---------------------------------------------------------------------------
// K11: synthetic Prometheus-shaped fleet.  Deterministic in the GLOBAL service
// id so every world size sees the same fleet (docs/BRAIN_SPEC.md, "synthetic
// fleet"); mirrors the daily/weekly seasonality + noise + injected faults of
// examples/spring-boot-demo/src/main/resources/load.txt.
// ---------------------------------------------------------------------------
struct SynthParams {
  float level, amp_d, amp_w, phase, noise;
};

__host__ __device__ __forceinline__ SynthParams synth_params(uint32_t gs, uint32_t m, uint32_t seed) {
  const uint32_t key = gs * 64u + m;
  SynthParams p;
  p.level = 1.0f + 99.0f * u01(hash3(key, 0u, seed));
  p.amp_d = 0.1f + 0.3f * u01(hash3(key, 1u, seed));
  p.amp_w = 0.01f + 0.04f * u01(hash3(key, 2u, seed));
  p.phase = 6.2831853f * u01(hash3(key, 3u, seed));
  p.noise = 0.005f + 0.015f * u01(hash3(key, 4u, seed));
  return p;
}

__device__ __forceinline__ float synth_value(const SynthParams& p, uint32_t key, int64_t t, uint32_t stream_id,
                                             uint32_t seed) {
  const float tf = (float)t;
  const float season = 1.0f + p.amp_d * sinf(6.2831853f * tf / 1440.0f + p.phase) +
                       p.amp_w * sinf(6.2831853f * tf / 10080.0f + p.phase);
  const uint32_t h1 = hash3(key, (uint32_t)t * 2654435761u + stream_id, seed ^ 0xA5A5A5A5u);
  const uint32_t h2 = hash_u32(h1 ^ 0x68E31DA4u);
  const float g = sqrtf(-2.0f * logf(u01(h1))) * cosf(6.2831853f * u01(h2));
  float v = p.level * season * (1.0f + p.noise * g);
  return v > 0.f ? v : 0.f;
}

// kind: 0 = history [R, ld] for t in [0, T); 1 = baseline (P pods x W points,
// t in [T-W, T)); 2 = current (P pods x W points, t in [T, T+W)) with faults
// injected into services whose hash falls under fault_rate.
__global__ void synth_kernel(float* __restrict__ out, int64_t ld, int64_t n_per_row, int64_t S, int M,
                             int64_t svc0, int T, int P, int W, int kind, float fault_rate, float fault_mag,
                             uint32_t seed) {
  const int64_t total = S * M * n_per_row;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = e / n_per_row;
    const int64_t j = e - row * n_per_row;
    const uint32_t gs = (uint32_t)(svc0 + row / M);
    const uint32_t m = (uint32_t)(row % M);
    const SynthParams p = synth_params(gs, m, seed);
    const uint32_t key = gs * 64u + m;
    float v;
    if (kind == 0) {
      v = synth_value(p, key, j, 0u, seed);
    } else {
      const int64_t pod = j / W, w = j - pod * W;
      const int64_t t = (kind == 1) ? (T - W + w) : (T + w);
      v = synth_value(p, key, t, 1000u + (uint32_t)pod + (kind == 2 ? 500u : 0u), seed);
      if (kind == 2) {
        const bool faulty = u01(hash3(gs, 7u, seed)) < fault_rate;
        if (faulty && (m % 4u) == 0u) v = v + p.level * fault_mag * (1.0f + p.amp_d + p.amp_w);
      }
    }
    out[row * ld + j] = v;
  }
  // padding columns of the history are NaN (missing samples)
  if (kind == 0 && ld > n_per_row) {
    const int64_t pad = ld - n_per_row;
    const int64_t tp = S * M * pad;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < tp; e += (int64_t)gridDim.x * blockDim.x) {
      const int64_t row = e / pad;
      out[row * ld + n_per_row + (e - row * pad)] = NAN;
    }
  }
}

FM_API int fm_synth_fleet(float* out, int64_t ld, int64_t n_per_row, int64_t S, int M, int64_t svc0, int T, int P,
                          int W, int kind, float fault_rate, float fault_mag, uint32_t seed, hipStream_t stream) {
  if (S <= 0) return 0;
  hipLaunchKernelGGL(synth_kernel, dim3(2048), dim3(256), 0, stream, out, ld, n_per_row, S, M, svc0, T, P, W, kind,
                     fault_rate, fault_mag, seed);
  FM_LAUNCH_CHECK();
  return 0;
}
