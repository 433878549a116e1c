// The sampling kernels' launch arguments and uniform draw: shared by the row
// kernel of csrc/sample.hip (the row held by one workgroup, V <= 65536) and the
// streaming kernel of csrc/sample_wide.hip (V <= 2^20).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace llm {

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// uniform in [0, 1) with 24 random bits (exactly representable in fp32)
__host__ __device__ __forceinline__ float sample_uniform(uint64_t seed, int row, int counter) {
  uint64_t z = seed ^ ((uint64_t)(uint32_t)row << 32) ^ (uint64_t)(uint32_t)counter;
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (float)(z >> 40) * (1.0f / 16777216.0f);
}

struct SampleArgs {
  const float* logits;
  int V;
  float temperature;
  int top_k;
  float top_p;
  uint64_t seed;
  const int32_t* counter;  // per-row draw counter (device), or NULL -> counter0
  int counter0;
  int row0;                // row id of this launch's first row (for the draw)
  int32_t* out;
  int32_t* out2;  // optional second destination (stride out2_stride)
  int out2_stride;
  // Optional per-row settings (device [rows]; NULL -> the scalar above), for
  // rows of different requests in one launch (continuous batching).  With
  // seed_v the draw's row term is 0: u = sample_uniform(seed_v[r], 0, counter),
  // so a request's draws depend on its seed and counter only, whichever row it
  // holds.
  const float* temperature_v;
  const int32_t* top_k_v;
  const float* top_p_v;
  const uint64_t* seed_v;
};

// The streaming forms (csrc/sample_wide.hip), any 1 <= V <= kWideMaxV
constexpr int kWideMaxV = 1 << 20;
hipError_t launch_sample_wide(const SampleArgs& a, int rows, hipStream_t st);
hipError_t launch_logprob_rows_wide(const float* logits, int rows, int V, const int32_t* chosen,
                                    int top_n, float* chosen_lp, float* top_lp, int32_t* top_id,
                                    float* stats, hipStream_t st);

}  // namespace llm
