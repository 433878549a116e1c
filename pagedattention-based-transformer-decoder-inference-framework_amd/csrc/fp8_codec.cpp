// Host codec of the LLM_FP8 KV element type (csrc/fp8.hpp): the C entries
// llm_fp8_e4m3_encode / llm_fp8_e4m3_decode.  No device call.
#include <cmath>

#include "common.hpp"
#include "fp8.hpp"

using namespace llm;

extern "C" int llm_fp8_e4m3_encode(const float* x, size_t n, float scale, uint8_t* out) {
  LLM_REQUIRE(n == 0 || (x && out), "llm_fp8_e4m3_encode: NULL pointer");
  LLM_REQUIRE(std::isfinite(scale) && scale > 0.f, "llm_fp8_e4m3_encode: scale must be finite and > 0");
  const float inv_scale = 1.0f / scale;
  for (size_t i = 0; i < n; ++i) out[i] = fp8_e4m3_encode_host(x[i] * inv_scale);
  return LLM_OK;
}

extern "C" int llm_fp8_e4m3_decode(const uint8_t* in, size_t n, float scale, float* out) {
  LLM_REQUIRE(n == 0 || (in && out), "llm_fp8_e4m3_decode: NULL pointer");
  LLM_REQUIRE(std::isfinite(scale) && scale > 0.f, "llm_fp8_e4m3_decode: scale must be finite and > 0");
  for (size_t i = 0; i < n; ++i) out[i] = fp8_e4m3_decode_host(in[i]) * scale;
  return LLM_OK;
}
