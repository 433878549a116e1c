// LLM_FP8 (OCP e4m3fn: bias 7, max +-448, no infinities, NaN = 0x7F / 0xFF) as
// a KV element type (include/llm_decoder.h, llm_dtype):
//   store: byte = cvt_e4m3_rne(clamp(y * inv_scale, -448, +448)), NaN -> NaN
//   load:  value = decode(byte) * scale
// Host encode / decode (the C entries llm_fp8_e4m3_encode / _decode use them)
// and the device forms over gfx950's conversion instructions.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

namespace llm {

constexpr float kFp8Max = 448.0f;

// One value, already multiplied by the inverse scale.  Round to nearest even in
// integer arithmetic (normals) / one fp32 add (subnormals: 2^14 has an ulp of
// 2^-9, the subnormal step), so the result does not depend on any conversion
// instruction.
inline uint8_t fp8_e4m3_encode_host(float x) {
  uint32_t b;
  std::memcpy(&b, &x, 4);
  const uint8_t sign = (uint8_t)((b >> 24) & 0x80u);
  uint32_t a = b & 0x7FFFFFFFu;
  if (a > 0x7F800000u) return sign | 0x7Fu;   // NaN
  if (a >= 0x43E00000u) return sign | 0x7Eu;  // |x| >= 448 (and inf): the explicit clamp
  if (a < 0x3C800000u) {                      // |x| < 2^-6: subnormal (or zero)
    float m;
    std::memcpy(&m, &a, 4);
    m += 16384.0f;
    uint32_t mb;
    std::memcpy(&mb, &m, 4);
    return sign | (uint8_t)(mb - 0x46800000u);  // 0..8 (8 = 2^-6, the smallest normal)
  }
  a += 0x7FFFFu + ((a >> 20) & 1u);  // nearest even at mantissa bit 20
  return sign | (uint8_t)((a >> 20) - (120u << 3));
}

inline float fp8_e4m3_decode_host(uint8_t c) {
  const uint32_t e = (c >> 3) & 15u, m = c & 7u;
  uint32_t b;
  if (e == 15u && m == 7u) {
    b = 0x7FC00000u;
  } else if (e == 0u) {
    const float v = (float)m * (1.0f / 512.0f);
    std::memcpy(&b, &v, 4);
  } else {
    b = ((e + 120u) << 23) | (m << 20);
  }
  b |= (uint32_t)(c & 0x80u) << 24;
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

#if defined(__HIPCC__)
// The byte of y at inverse scale inv_scale.  The clamp is explicit (fp32
// min / max before the convert, whose own overflow behaviour is never relied
// on); min / max drop a NaN, so it is routed round them.
__device__ __forceinline__ uint32_t fp8_e4m3_byte(float y, float inv_scale) {
  const float x = y * inv_scale;
  if (x != x) return 0x7Fu | ((__float_as_uint(x) >> 24) & 0x80u);
  const float c = fminf(fmaxf(x, -kFp8Max), kFp8Max);
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(c, c, 0, false) & 0xFFu;
}
#endif

}  // namespace llm
