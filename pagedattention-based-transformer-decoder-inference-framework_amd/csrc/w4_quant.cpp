// Host side of the 4-bit weight format (include/llm_decoder.h, "INT4
// weights"): the quantiser from per-column int8 weights, its inverse, and the
// reader of the device layout of csrc/gemm_w4.hip.  Plain C++, no device code.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <numeric>

#include "common.hpp"
#include "w4_quant.hpp"

namespace {
constexpr int kGroup = 128;
constexpr int kMaxMul = 18;  // 7 * 18 = 126 <= 127

inline int nibble_value(unsigned nib) { return (int)((nib & 0xFu) ^ 8u) - 8; }
}  // namespace

extern "C" int w4_quantize(const int8_t* W8, int K, int N, uint8_t* q, uint8_t* m) {
  LLM_REQUIRE(W8 && q && m, "w4_quantize: NULL operand");
  LLM_REQUIRE(K > 0 && K % kGroup == 0 && K < 131072 && N > 0,
              "w4_quantize: K must be a multiple of 128 below 131072");
  std::fill(q, q + (size_t)(K / 2) * N, (uint8_t)0);
  for (int g = 0; g < K / kGroup; ++g) {
    for (int n = 0; n < N; ++n) {
      const int8_t* col = W8 + (size_t)g * kGroup * N + n;
      int mx = 0, gcd = 0;
      for (int i = 0; i < kGroup; ++i) {
        const int v = std::abs((int)col[(size_t)i * N]);
        mx = std::max(mx, v);
        gcd = std::gcd(gcd, v);
      }
      // m = ceil(max / 7), at least 1 and at most 18 (a weight of +-127 / -128
      // rounds to +-7 * 18).  A group some multiplier reproduces exactly takes
      // the smallest such one, so representable weights are a fixed point.
      int mul = std::min(kMaxMul, std::max(1, (mx + 6) / 7));
      for (int c = mul; c <= kMaxMul; ++c)
        if (gcd % c == 0 && mx <= 7 * c) {
          mul = c;
          break;
        }
      m[(size_t)g * N + n] = (uint8_t)mul;
      for (int i = 0; i < kGroup; ++i) {
        const int k = g * kGroup + i;
        // rint of the exact quotient, ties to even (the default rounding mode)
        int v = (int)std::nearbyint((double)col[(size_t)i * N] / (double)mul);
        v = std::max(-7, std::min(7, v));
        q[(size_t)(k >> 1) * N + n] |= (uint8_t)((v & 0xF) << ((k & 1) * 4));
      }
    }
  }
  return LLM_OK;
}

extern "C" int w4_expand(const uint8_t* q, const uint8_t* m, int K, int N, int8_t* W8) {
  LLM_REQUIRE(W8 && q && m, "w4_expand: NULL operand");
  LLM_REQUIRE(K > 0 && K % kGroup == 0 && K < 131072 && N > 0,
              "w4_expand: K must be a multiple of 128 below 131072");
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < N; ++n) {
      const int v = nibble_value(q[(size_t)(k >> 1) * N + n] >> ((k & 1) * 4));
      W8[(size_t)k * N + n] = (int8_t)(v * (int)m[(size_t)(k / kGroup) * N + n]);
    }
  return LLM_OK;
}

// The expanded int8 [K][N] of a host copy of w4_pack_weights' output.
void llm::w4_unpack_host(const uint8_t* P, int K, int N, int8_t* W8) {
  const int G = K / kGroup, ntiles = N / 16;
  const uint8_t* mul = P + (size_t)ntiles * G * 1024;
  for (int nt = 0; nt < ntiles; ++nt)
    for (int g = 0; g < G; ++g) {
      const size_t blk = (size_t)nt * G + g;
      for (int lane = 0; lane < 64; ++lane) {
        const int n = nt * 16 + (lane & 15);
        const int mu = mul[blk * 16 + (lane & 15)];
        const int kb = g * kGroup + (lane >> 4) * 16;
        for (int i = 0; i < 16; ++i) {
          const unsigned b = P[(blk * 64 + lane) * 16 + i];
          W8[(size_t)(kb + i) * N + n] = (int8_t)(nibble_value(b) * mu);
          W8[(size_t)(kb + 64 + i) * N + n] = (int8_t)(nibble_value(b >> 4) * mu);
        }
      }
    }
}
