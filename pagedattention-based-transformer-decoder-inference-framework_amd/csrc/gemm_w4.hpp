// Internal entry of csrc/gemm_w4.hip used by the decoder runtime: the W4A8
// weight GEMM (4-bit weights x int8 activations, exact int32 sums).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "llm_decoder.h"

namespace llm {

// One W4 weight GEMM (decoder-internal form of w4_gemm):
//   acc[m, n] = sum_k A[m, k] * (q[k, n] * mul[k / 128, n])      exact int32
//   C[m, n]   = act(float(acc) * (sa[m] * sw[n]) + bias[n])      two roundings
// A int8, row-major (lda) or packed-A (common.hpp a_frag_off_i8); W_packed from
// w4_pack_weights.  sa / sw / bias / acc_out / C may each be NULL.
struct W4Gemm {
  const int8_t* A = nullptr;
  int lda = 0;
  int a_packed = 0;
  const void* W_packed = nullptr;
  int M = 0, N = 0, K = 0;
  const float* sa = nullptr;
  const float* sw = nullptr;
  const float* bias = nullptr;
  int act = LLM_ACT_NONE;
  float* C = nullptr;
  int c_ld = 0;  // row stride of C (0: N)
  int32_t* acc_out = nullptr;
  int w_keep = 0;  // weights with the default cache policy (kept in the Infinity Cache), else nt
};

int w4_weight_gemm(const W4Gemm& g, hipStream_t st);

}  // namespace llm
