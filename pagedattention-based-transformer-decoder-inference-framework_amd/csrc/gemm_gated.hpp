// Internal entry of csrc/gemm_gated.hip used by the decoder runtime.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "llm_decoder.h"

namespace llm {

// One gated-MLP launch (decoder-internal form of i8_gemm_gated / f16_gemm_gated):
//   G = acc_gate[m, n] * (sa[m] * sw_gate[n]) + b_gate[n]   (F16: acc + bias)
//   U = acc_up[m, n]   * (sa[m] * sw_up[n])   + b_up[n]
//   H[m, n] = act(G) * U,  act = SiLU (LLM_MLP_GATED_SILU) or GELU (.._GELU)
// A row-major (lda) or packed-A (common.hpp a_frag_off_*); both weights in
// gemm_pack_weights' layout.  H (fp32 [M][N]) and H16 (fp16, packed-A order
// with ceil(N / 32) k-steps per row tile) may each be NULL; acc_gate / acc_up
// (I8: the exact int32 sums, [M][N]) too.
struct GatedGemm {
  int dtype = LLM_I8;
  const void* A = nullptr;
  int lda = 0;
  int a_packed = 0;
  const void* Wg_packed = nullptr;
  const void* Wu_packed = nullptr;
  int M = 0, N = 0, K = 0;
  const float* sa = nullptr;
  const float* sw_gate = nullptr;
  const float* sw_up = nullptr;
  const float* b_gate = nullptr;
  const float* b_up = nullptr;
  int mlp = LLM_MLP_GATED_SILU;
  float* H = nullptr;
  void* H16 = nullptr;
  int32_t* acc_gate = nullptr;
  int32_t* acc_up = nullptr;
  int w_keep = 0;  // weights with the default cache policy, else nt (WeightGemm::w_keep)
  // RMSNorm prologue (gated_rms_fusable rows only): A = RMSNorm(ln_x) with
  // ln_g / ln_eps, built per workgroup in LDS (I8: quantised per row, the row
  // scales replace sa); A / lda / a_packed / sa are then ignored.  act_out /
  // sa_out optionally receive the image (packed-A order) and the row scales.
  const float* ln_x = nullptr;
  const float* ln_g = nullptr;
  float ln_eps = 1e-5f;
  void* act_out = nullptr;
  float* sa_out = nullptr;
};

// `who` names the entry in error messages.  Every check runs on the host
// before the launch.
int gated_gemm(const GatedGemm& g, hipStream_t st, const char* who = "gated_gemm");
// Whether gated_gemm can run the RMSNorm prologue for M rows of K into N columns.
bool gated_rms_fusable(int dtype, int M, int N, int K);

}  // namespace llm
