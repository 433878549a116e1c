// One-wave-per-row LayerNorm (+ int8 quantisation) of the weight GEMM's
// LayerNorm prologue (gemm.hip), plus the quantise / fp16 helpers the
// LayerNorm launch (row_ops.hip layernorm_rows_kernel, 256 threads per row)
// shares with it.
//
// LayerNorm<T>::forward (decoder/layer_norm.hpp:20-37): biased variance,
// inv_std = 1.0 / sqrt(var + eps) (double division of the float sqrt), y =
// ((x - mean) * inv_std) * gamma + beta, every step rounded (no contraction);
// int8_quant.cpp:5-13,59-64: scale = 127 / (absmax + 1e-6), q = clamp(round(y *
// scale), -128, 127), dequantisation factor 1 / scale.
//
// Row layout per lane: float4 chunks c = 64 j + lane (j < CPL), i.e. lane l
// holds elements 4 (64 j + l) .. +3 — every load instruction of the wave reads
// 1 KiB contiguous (fully coalesced), and every output is one dword (4 int8)
// or 8 bytes (4 fp16) per chunk.  The reduction order does not depend on the
// output type, and any CPL that covers the row gives the same bits (empty
// chunks add exact zeros).  It is the LayerNorm launch's order (ln_row_sum:
// per-thread partials, the launch's four wave sums, then their fixed
// combination), so a row's LN, int8 image and scale are the same bits whether
// the launch or the GEMM prologue computes them -- whatever the batch size
// (tests/test_weight_gemm_gpu.py compares the taps bit for bit, K <= 2048).
#pragma once

#include "common.hpp"

namespace llm {

// Wave-wide max with DPP row moves (every lane ends with the maximum).
__device__ __forceinline__ float ln_wave_max(float x) {
  x = fmaxf(x, mov_dpp<0xB1>(x));   // quad_perm [1,0,3,2]
  x = fmaxf(x, mov_dpp<0x4E>(x));   // quad_perm [2,3,0,1]
  x = fmaxf(x, mov_dpp<0x141>(x));  // row_half_mirror
  x = fmaxf(x, mov_dpp<0x140>(x));  // row_mirror
  x = fmaxf(x, __shfl_xor(x, 16, 64));
  return fmaxf(x, __shfl_xor(x, 32, 64));
}

// DPP move into the lanes of the 4-lane banks in BANKS; the others keep `old`.
template <int CTRL, int BANKS>
__device__ __forceinline__ float ln_upd_dpp(float old, float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old),
                                                               __builtin_bit_cast(int, x), CTRL,
                                                               0xF, BANKS, false));
}

// The LayerNorm launch's block_sum_fast (row_ops.hip) in one wave: p[w] is
// this lane's partial of launch wave w (chunks [64 w, 64 w + 64); zeros past
// the row).  Each of the four sums pairs lane ^ 32, 16, 8, 4, 2, 1 in that
// order, as the launch's wave_sum does -- the same bits -- and the four run in
// lockstep, straight-line, so that their shuffles overlap: the prologue waits
// on these chains.  lane ^ 8 and lane ^ 4 are two banked row shifts each
// (row_shl: lane l reads l + n, row_shr: l - n) instead of shuffles through
// the LDS crossbar.
__device__ __forceinline__ float ln_row_sum(const float (&p)[4]) {
  float t[4] = {p[0], p[1], p[2], p[3]};
#pragma unroll
  for (int w = 0; w < 4; ++w) t[w] += __shfl_xor(t[w], 32, 64);
#pragma unroll
  for (int w = 0; w < 4; ++w) t[w] += __shfl_xor(t[w], 16, 64);
#pragma unroll
  for (int w = 0; w < 4; ++w)  // row_shl:8 | row_shr:8
    t[w] += ln_upd_dpp<0x118, 0xC>(ln_upd_dpp<0x108, 0x3>(t[w], t[w]), t[w]);
#pragma unroll
  for (int w = 0; w < 4; ++w)  // row_shl:4 | row_shr:4
    t[w] += ln_upd_dpp<0x114, 0xA>(ln_upd_dpp<0x104, 0x5>(t[w], t[w]), t[w]);
#pragma unroll
  for (int w = 0; w < 4; ++w) t[w] += mov_dpp<0x4E>(t[w]);  // quad_perm [2,3,0,1]
#pragma unroll
  for (int w = 0; w < 4; ++w) t[w] += mov_dpp<0xB1>(t[w]);  // quad_perm [1,0,3,2]
  return (t[0] + t[1]) + (t[2] + t[3]);
}

template <int CPL>
struct LnRow {
  f32x4 v[CPL];
};

// Issue the loads of one row of K4 float4 chunks (!ok: zeros).
template <int CPL>
__device__ __forceinline__ void ln_wave_load(const float* __restrict__ row, int K4, bool ok,
                                             LnRow<CPL>& r) {
  const int lane = lane_id();
  const f32x4* row4 = reinterpret_cast<const f32x4*>(row);
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int c = 64 * j + lane;
    r.v[j] = (ok && c < K4) ? row4[c] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// The same chunks from an fp16 row (an embedding row: TokenEmbedding::forward,
// decoder/token_embedding.hpp:19-26, widened exactly).
template <int CPL>
__device__ __forceinline__ void ln_wave_load_f16(const _Float16* __restrict__ row, int K4, bool ok,
                                                 LnRow<CPL>& r) {
  const int lane = lane_id();
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  const h4* row4 = reinterpret_cast<const h4*>(row);
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int c = 64 * j + lane;
    const h4 h = (ok && c < K4) ? row4[c] : h4{0, 0, 0, 0};
    r.v[j] = f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
  }
}

// Embedding row of token id tok (clamped to [0, V), as embed_kernel).
__device__ __forceinline__ const _Float16* ln_embed_row(const _Float16* E, const int32_t* tok,
                                                        int m, int V, int K) {
  int t = tok[m];
  t = t < 0 ? 0 : (t >= V ? V - 1 : t);
  return E + (size_t)t * K;
}

// x -> LN(x) in place; returns the row's |max| (wave-uniform).
template <int CPL>
__device__ __forceinline__ float ln_wave_compute(LnRow<CPL>& x, const LnRow<CPL>& gm,
                                                 const LnRow<CPL>& bt, int K, float eps) {
  const int lane = lane_id();
  const int K4 = K >> 2;
  // Lane l's chunk j = w + 4 i is chunk i of thread 64 w + l of the launch
  // (chunk c = threadIdx.x + 256 i): the same per-thread partials, summed per
  // launch wave w and combined as the launch does.  A chunk the launch's
  // thread does not hold (VPT 1 at K <= 1024) lies past the row: it adds an
  // exact +0 to a partial that is never -0, and the variance skips it.
  float p[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    p[w] = 0.f;
#pragma unroll
    for (int i = 0; w + 4 * i < CPL; ++i) {
      const int j = w + 4 * i;
      p[w] += (x.v[j][0] + x.v[j][1]) + (x.v[j][2] + x.v[j][3]);
    }
  }
  const float mean = ln_row_sum(p) / (float)K;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    p[w] = 0.f;
#pragma unroll
    for (int i = 0; w + 4 * i < CPL; ++i) {
      const int j = w + 4 * i;
      if (64 * j + lane >= K4) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = x.v[j][e] - mean;
        p[w] = fmaf(d, d, p[w]);
      }
    }
  }
  const float var = ln_row_sum(p) / (float)K;
  const float inv_std = (float)(1.0 / (double)sqrtf(var + eps));
  float am = 0.f;
#pragma unroll
  for (int j = 0; j < CPL; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float y = __fmul_rn(__fmul_rn(x.v[j][e] - mean, inv_std), gm.v[j][e]);
      x.v[j][e] = __fadd_rn(y, bt.v[j][e]);
      am = fmaxf(am, fabsf(x.v[j][e]));  // empty chunks: beta 0 -> 0
    }
  return ln_wave_max(am);
}

// 4 values -> 4 int8 in one dword (int8_quant.cpp quantize_to_int8 semantics)
__device__ __forceinline__ uint32_t ln_quant4(f32x4 y, float scale) {
  uint32_t wd = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float t = roundf(__fmul_rn(y[e], scale));
    t = fminf(fmaxf(t, -128.f), 127.f);
    wd |= (uint32_t)(uint8_t)(int8_t)(int)t << (8 * e);
  }
  return wd;
}

typedef _Float16 ln_f16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ ln_f16x4 ln_half4(f32x4 y) {
  return ln_f16x4{(_Float16)y[0], (_Float16)y[1], (_Float16)y[2], (_Float16)y[3]};
}

}  // namespace llm
