// Internal launchers of csrc/row_ops.hip (used by the decoder runtime).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace llm {

// pack = 1: int8 / fp16 outputs in packed-A order (common.hpp a_frag_off_*;
// needs cols % 64 == 0), consumed by the weight GEMMs with a_packed.
hipError_t launch_quantize_rows(const float* x, int rows, int cols, int8_t* q, float* inv,
                                hipStream_t st, int pack = 0);
struct LnSource;
// pp (optional): read the rows as embedding rows E[tok[r]] instead of x
// (gemm.hpp LnSource)
hipError_t launch_layernorm_quant(const float* x, int rows, int cols, const float* g,
                                  const float* b, float eps, float* out, int8_t* q, float* inv,
                                  hipStream_t st, int pack = 0, const LnSource* pp = nullptr);
hipError_t launch_layernorm_f16(const float* x, int rows, int cols, const float* g,
                                const float* b, float eps, void* out16, hipStream_t st,
                                int pack = 0, const LnSource* pp = nullptr);
hipError_t launch_to_f16(const float* x, size_t n, void* y, hipStream_t st, int pack_cols = 0);
hipError_t launch_advance(int32_t* pos, int32_t* ctx, int n, hipStream_t st);
hipError_t launch_argmax(const float* logits, int rows, int V, int32_t* out, int32_t* out2,
                         int out2_stride, hipStream_t st);
hipError_t launch_embed(const void* E, const int32_t* tok, int rows, int hid, int V, float* x,
                        hipStream_t st);
hipError_t launch_scatter_i32(int32_t* dst, const int64_t* idx, const int32_t* val, int n,
                              hipStream_t st);
// LM head (csrc/lm_head.hip): logits = x . E^T (E packed by launch_lm_pack); with part_val/part_idx also the
// per-(row, workgroup) first maxima that launch_argmax_partials reduces to ids.
int lm_head_workgroups(int V);
size_t lm_head_packed_bytes(int V, int K);
hipError_t launch_lm_pack(const void* E, void* P, int V, int K, hipStream_t st);  // E -> packed
hipError_t launch_lm_head(const float* x, const void* E, float* logits, int M, int V, int K,
                          float* part_val, int32_t* part_idx, hipStream_t st);
hipError_t launch_argmax_partials(const float* part_val, const int32_t* part_idx, int M, int nwg,
                                  int32_t* out, hipStream_t st, int32_t* pos = nullptr,
                                  int32_t* ctx = nullptr);
// The LM head with a log-softmax epilogue (lm_head_logprobs in llm_decoder.h)
// over a packed E: the partials launch and the merge launch on `st`, both
// capturable.  ws: device scratch of lm_head_logprobs_ws_floats(M, V) floats.
size_t lm_head_logprobs_ws_floats(int M, int V);
hipError_t launch_lm_head_logprobs(const float* x, const void* E, const int32_t* targets,
                                   float* logprob, float* stats, int M, int V, int K, float* ws,
                                   hipStream_t st);
// Chosen and top-n log-probabilities of materialised rows (csrc/logprobs.hip,
// logprob_rows in llm_decoder.h); one launch, capturable.
hipError_t launch_logprob_rows(const float* logits, int rows, int V, const int32_t* chosen,
                               int top_n, float* chosen_lp, float* top_lp, int32_t* top_id,
                               float* stats, hipStream_t st);
// Device sampling (csrc/sample.hip); counter[r] is the per-row draw counter.
hipError_t launch_sample(const float* logits, int rows, int row0, int V, float temperature,
                         int top_k, float top_p, uint64_t seed, const int32_t* counter,
                         int32_t* out, hipStream_t st);
// launch_sample with each row's own settings (device [rows] each; a NULL array
// takes sample_rows_each's default for it): the token choice of a serving step
hipError_t launch_sample_each(const float* logits, int rows, int V, const float* temperature,
                              const int32_t* top_k, const float* top_p, const uint64_t* seed,
                              const int32_t* counter, int32_t* out, hipStream_t st);
// Beam candidates (csrc/beam_select.hip, beam_select_rows in llm_decoder.h):
// the row stage and the merge stage on `st`, both capturable.  ws: device
// scratch of beam_select_ws_floats(num_seqs, W) floats (the row stage's
// m, log(s + 1e-6) and 2W (logit, token) pairs per row).
size_t beam_select_ws_floats(int num_seqs, int W);
hipError_t launch_beam_select(const float* logits, const float* score_in, int num_seqs, int W,
                              int V, float* cand_score, int32_t* cand_parent,
                              int32_t* cand_token, float* ws, hipStream_t st);
// pool[pairs[2i+1]] := pool[pairs[2i]] for i < n, pages of page_stride bytes
// (a multiple of 16) at pool + page * page_stride: one workgroup per pair,
// 16-byte loads and stores.  No destination may be another pair's source.
hipError_t launch_copy_pages(void* pool, size_t page_stride, const int32_t* pairs, int n,
                             hipStream_t st);
// Seeded uniform (variance-1 x scale) fp16 over `pages` pages of page_elems
// elements, page p at p + p * page_stride elements.
hipError_t launch_fill_random_f16(void* p, size_t pages, size_t page_elems, size_t page_stride,
                                  uint64_t seed, float scale, hipStream_t st);
// The same seeded values as LLM_FP8 bytes (csrc/fp8.hpp) at scale 1;
// page_stride in bytes.
hipError_t launch_fill_random_fp8(void* p, size_t pages, size_t page_elems, size_t page_stride,
                                  uint64_t seed, float scale, hipStream_t st);

}  // namespace llm
