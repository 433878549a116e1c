// Tuning build only (make tune -> libllm_decoder_hip_tune.so; never in
// libllm_decoder_hip.so): C entries over the internal row-kernel launchers in
// the forms the decoder runs them (packed-A outputs, the embedding source, the
// zeroing source, fp16 outputs), for tests/test_row_ops_gpu.py.  No kernel
// code here: every entry forwards to a launcher of csrc/row_ops.hip.
#include "common.hpp"
#include "gemm.hpp"
#include "row_ops.hpp"

using namespace llm;

// emb != NULL: rows are E[clamp(tok[r])] (x unused); zero_x: see gemm.hpp LnSource.
static LnSource ln_source(const void* emb, const int32_t* tok, int V, float* zero_x) {
  LnSource s{};
  s.emb = static_cast<const _Float16*>(emb);
  s.tok = tok;
  s.V = V;
  s.zero_x = zero_x;
  return s;
}

extern "C" int layernorm_quant_tune(const float* x, int rows, int cols, const float* gamma,
                                    const float* beta, float eps, float* out, int8_t* q,
                                    float* inv_scale, int pack, const void* emb,
                                    const int32_t* tok, int V, float* zero_x, void* stream) {
  LLM_REQUIRE(rows > 0 && cols > 0 && cols <= 16384, "layernorm_quant_tune: shape");
  LLM_REQUIRE((x || emb) && gamma && beta && (out || q), "layernorm_quant_tune: NULL pointer");
  LLM_REQUIRE((q == nullptr) == (inv_scale == nullptr), "layernorm_quant_tune: q and inv_scale");
  LLM_REQUIRE(!emb || (tok && V > 0), "layernorm_quant_tune: emb needs tok and V");
  const LnSource s = ln_source(emb, tok, V, zero_x);
  hipError_t e = launch_layernorm_quant(x, rows, cols, gamma, beta, eps, out, q, inv_scale,
                                        as_stream(stream), pack, &s);
  return e == hipSuccess ? LLM_OK : fail(LLM_ERR_HIP, "layernorm_quant_tune");
}

extern "C" int layernorm_f16_tune(const float* x, int rows, int cols, const float* gamma,
                                  const float* beta, float eps, void* out16, int pack,
                                  const void* emb, const int32_t* tok, int V, float* zero_x,
                                  void* stream) {
  LLM_REQUIRE(rows > 0 && cols > 0 && cols <= 16384, "layernorm_f16_tune: shape");
  LLM_REQUIRE((x || emb) && gamma && beta && out16, "layernorm_f16_tune: NULL pointer");
  LLM_REQUIRE(!emb || (tok && V > 0), "layernorm_f16_tune: emb needs tok and V");
  const LnSource s = ln_source(emb, tok, V, zero_x);
  hipError_t e = launch_layernorm_f16(x, rows, cols, gamma, beta, eps, out16, as_stream(stream),
                                      pack, &s);
  return e == hipSuccess ? LLM_OK : fail(LLM_ERR_HIP, "layernorm_f16_tune");
}

extern "C" int quantize_rows_tune(const float* x, int rows, int cols, int8_t* q, float* inv_scale,
                                  int pack, void* stream) {
  LLM_REQUIRE(rows > 0 && cols > 0, "quantize_rows_tune: shape");
  LLM_REQUIRE(x && q && inv_scale, "quantize_rows_tune: NULL pointer");
  hipError_t e = launch_quantize_rows(x, rows, cols, q, inv_scale, as_stream(stream), pack);
  return e == hipSuccess ? LLM_OK : fail(LLM_ERR_HIP, "quantize_rows_tune");
}

// pack_cols > 0: y in packed-A fp16 order of rows of pack_cols (n a multiple of it).
extern "C" int to_f16_tune(const float* x, size_t n, void* y, int pack_cols, void* stream) {
  LLM_REQUIRE(x && y, "to_f16_tune: NULL pointer");
  LLM_REQUIRE(pack_cols >= 0 && (pack_cols == 0 || n % (size_t)pack_cols == 0), "to_f16_tune: shape");
  hipError_t e = launch_to_f16(x, n, y, as_stream(stream), pack_cols);
  return e == hipSuccess ? LLM_OK : fail(LLM_ERR_HIP, "to_f16_tune");
}
