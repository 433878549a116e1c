// Log-probabilities of materialised logits rows (logprob_rows,
// include/llm_decoder.h): the chosen token's and the row's top-n, always of the
// raw logits (temperature 1, before top-k / top-p).
//
// One workgroup per row, the row in registers + LDS (RowVals of
// csrc/row_vals.hpp, as sample_rows_kernel and beam_rows_kernel hold it):
// m = max x and s = sum exp(x - m) reduced in a fixed order, lse = log(s + 1e-6)
// and logprob(t) = (x_t - m) - lse -- beam_rows_kernel's term, so a served
// token's value and a beam hypothesis's sum_logprob mean the same thing.
// The top-n are n rounds of block argmax over the entries that rank strictly
// after the previous round's winner in (logit descending, token id ascending):
// nothing is masked, so -inf entries keep their place (by id) at the end of the
// order.  Ranking never looks at a rounded log-probability.
#include <algorithm>

#include "common.hpp"
#include "row_ops.hpp"
#include "row_vals.hpp"

namespace llm {

template <int VPT>
__global__ __launch_bounds__(kSampleThreads) void logprob_rows_kernel(
    const float* __restrict__ logits, int V, const int32_t* __restrict__ chosen, int top_n,
    float* __restrict__ chosen_lp, float* __restrict__ top_lp, int32_t* __restrict__ top_id,
    float* __restrict__ stats) {
  __shared__ float shf[16];
  __shared__ int shi[16];
  extern __shared__ float spill[];
  const int r = blockIdx.x;
  const float* lg = logits + (size_t)r * V;
  const int base = threadIdx.x * VPT;
  RowVals<VPT> p;
  p.lds = spill;
  float mloc = -INFINITY;
  p.each([&](int i, float& v) {
    v = base + i < V ? lg[base + i] : -INFINITY;
    mloc = fmaxf(mloc, v);
  });
  const float m = block_reduce(mloc, shf, [](float x, float y) { return fmaxf(x, y); });
  float sloc = 0.f;
  // (the slots past V hold -inf: exp(-inf - m) is exactly 0, as in beam_rows_kernel)
  p.each([&](int, float& v) { sloc += expf(v - m); });
  const float s = block_reduce(sloc, shf, [](float x, float y) { return x + y; });
  const float lse = logf(s + 1e-6f);
  if (threadIdx.x == 0) {
    if (stats) { stats[2 * r] = m; stats[2 * r + 1] = lse; }
    if (chosen) {
      const int c = chosen[r];
      chosen_lp[r] = c >= 0 && c < V ? (lg[c] - m) - lse : 0.f;
    }
  }

  float pv = INFINITY;  // the previous round's winner: (value, id)
  int pid = -1;
  for (int k = 0; k < top_n; ++k) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
    p.each([&](int i, float& v) {  // first maximum of the chunk's entries after (pv, pid)
      const int id = base + i;
      const bool after = id < V && (v < pv || (v == pv && id > pid));
      if (after && (v > best || bi == 0x7fffffff)) { best = v; bi = id; }
    });
    const float bm = block_reduce(best, shf, [](float x, float y) { return fmaxf(x, y); });
    int cand = (best == bm) ? bi : 0x7fffffff;  // (a thread with no entry left holds 0x7fffffff)
    cand = block_reduce(cand, shi, [](int x, int y) { return min(x, y); });
    // (V >= top_n: an entry is left in every round, unless the row holds NaN)
    pv = bm;
    pid = cand;
    if (threadIdx.x == 0) {
      top_id[(size_t)r * top_n + k] = cand == 0x7fffffff ? 0 : cand;
      top_lp[(size_t)r * top_n + k] = (bm - m) - lse;
    }
  }
}

template <int VPT>
static hipError_t launch_logprob_rows_vpt(const float* logits, int rows, int V,
                                          const int32_t* chosen, int top_n, float* chosen_lp,
                                          float* top_lp, int32_t* top_id, float* stats,
                                          hipStream_t st) {
  constexpr size_t lds = (size_t)(VPT - RowVals<VPT>::R) * kSampleThreads * sizeof(float);
  if constexpr (lds > 65536) {
    static bool attr = false;
    if (!attr) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&logprob_rows_kernel<VPT>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      attr = true;
    }
  }
  hipLaunchKernelGGL(logprob_rows_kernel<VPT>, dim3(rows), dim3(kSampleThreads), lds, st, logits,
                     V, chosen, top_n, chosen_lp, top_lp, top_id, stats);
  return hipGetLastError();
}

hipError_t launch_logprob_rows(const float* logits, int rows, int V, const int32_t* chosen,
                               int top_n, float* chosen_lp, float* top_lp, int32_t* top_id,
                               float* stats, hipStream_t st) {
  const int vpt = (V + kSampleThreads - 1) / kSampleThreads;
  if (vpt <= 16)
    return launch_logprob_rows_vpt<16>(logits, rows, V, chosen, top_n, chosen_lp, top_lp, top_id, stats, st);
  if (vpt <= 32)
    return launch_logprob_rows_vpt<32>(logits, rows, V, chosen, top_n, chosen_lp, top_lp, top_id, stats, st);
  if (vpt <= 64)
    return launch_logprob_rows_vpt<64>(logits, rows, V, chosen, top_n, chosen_lp, top_lp, top_id, stats, st);
  if (vpt <= 128)
    return launch_logprob_rows_vpt<128>(logits, rows, V, chosen, top_n, chosen_lp, top_lp, top_id, stats, st);
  return hipErrorInvalidValue;
}

}  // namespace llm

using namespace llm;

extern "C" int logprob_rows(const float* logits, int rows, int V, const int32_t* chosen, int top_n,
                            float* chosen_lp, float* top_lp, int32_t* top_id, float* stats,
                            void* stream) {
  LLM_REQUIRE(top_n >= 0 && top_n <= LLM_MAX_TOP_LOGPROBS, "logprob_rows: top_n must be in [0, 8]");
  LLM_REQUIRE(rows >= 0 && V >= std::max(1, top_n), "logprob_rows: V < max(1, top_n)");
  LLM_REQUIRE(V <= 128 * kSampleThreads, "logprob_rows: V > 65536");
  if (rows == 0) return LLM_OK;
  LLM_REQUIRE(logits && (!chosen || chosen_lp) && (top_n == 0 || (top_lp && top_id)),
              "logprob_rows: NULL pointer");
  LLM_HIP_RET(launch_logprob_rows(logits, rows, V, chosen, top_n, chosen_lp, top_lp, top_id, stats,
                                  as_stream(stream)));
  return LLM_OK;
}
