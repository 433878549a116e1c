// Beam-search candidate selection on the device (beam_select_rows,
// include/llm_decoder.h): per decode step, the 2W best continuations of every
// sequence's W beams, ranked by cumulative log-probability.
//
// Row stage, one workgroup per row (the row in registers + LDS, RowVals of
// csrc/row_vals.hpp, as sample_rows_kernel holds it): m = max x and
// s = sum exp(x - m) reduced in a fixed order, then the row's 2W largest RAW
// logits in 2W rounds of block argmax (first maximum wins; the winner of a
// round is masked in the next round's pass).  Ranking inside a row never looks
// at a rounded log-probability, so W = 1 picks argmax_rows' id.  A row whose
// score is -inf (a beam that is not live) is not read.
// Merge stage, one wave per sequence: lane l holds candidate l of the W * 2W
// (<= 32), scores it score_in + ((x - m) - log(s + 1e-6)) and counts the
// lanes that rank before it by (score desc, parent asc, token asc) with
// read-lane broadcasts; rank < 2W writes slot `rank`.
// No atomics and no last-arriver hand-off: two launches, ordered
// by the stream, both capturable.
#include <algorithm>
#include <mutex>

#include "common.hpp"
#include "row_ops.hpp"
#include "row_vals.hpp"

namespace llm {

// per row: [0] m, [1] log(s + 1e-6), then 2W logits, then 2W token ids (as int bits)
__host__ __device__ __forceinline__ int beam_row_floats(int W) { return 2 + 4 * W; }

template <int VPT>
__global__ __launch_bounds__(kSampleThreads) void beam_rows_kernel(
    const float* __restrict__ logits, const float* __restrict__ score_in, int V, int W,
    float* __restrict__ ws) {
  __shared__ float shf[16];
  __shared__ int shi[16];
  extern __shared__ float spill[];
  const int r = blockIdx.x;
  float* out = ws + (size_t)r * beam_row_floats(W);
  const int K = 2 * W;
  if (score_in[r] == -INFINITY) {  // not a live beam (uniform over the workgroup)
    if ((int)threadIdx.x < K) {
      out[2 + threadIdx.x] = -INFINITY;
      out[2 + K + threadIdx.x] = __int_as_float((int)threadIdx.x);  // distinct ids
    }
    if (threadIdx.x == 0) { out[0] = 0.f; out[1] = 0.f; }
    return;
  }
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
  // (the slots past V hold -inf: exp(-inf - m) is exactly 0, so no bounds mask
  // here -- 56 lane masks kept from the load spilled SGPRs at VPT 128)
  p.each([&](int, float& v) { sloc += expf(v - m); });
  const float s = block_reduce(sloc, shf, [](float x, float y) { return x + y; });
  if (threadIdx.x == 0) { out[0] = m; out[1] = logf(s + 1e-6f); }

  int prev = -1;  // the previous round's winner, masked as this round's pass meets it
  for (int k = 0; k < K; ++k) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
    p.each([&](int i, float& v) {  // first max in the chunk
      if (base + i == prev) v = -INFINITY;
      if (v > best) { best = v; bi = base + i; }
    });
    const float bm = block_reduce(best, shf, [](float x, float y) { return fmaxf(x, y); });
    int cand = (best == bm) ? bi : 0x7fffffff;
    cand = block_reduce(cand, shi, [](int x, int y) { return min(x, y); });
    // (cand stays 0x7fffffff only when nothing finite is left: V >= 2W rules it
    // out for finite logits)
    prev = cand;
    if (threadIdx.x == 0) {
      out[2 + k] = bm;
      out[2 + K + k] = __int_as_float(cand == 0x7fffffff ? 0 : cand);
    }
  }
}

__global__ __launch_bounds__(64) void beam_merge_kernel(const float* __restrict__ ws,
                                                        const float* __restrict__ score_in,
                                                        int W, float* __restrict__ cand_score,
                                                        int32_t* __restrict__ cand_parent,
                                                        int32_t* __restrict__ cand_token) {
  const int sq = blockIdx.x;
  const int K = 2 * W, n = W * K;
  const int l = threadIdx.x;
  float sc = -INFINITY;
  int par = 0x7fffffff, tok = 0x7fffffff;
  if (l < n) {
    par = l / K;
    const int j = l - par * K;
    const int row = sq * W + par;
    const float* rw = ws + (size_t)row * beam_row_floats(W);
    tok = __float_as_int(rw[2 + K + j]);
    sc = score_in[row] + ((rw[2 + j] - rw[0]) - rw[1]);
  }
  int rank = 0;
  for (int k = 0; k < n; ++k) {  // n <= 32 broadcasts
    const float sk = __shfl(sc, k, 64);
    const int pk = __shfl(par, k, 64);
    const int tk = __shfl(tok, k, 64);
    rank += sk > sc || (sk == sc && (pk < par || (pk == par && tk < tok)));
  }
  if (l < n && rank < K) {
    cand_score[(size_t)sq * K + rank] = sc;
    cand_parent[(size_t)sq * K + rank] = par;
    cand_token[(size_t)sq * K + rank] = tok;
  }
}

template <int VPT>
static hipError_t launch_beam_rows_vpt(const float* logits, const float* score_in, int rows, int V,
                                       int W, float* ws, hipStream_t st) {
  constexpr size_t lds = (size_t)(VPT - RowVals<VPT>::R) * kSampleThreads * sizeof(float);
  if constexpr (lds > 65536) {
    static bool attr = false;
    if (!attr) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&beam_rows_kernel<VPT>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      attr = true;
    }
  }
  hipLaunchKernelGGL(beam_rows_kernel<VPT>, dim3(rows), dim3(kSampleThreads), lds, st, logits,
                     score_in, V, W, ws);
  return hipGetLastError();
}

size_t beam_select_ws_floats(int num_seqs, int W) {
  return (size_t)num_seqs * W * beam_row_floats(W);
}

hipError_t launch_beam_select(const float* logits, const float* score_in, int num_seqs, int W,
                              int V, float* cand_score, int32_t* cand_parent,
                              int32_t* cand_token, float* ws, hipStream_t st) {
  const int rows = num_seqs * W;
  const int vpt = (V + kSampleThreads - 1) / kSampleThreads;
  hipError_t e;
  if (vpt <= 16) e = launch_beam_rows_vpt<16>(logits, score_in, rows, V, W, ws, st);
  else if (vpt <= 32) e = launch_beam_rows_vpt<32>(logits, score_in, rows, V, W, ws, st);
  else if (vpt <= 64) e = launch_beam_rows_vpt<64>(logits, score_in, rows, V, W, ws, st);
  else if (vpt <= 128) e = launch_beam_rows_vpt<128>(logits, score_in, rows, V, W, ws, st);
  else return hipErrorInvalidValue;
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(beam_merge_kernel, dim3(num_seqs), dim3(64), 0, st, ws, score_in, W,
                     cand_score, cand_parent, cand_token);
  return hipGetLastError();
}

}  // namespace llm

using namespace llm;

extern "C" int beam_select_rows(const float* logits, const float* score_in, int num_seqs, int W,
                                int V, float* cand_score, int32_t* cand_parent,
                                int32_t* cand_token, void* stream) {
  LLM_REQUIRE(W >= 1 && W <= 4, "beam_select_rows: W must be in [1, 4]");
  LLM_REQUIRE(num_seqs >= 0 && num_seqs <= (1 << 20), "beam_select_rows: bad num_seqs");
  LLM_REQUIRE(V >= 2 * W, "beam_select_rows: V < 2W");
  LLM_REQUIRE(V <= 128 * kSampleThreads, "beam_select_rows: V > 65536");
  if (num_seqs == 0) return LLM_OK;
  LLM_REQUIRE(logits && score_in && cand_score && cand_parent && cand_token,
              "beam_select_rows: NULL pointer");
  // the row stage's scratch: kept by the library, grown (never shrunk) on demand
  static std::mutex mu;
  static float* ws = nullptr;
  static size_t cap = 0;
  std::lock_guard<std::mutex> g(mu);
  const size_t need = beam_select_ws_floats(num_seqs, W);
  if (need > cap) {
    if (ws) {
      LLM_HIP_RET(hipDeviceSynchronize());  // an earlier call may still read it
      LLM_HIP_RET(hipFree(ws));
      ws = nullptr;
      cap = 0;
    }
    const size_t want = std::max<size_t>(need, 4096);
    if (hipMalloc(&ws, want * sizeof(float)) != hipSuccess) {
      (void)hipGetLastError();
      ws = nullptr;
      return fail(LLM_ERR_OOM, "beam_select_rows: scratch allocation failed");
    }
    cap = want;
  }
  LLM_HIP_RET(launch_beam_select(logits, score_in, num_seqs, W, V, cand_score, cand_parent,
                                 cand_token, ws, as_stream(stream)));
  return LLM_OK;
}
