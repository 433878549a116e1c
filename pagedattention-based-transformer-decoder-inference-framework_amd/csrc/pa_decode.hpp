// Internal entry of the paged decode attention (csrc/pa_decode.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "llm_decoder.h"
#include "pa_plan.hpp"

namespace llm {

// Optional per-row conversions of the attention output fused into the split
// merge (the o_proj input): int8 + inv_scale (per-row quantisation) and/or fp16.
struct PaRowOutputs {
  int8_t* q = nullptr;
  float* inv_scale = nullptr;
  void* out16 = nullptr;
  int pack = 0;  // q / out16 in packed-A order (common.hpp a_frag_off_*)
  int keep_out = 1;  // 0: a split launch skips the fp32 `out` rows (only q / out16 are read)
  // FP16 decoder, fused o_proj (workgroup-merge launches only, pa_decode_plan
  // form LLM_PA_FORM_WG_MERGE | LLM_PA_FORM_OPROJ): each (row, head)
  // workgroup multiplies its merged head (rounded to fp16, as the o_proj
  // input) by W_o's rows of that head and adds the o_n products into o_acc
  // row b with atomics (counted fixed point, common.hpp oacc_term; all zero
  // between launches); the adder completing a column writes o_x[b][n] (fp32,
  // what the o_proj GEMM would have written) and clears the column.
  // wo_heads: fp16 [H][D/8][o_n][8] (8 consecutive k of one column per 16 bytes).
  long long* o_acc = nullptr;
  float* o_x = nullptr;
  const void* wo_heads = nullptr;
  int o_n = 0;
  // device int set to 1 when a head's term left the accumulator's range and was
  // clamped (common.hpp oacc_term); required with o_acc
  int* o_flag = nullptr;
  // Beam-group launches (row_group 4, fp16 KV): 2 * ceil(B / 4) * H counters,
  // zero before the first launch and left at zero by every launch; with them
  // the launch assigns tiles dynamically (csrc/tune/pa_beam_steal.hpp,
  // LLM_PA_FORM_STEAL), without them it runs the static BEAM form
  unsigned* beam_ctr = nullptr;
  // LLM_FP8 pools: the layer's V scale, multiplied into the normalised output
  // once per (row, head) by every launch form, before any of the conversions
  // above rounds it (K's scale is the caller's to fold into sm_scale)
  float out_scale = 1.f;
};

// Bytes per element of a KV pool type (0: unknown type).
constexpr int kv_elem_size(int kvt) {
  return kvt == LLM_F16 || kvt == LLM_BF16 ? 2
         : kvt == LLM_F32                  ? 4
         : kvt == LLM_I8 || kvt == LLM_FP8 ? 1
                                           : 0;
}

// The request (pa_plan.hpp) of a launch over a view's pages.
inline PaRequest pa_request(const pa_kv_view* kv, int B, int H, int D, int T, int pages_per_split,
                            int row_group = 1, PaOut out = PaOut::F32, int window = 0) {
  PaRequest rq;
  rq.B = B, rq.H = H, rq.D = D, rq.T = T;
  if (kv) rq.TS = kv->page_size, rq.max_tiles = kv->max_tiles, rq.kv_dtype = kv->kv_dtype;
  rq.pps_fixed = pages_per_split > 0 ? std::min(pages_per_split, kMaxPps) : 0;
  rq.row_group = row_group;
  rq.out = out;
  rq.window = window;
  return rq;
}

// pa_plan on this device: the resident-wave counts come from occupancy queries
// of the kernels the launch would run (cached), made only for dynamic splits.
// A count >= 0 given here replaces its query (tests).  LLM_ERR_UNSUPPORTED as
// pa_plan, and for a shape no split kernel is built for; sets no error text.
int pa_plan_device(const PaRequest& rq, PaLaunch* launch, long long resident = -1,
                   long long beam_resident = -1, long long beam4_resident = -1);

// Runs the launch pa_plan_device gives for rq over kv.  q has a row stride (the
// decoder reads q in place from the fused qkv projection output, rows of 3*hid
// floats).  rq.out says what comes back: F32 in `out`, every other kind through
// the pointers of `rows` (F32_ROWS: `out`, as rows [B][H*D]); `out` may be NULL
// when rows are asked for and the launch splits.
// plan != NULL: only report the launch (no pointer but kv's is read).
int pa_decode_internal(const pa_kv_view* kv, const PaRequest& rq, const float* q, int q_stride,
                       float* out, const int32_t* beam_ids, const int32_t* context_lens,
                       float sm_scale, void* workspace, size_t workspace_bytes, hipStream_t st,
                       const PaRowOutputs* rows = nullptr, PaLaunch* plan = nullptr);
int pa_pages_per_split(int B, int H, int T, int TS, int max_tiles);
// Whether the FP16 decoder fuses its o_proj into the attention's workgroup
// merge (PaRowOutputs::o_acc); always in the product build.
bool oproj_fuse_on();

// Whether the decoder's beam launches assign tiles while they run
// (PaRowOutputs::beam_ctr, csrc/tune/pa_beam_steal.hpp): tuning build, LLM_BEAM_STEAL=1
// (same-box it lost to the static BEAM form).
bool beam_steal_on();

// Split merge of per-(row, head, split) partial softmax states into rows
// (out fp32 [B][H*D] and/or the rows->q / out16 o_proj inputs); row b's
// context is context_lens[b], or ctx_p0 + b + 1 when context_lens is NULL and
// ctx_p0 >= 0, or T.  Split s of a row covers tiles [s*pps, (s+1)*pps), counted
// from the row's first live tile under `window` (pa_split.hpp row_span; 0: none).
// out_scale multiplies every merged head (LLM_FP8 pools: the V scale).
int pa_merge_rows_internal(const float* part_acc, const float* part_ml, float* out,
                           const PaRowOutputs* rows, const int32_t* context_lens, int ctx_p0,
                           int B, int H, int D, int T, int TS, int pps, int nsplit, int max_tiles,
                           hipStream_t st, float out_scale = 1.f, int window = 0);

int pa_merge_splits_internal(const float* part_acc, const float* part_ml, float* out,
                             const int32_t* context_lens, int B, int H, int D, int T, int TS,
                             int pps, int nsplit, int max_tiles, hipStream_t st,
                             float out_scale = 1.f, int window = 0);

// Causal MFMA attention of a prompt chunk (csrc/pa_prefill.hip, C entry
// pa_prefill): out rows i < m = attention of query i (position p0 + i) over
// positions 0 .. p0 + i of page-table row `row`.
// With workspace (pa_prefill_workspace_bytes) the key range is split over
// workgroups and merged by pa_merge_rows_internal, which also writes `rows`
// (the o_proj input); without, one pass writes out and `rows` is converted by
// the row quantiser.  `out` may be NULL only when it splits and rows is set.
// The split form is refused for H*D > 16384 (the merge's LDS row).
// window > 0: query i attends to positions max(0, p0 + i - window + 1) .. p0 + i.
bool pa_prefill_supported(const pa_kv_view* kv);
size_t pa_prefill_ws_bytes(const pa_kv_view* kv, int p0, int m);
int pa_prefill_internal(const pa_kv_view* kv, const float* q, int q_stride, float* out,
                        int out_stride, int row, int p0, int m, float sm_scale, void* workspace,
                        size_t workspace_bytes, hipStream_t st, const PaRowOutputs* rows = nullptr,
                        int window = 0);

// The packed form (C entry pa_prefill_packed): m dense rows of q / out made of
// segments of several sequences, driven by a device tile table
// tiles_dev[ntile][4] = {q0, nq, row, p0} (pa_prefill_packed_tiles) and the
// rows' device context lengths ctx_dev[m] (position + 1); maxend = the longest
// segment's end.  part_ws (pa_prefill_packed_part_bytes, or the bound over any
// launch of up to max_rows rows) selects the split form as workspace does above.
size_t pa_prefill_packed_meta_bytes(int m, int ntile);
size_t pa_prefill_packed_part_bytes(const pa_kv_view* kv, int maxend, int ntile, int m);
size_t pa_prefill_packed_part_bound(const pa_kv_view* kv, int max_rows);
int pa_prefill_packed_internal(const pa_kv_view* kv, const float* q, int q_stride, float* out,
                               int out_stride, const int32_t* tiles_dev, int ntile,
                               const int32_t* ctx_dev, int m, int maxend, float sm_scale,
                               void* part_ws, size_t part_bytes, hipStream_t st,
                               const PaRowOutputs* rows = nullptr, int window = 0);
// The same from a host segment list, as the C entry takes it: the list is
// checked, the tile table and the contexts are written on the device into the
// first pa_prefill_packed_meta_bytes of `workspace`, and what follows them is
// the split workspace (part_ws above).
int pa_prefill_packed_segs_internal(const pa_kv_view* kv, const float* q, int q_stride, float* out,
                                    int out_stride, const pa_prefill_seg* segs, int nseg,
                                    float sm_scale, int window, void* workspace,
                                    size_t workspace_bytes, hipStream_t st,
                                    const PaRowOutputs* rows = nullptr);

// Bytes from page p to page p + 1 of a view's pools (page_stride 0 = dense).
inline size_t kv_view_page_stride(const pa_kv_view& v) {
  return v.page_stride > 0 ? (size_t)v.page_stride
                           : (size_t)v.page_size * v.head_dim * kv_elem_size(v.kv_dtype);
}

}  // namespace llm
