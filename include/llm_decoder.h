/*
 * llm_decoder.h — C ABI of the MI355X (gfx950) paged-attention decode path.
 *
 * This is the drop-in boundary: plain pointers, sizes and opaque handles, no
 * torch or HIP types (a hipStream_t is passed as `void*`).  Every entry point
 * returns 0 (LLM_OK) or one of the llm_status codes; llm_last_error() gives a
 * message for the calling thread.  The pybind11 module `llm_decoder`
 * (csrc/bindings.cpp) wraps these exactly as the reference's
 * src/bindings.cpp:3-35 exposes its classes, mapping non-zero status to
 * RuntimeError (the reference's loaders throw std::runtime_error,
 * decoder/decoder_block.hpp:13-19).
 *
 * Citations are file:line in the reference tree.
 */
#ifndef LLM_DECODER_H_
#define LLM_DECODER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum llm_status {
  LLM_OK = 0,
  LLM_ERR_INVALID = 1,      /* bad shape / argument (checked on the host before any launch) */
  LLM_ERR_UNSUPPORTED = 2,  /* valid request this build does not implement (e.g. top-k in attention) */
  LLM_ERR_HIP = 3,          /* HIP runtime error */
  LLM_ERR_OOM = 4,          /* device or page-pool allocation failure */
  LLM_ERR_IO = 5,           /* weight / cache file I/O */
  LLM_ERR_RANGE = 6         /* a device value left a fixed-point accumulator's range (the
                               FP16 decoder's fused o_proj); reported ONCE per clamp, by the
                               first llm_decoder_sync or synchronous step after it */
};

/* Element types.  KV pools may be any of the four of the reference (the T of
 * AttentionCUDA::forward, attention/attention_cuda.cu:58-94: __half, bf16,
 * int8_t (raw values, no scale), float) or LLM_FP8; weights are LLM_I8 or
 * LLM_F16.
 * LLM_FP8 is OCP e4m3fn (bias 7, max +-448, no infinities, NaN = 0x7F / 0xFF:
 * the gfx950 hardware format, not MI300's fnuz), one byte per element:
 *   store: byte = cvt_e4m3_rne(clamp(y * (1 / scale), -448, +448)), NaN -> NaN
 *   load:  value = decode(byte) * scale
 * pa_decode / pa_decode_grouped / pa_decode_ex read LLM_FP8 pools as plain
 * numbers (scale 1), as they read LLM_I8: a caller with scales folds K's into
 * sm_scale and multiplies `out` by V's.  The decoder keeps one k_scale and one
 * v_scale per layer (llm_decoder_set_kv_scales). */
enum llm_dtype { LLM_F16 = 0, LLM_I8 = 1, LLM_F32 = 2, LLM_BF16 = 3, LLM_FP8 = 4 };
enum llm_act { LLM_ACT_NONE = 0, LLM_ACT_RELU = 1, LLM_ACT_GELU = 2 };

const char* llm_last_error(void);
int llm_abi_version(void);

/* Host-only codec of LLM_FP8 with the semantics above (plain C++, no device
 * call): out[i] = encode(x[i] / scale) and out[i] = decode(in[i]) * scale.
 * scale must be finite and > 0; values beyond +-448 * scale saturate to
 * 0x7E / 0xFE; a NaN encodes to 0x7F (0xFF with the sign bit set). */
int llm_fp8_e4m3_encode(const float* x, size_t n, float scale, uint8_t* out);
int llm_fp8_e4m3_decode(const uint8_t* in, size_t n, float scale, float* out);

/* ------------------------------------------------------------------------ */
/* Paged decode attention                                                    */
/* ------------------------------------------------------------------------ */

/* POD device view of one layer's KV pools + page table, passed BY VALUE to the
 * kernel.  Replaces handing the host KVTileCache object (std containers,
 * mutex) to device code (attention/attention_tile_launcher.hpp:43,
 * attention/paged_flash_attention_kernel_fused.cu:13).  Semantics of
 * KVTileCache<T>::get (kv_cache/kv_tile_cache.hpp:21-26) and
 * PageTable::lookup (kv_cache/page_table.hpp:39-49): entry
 * page_table[(beam*num_heads + head)*max_tiles + tile]; a page < 0 or
 * >= num_pages means "no tile" (its tokens are masked). */
typedef struct pa_kv_view {
  const void* k_pool;         /* [num_pages][page_size][head_dim] of kv_dtype */
  const void* v_pool;         /* same layout */
  const int32_t* page_table;  /* [num_beams][num_heads][max_tiles] int32, device */
  int32_t num_pages;
  int32_t page_size;          /* tokens per page (tile_size) */
  int32_t head_dim;
  int32_t num_beams;
  int32_t num_heads;
  int32_t max_tiles;
  int32_t kv_dtype;           /* LLM_F16 (default), LLM_BF16, LLM_F32, LLM_I8 or LLM_FP8; one page
                               * (page_size * head_dim elements) must be 1..16 KiB */
  int64_t page_stride;        /* bytes from page p to page p + 1 within each pool; 0 = one
                               * page (dense pools).  kv_cache's own pools interleave K and
                               * V pages ([num_pages][K page | V page], stride 2 pages,
                               * v_pool = k_pool + 1 page) */
} pa_kv_view;

/* Bytes of device workspace pa_decode needs (split-T partial softmax state). */
size_t pa_decode_workspace_bytes(int B, int H, int D, int max_tiles, int pages_per_split);

/* Host-only ESTIMATE of the split-T size pa_decode picks when
 * pages_per_split <= 0, for a uniform context T: it assumes 3,072 resident
 * waves (256 CUs x 12) where pa_decode queries the device's occupancy for the
 * kernel it launches and derives each row's split length from that row's own
 * context, so the two can differ.  For labelling runs, not for sizing them. */
int pa_decode_pages_per_split(int B, int H, int T, int page_size, int max_tiles);

/* The launch a pa_decode / pa_decode_grouped call with these arguments
 * takes, without launching it: *nsplit = splits per (row, head) and *form =
 * LLM_PA_FORM_* (direct: one split, no merge; split + merge launch;
 * LLM_PA_FORM_BEAM is or-ed in for the beam-group kernel).  For tests and
 * run labels; the decoder's own step reports its launch with
 * llm_decoder_attention_plan. */
#define LLM_PA_FORM_DIRECT 0
#define LLM_PA_FORM_SPLIT_MERGE 1     /* split launch + pa_merge_kernel (fp32 rows) */
#define LLM_PA_FORM_SPLIT_MERGE_ROW 2 /* split launch + pa_merge_row_kernel (o_proj input) */
#define LLM_PA_FORM_WG_MERGE 3        /* splits merged inside the split workgroup */
#define LLM_PA_FORM_BEAM 16
#define LLM_PA_FORM_OPROJ 32 /* FP16 decoder: o_proj fused into the workgroup merge */
#define LLM_PA_FORM_STEAL 64 /* tuning library only (LLM_BEAM_STEAL=1): beam groups with
                                tiles assigned to the splits while the launch runs (with
                                LLM_PA_FORM_BEAM); the product never reports it */
int pa_decode_plan(const pa_kv_view* kv, int B, int H, int D, int T, int pages_per_split,
                   int row_group, int* nsplit, int* form);

/* Paged decode attention (replaces paged_flash_attention_kernel_fused,
 * attention/paged_flash_attention_kernel_fused.cu:5-90, launched by
 * AttentionTileLauncher::launch, attention/attention_tile_launcher.hpp:36-89,
 * from AttentionCUDA::forward, attention/attention_cuda.cu:41-95), with the
 * INTENDED maths of cpu_paged_attention_forward
 * (attention_cpu/cpu_attention_kernel.cpp:37-129):
 *   r = beam_ids ? beam_ids[b] : b;  T_b = context_lens ? context_lens[b] : T
 *   s_t = (q[b,h] . k_t) * sm_scale        (sm_scale = 1/temperature^2 reproduces
 *                                           the reference's double division)
 *   out[b,h] = sum_t exp(s_t - max s) v_t / (sum_t exp(s_t - max s) + 1e-6)
 * over t < T_b whose page is present.  q, out: fp32 [B][H][D] device.
 * pages_per_split <= 0: the split count is chosen on the device side of the
 * call from the launch's occupancy (a whole number of resident-wave rounds)
 * and each row's split length from its own context; pa_decode_pages_per_split
 * only estimates it, and pa_decode_plan reports the choice exactly.
 * workspace may be NULL when the call needs none (single split). */
int pa_decode(const pa_kv_view* kv, const float* q, float* out, const int32_t* beam_ids,
              const int32_t* context_lens, int B, int H, int D, int T, float sm_scale,
              int pages_per_split, void* workspace, size_t workspace_bytes, void* stream);

/* pa_decode with beam-aware scheduling (the beam routing of
 * paged_flash_attention_kernel_fused.cu:22 plus "beam-aware KV tile prefetch",
 * README.md:64): rows are taken in groups of row_group (1..4, e.g. the beams of
 * one sequence, rows g*row_group .. g*row_group+row_group-1); the group's rows
 * for one (head, split) run as adjacent waves of one workgroup, so KV pages
 * they share through kv_cache_fork are read from HBM once (row_group 4: staged
 * through LDS, with split boundaries placed by cost so the splits holding the
 * beam-private tail are not the slowest).  Results equal pa_decode bit for
 * bit, except for groups of 4 equal-context rows under dynamic splits
 * (pages_per_split 0), whose cost-balanced partition changes only the fp32
 * rounding of the split merge.  The workspace is sized by
 * pa_decode_workspace_bytes as for pa_decode. */
int pa_decode_grouped(const pa_kv_view* kv, const float* q, float* out, const int32_t* beam_ids,
                      const int32_t* context_lens, int B, int H, int D, int T, float sm_scale,
                      int pages_per_split, int row_group, void* workspace,
                      size_t workspace_bytes, void* stream);

/* pa_decode over a sliding window: row b attends to its last `window` tokens,
 *   max(0, T_b - window) <= t < T_b
 * (T_b counts the row's own token), whose page is present; the maths is
 * pa_decode's over those keys.  window 0 is off and window < 0 is
 * LLM_ERR_INVALID.  Rows are ungrouped (pa_decode_grouped and pa_decode_ex
 * take no window).  The tiles below a row's window are never read: their
 * table entries may be -1 (kv_cache_release_before) and their pages may hold
 * anything.  The splits are cut over the window, not the context: split s of
 * a row starts s split lengths after the tile that holds T_b - window, and the
 * plan sizes the splits for ceil(window / page_size) + 1 tiles, the most a
 * window touches.  With window >= T the launch, its plan and its output bits
 * are pa_decode's.  Workspace as pa_decode (pa_decode_workspace_bytes). */
int pa_decode_window(const pa_kv_view* kv, const float* q, float* out, const int32_t* beam_ids,
                     const int32_t* context_lens, int B, int H, int D, int T, float sm_scale,
                     int pages_per_split, int window, void* workspace, size_t workspace_bytes,
                     void* stream);
/* pa_decode_plan for a pa_decode_window call (row_group 1). */
int pa_decode_window_plan(const pa_kv_view* kv, int B, int H, int D, int T, int pages_per_split,
                          int window, int* nsplit, int* form);

/* Causal paged attention of a prompt chunk: the reference's prefill pass
 * (AttentionCUDA's is_prefill flag, attention/attention_cuda.hpp:21; maths of
 * cpu_paged_attention_forward, attention_cpu/cpu_attention_kernel.cpp:37-129,
 * per query).  m query tokens of ONE sequence at positions p0 .. p0+m-1, whose
 * K/V are already in the pages of page-table row `row`; query i attends to
 * positions 0 .. p0+i.  Equals pa_decode with B = m, beam_ids[i] = row,
 * context_lens[i] = p0 + i + 1 (within 1e-3 relative), but each K/V page is
 * read once per 32 queries instead of once per query (MFMA tiles).
 * q, out: fp32 [m][H][D] with row strides q_stride / out_stride floats
 * (<= 0: H*D), 16-byte aligned.  fp16 or LLM_FP8 pools, head_dim 64 or 128,
 * page_size 16 or 32 (else LLM_ERR_UNSUPPORTED; pa_decode covers every shape).
 * LLM_FP8 pools are read as plain numbers (scale 1, as pa_decode: fold a K
 * scale into sm_scale); their bytes are decoded to fp16 exactly, so the result
 * is bit-equal to the same call on fp16 pools holding the decoded values.
 * With workspace_bytes >= pa_prefill_workspace_bytes(kv, p0, m) (and
 * out_stride H*D) the key range is split over more workgroups and merged as
 * pa_decode's splits; with less (or NULL) it runs in one pass. */
size_t pa_prefill_workspace_bytes(const pa_kv_view* kv, int p0, int m);
int pa_prefill(const pa_kv_view* kv, const float* q, int q_stride, float* out, int out_stride,
               int row, int p0, int m, float sm_scale, void* workspace, size_t workspace_bytes,
               void* stream);
/* pa_prefill over a sliding window: query i attends to positions
 * max(0, p0 + i - window + 1) .. p0 + i.  Equals pa_decode_window with B = m,
 * beam_ids[i] = row, context_lens[i] = p0 + i + 1 (within 1e-3 relative).
 * window 0 is off (pa_prefill itself), window < 0 LLM_ERR_INVALID.  The key
 * blocks below the chunk's first visible position are not read.  The
 * workspace size is pa_prefill_workspace_bytes' (an upper bound: the key
 * split is planned over the whole range, and the splits wholly below the
 * window cost no reads). */
int pa_prefill_window(const pa_kv_view* kv, const float* q, int q_stride, float* out,
                      int out_stride, int row, int p0, int m, float sm_scale, int window,
                      void* workspace, size_t workspace_bytes, void* stream);

/* pa_prefill over prompt chunks of SEVERAL sequences in one launch.  The m =
 * sum(len) query rows are dense in q / out (strides and alignment as
 * pa_prefill) and made of nseg segments in the order given: segment j is len
 * consecutive rows at positions p0 .. p0+len-1 of page-table row `row`, whose
 * K/V are already in that row's pages.  A page-table row appears in at most
 * one segment.  Row i of segment j equals pa_prefill(row, p0, len) row i; in
 * the one-pass form bit for bit (a query's result does not depend on the
 * other queries of its tile).
 * The launch is driven by a tile table, one entry {q0, nq, row, p0} per
 * workgroup column: nq <= 64 rows from packed row q0, at positions p0 .. of
 * page-table row `row`; a segment of length len gets ceil(len / 64) tiles and
 * no tile straddles two segments.  pa_prefill_packed_tiles (host only) fills
 * tiles[cap][4] and returns the tile count -- also when cap is too small or
 * tiles is NULL, then writing nothing -- or < 0 for an invalid segment list.
 * workspace is always required: it holds the tile table and the rows' context
 * lengths, and at the split = 1 size also the split partials.  With at least
 * pa_prefill_packed_workspace_bytes(.., 1) (and out_stride H*D) the key range
 * is split -- one split length for the launch, planned as pa_prefill's from
 * the longest segment end and the tile count; a tile skips the splits past
 * its last query -- and merged as pa_decode's splits; with at least the
 * split = 0 size it runs in one pass; with less, LLM_ERR_INVALID.
 * LLM_ERR_INVALID (on the host, before any launch) also for nseg < 1, a
 * segment with len < 1 or p0 < 0, a row outside the table or repeated,
 * positions past max_tiles, and strides or alignment pa_prefill refuses;
 * LLM_ERR_UNSUPPORTED for pools pa_prefill does not take.
 * `segs` may be freed when the call returns: the table and the context
 * lengths are written in stream order by small launches that carry the
 * segment descriptors as kernel arguments, which the launch call copies (no
 * host-to-device copy from the caller's memory is left in flight).  The call
 * must not be captured into a graph: the nodes would carry this call's segment
 * list, and the entry makes no promise about its launch count. */
typedef struct pa_prefill_seg { int32_t row, p0, len; } pa_prefill_seg;
int pa_prefill_packed_tiles(const pa_kv_view* kv, const pa_prefill_seg* segs, int nseg,
                            int32_t* tiles, int cap);
size_t pa_prefill_packed_workspace_bytes(const pa_kv_view* kv, const pa_prefill_seg* segs,
                                         int nseg, int split);
int pa_prefill_packed(const pa_kv_view* kv, const float* q, int q_stride, float* out,
                      int out_stride, const pa_prefill_seg* segs, int nseg, float sm_scale,
                      void* workspace, size_t workspace_bytes, void* stream);
/* pa_prefill_packed over a sliding window: row i of segment j equals
 * pa_prefill_window(row, p0, len) row i, in the one-pass form bit for bit.
 * Workspace sizes as pa_prefill_packed. */
int pa_prefill_packed_window(const pa_kv_view* kv, const float* q, int q_stride, float* out,
                             int out_stride, const pa_prefill_seg* segs, int nseg,
                             float sm_scale, int window, void* workspace,
                             size_t workspace_bytes, void* stream);

/* The optional stages of the reference attention, CPUAttentionInput /
 * CPUAttentionOutput (attention_cpu/attention_cpu.hpp:8-43) as used by
 * cpu_paged_attention_forward (attention_cpu/cpu_attention_kernel.cpp:37-129):
 *   scores_t = q.k_t / temperature (-1e9 where the tile is missing)
 *   p = exp((scores - max) / temperature) / (sum + 1e-6)  (softmax_lut.cpp:203-231)
 *   apply_topk_topp_filter (softmax_lut.cpp:233-256): rank by (p, index)
 *     descending, zero rank >= top_k (top_k > 0) and every entry whose
 *     higher-ranked mass is >= top_p (top_p < 1); no renormalisation; then if
 *     eos_token >= 0 and p[eos_token] > eos_threshold, zero all other entries
 *   out = sum_t p_t v_t
 * The GPU kernel of the reference exposes the same knobs (top_k, top_p,
 * rerank_scores: paged_flash_attention_kernel_fused.cu:5-90). */
typedef struct pa_decode_options {
  float temperature;   /* > 0; 1 = reference default (attention_config.hpp:20) */
  int top_k;           /* 0 = off */
  float top_p;         /* 1 = off */
  int eos_token;       /* -1 = off (a KV position) */
  float eos_threshold;
  float* probs_out;    /* [B][H][T] attention weights after filtering, 0 past T_b (nullable) */
  float* scores_out;   /* [B][H][T] scores, -1e9 past T_b / for missing tiles (nullable) */
} pa_decode_options;

/* pa_decode with the options above.  With every option off (top_k 0, top_p 1,
 * eos -1, no outputs) this is pa_decode with sm_scale = 1/temperature^2 (the
 * hot path; workspace as for pa_decode).  Otherwise one workgroup per (b, h)
 * keeps the row's scores in LDS when T <= 8192 (workspace unused), and in the
 * workspace for longer rows: T > 8192 needs an 8-byte aligned workspace of
 * pa_decode_ex_workspace_bytes(B, H, T) bytes (else LLM_ERR_INVALID); like
 * cpu_paged_attention_forward (attention_cpu/cpu_attention_kernel.cpp:61) the
 * context has no practical upper bound: D <= 256 and T <= 2^30 (else
 * LLM_ERR_UNSUPPORTED; the workspace size is then 0). */
size_t pa_decode_ex_workspace_bytes(int B, int H, int T);
int pa_decode_ex(const pa_kv_view* kv, const float* q, float* out, const int32_t* beam_ids,
                 const int32_t* context_lens, int B, int H, int D, int T,
                 const pa_decode_options* opt, void* workspace, size_t workspace_bytes,
                 void* stream);

/* ------------------------------------------------------------------------ */
/* INT8 / FP16 weight GEMMs (MFMA)                                          */
/* ------------------------------------------------------------------------ */

/* Bytes of the packed (MFMA-fragment-ordered) weight for a [K][N] matrix. */
size_t gemm_packed_bytes(int dtype, int K, int N);

/* Repack W [K][N] row-major (the reference layout, decoder/mlp.hpp:28-31) into
 * the MFMA fragment order the GEMM streams (device -> device). */
int gemm_pack_weights(int dtype, const void* W_kn, void* W_packed, int K, int N, void* stream);

/* INT8 GEMM, contract of dnnl_matmul_int8 (attention_cpu/dnnl_matmul_int8.cpp:7-75)
 * restated for decode:
 *   acc[m,n] = sum_k int32(A[m,k]) * int32(W[k,n])          exact int32
 *   C[m,n]   = act(float(acc) * (sa[m] * sw[n]) + bias[n])  fp32
 * A int8 [M][K] (row stride lda >= K), W_packed from gemm_pack_weights.
 * sa / sw / bias may be NULL (1, 1, 0).  acc_out (int32 [M][N]) and C
 * (fp32 [M][N]) may each be NULL.  K % 64 == 0, N % 16 == 0. */
int i8_gemm(const int8_t* A, int lda, const void* W_packed, int32_t* acc_out, float* C,
            int M, int N, int K, const float* sa, const float* sw, const float* bias,
            int act, void* stream);

/* Batched INT8 matmul with int8 output, the full form of dnnl_matmul_int8
 * (attention_cpu/dnnl_matmul_int8.cpp:7-75, dnnl_matmul_int8.hpp:5-13):
 *   A s8 [batch][M][K], B s8 [batch][K][N] (row-major, unpacked), C s8 [batch][M][N]
 *   y = act((float(acc) + bias[n]) * alpha),  alpha = scale_a * scale_b / scale_c
 *   C = round_half_even(saturate(y, -128, 127))
 * bias (fp32 [N]) may be NULL; act LLM_ACT_NONE / RELU / GELU (erf).  Any M, N,
 * K (K < 131072); batch * M * N == 0 is a no-op.  The reference returns false
 * on any failure; this returns a status code (llm_last_error()). */
int i8_matmul_s8(const int8_t* A, const int8_t* B, int8_t* C, int batch, int M, int N, int K,
                 float scale_a, float scale_b, float scale_c, const float* bias, int act,
                 void* stream);

/* FP16 GEMM with fp32 accumulate (CUDADecoder weights):
 *   C[m,n] = act(sum_k A[m,k] W[k,n] + bias[n]),  A fp16 [M][K], K % 32 == 0. */
int f16_gemm(const void* A, int lda, const void* W_packed, float* C, int M, int N, int K,
             const float* bias, int act, void* stream);

/* Tied-embedding LM head: logits[m,v] = sum_k x[m,k] * E[v,k], x fp32 [M][K],
 * E fp16 [V][K] (token_embedding.hpp layout).  x is split hi+lo into two fp16
 * MFMA operands so the product keeps ~fp32 accuracy.  K % 32 == 0. */
int lm_head(const float* x, const void* E, float* logits, int M, int V, int K, void* stream);

/* Row-wise argmax (first maximum wins, std::max_element, decoder/cuda_decoder.cu:7-14). */
int argmax_rows(const float* logits, int rows, int V, int32_t* out, void* stream);

/* Device token sampling per row, reference semantics of
 * top_k_top_p_filter (attention/top_k_top_p_filter.cuh:55-111) and
 * apply_topk_topp_filter (attention_cpu/softmax_lut.cpp:233-256):
 *   p = softmax(logits / temperature) (max-subtracted, sum + 1e-6);
 *   token i is dropped if its probability rank >= top_k (top_k > 0) or if the
 *   probability mass ranked above it is >= top_p (top_p < 1);
 *   the kept mass is sampled by inverse CDF in token-index order with
 *   u = sample_uniform_host(seed, row, counter) in [0, 1).
 * temperature <= 0 or top_k == 1: greedy argmax (cuda_decoder.cu:7-14).
 * V <= 65536. */
int sample_rows(const float* logits, int rows, int V, float temperature, int top_k, float top_p,
                uint64_t seed, int counter, int32_t* out, void* stream);
/* sample_rows with every row's own settings, for rows of different requests in
 * one launch (the token choice of llm_decoder_serve_step): temperature /
 * top_p fp32 [rows], top_k / counter int32 [rows], seed uint64 [rows], all
 * DEVICE arrays read by the one launch (the same kernel as sample_rows: a
 * workgroup handles one row, so the choice between the greedy and the
 * sampling path is uniform within it).  Row r is greedy if temperature[r] <= 0
 * or top_k[r] == 1 (first maximum wins); else it draws with
 *   u = sample_uniform_host(seed[r], 0, counter[r]):
 * the row term of the hash is 0, so a row's token depends on its logits, its
 * settings, its seed and its counter, not on where it sits in the launch.
 * Any array may be NULL: temperature 1, top_k 0 (off), top_p 1 (off),
 * counter 0, and a NULL seed is sample_rows' draw, u = sample_uniform_host(0,
 * r, counter) -- all NULL is sample_rows(logits, rows, V, 1, 0, 1, 0, 0, ..).
 * The shape checks are sample_rows' (V <= 65536); the settings are device
 * data and are not checked: top_k < 0 counts as 0, top_p >= 1 as off. */
int sample_rows_each(const float* logits, int rows, int V, const float* temperature,
                     const int32_t* top_k, const float* top_p, const uint64_t* seed,
                     const int32_t* counter, int32_t* out, void* stream);
/* Beam candidates of one decode step (csrc/beam_select.hip).  logits fp32
 * [rows][V] device with rows = num_seqs * W, row = seq * W + beam, 1 <= W <= 4;
 * score_in fp32 [rows] device, a beam's cumulative log-probability, -inf for
 * a beam that is not live (its row is not read and competes with -inf).
 * Row stage, one workgroup per row: m = max x, s = sum exp(x - m), and the
 * row's 2W largest RAW logits (ties: lower token id first), so with W = 1 the
 * winner is argmax_rows' id whatever the rounding of a log-probability.
 * Merge stage, one wave per sequence: the W * 2W candidates get
 *   score = score_in[row] + ((x - m) - log(s + 1e-6))    (sample_rows' sum + 1e-6)
 * and are ranked by (score descending, parent ascending, token ascending);
 * the best 2W, in that order, go to cand_score / cand_parent (the beam, 0 ..
 * W-1) / cand_token, each [num_seqs][2W] device.  Two launches, no atomics,
 * the same result on every run.  2W <= V <= 65536 (else LLM_ERR_INVALID, as W
 * outside 1..4: all checked on the host before any launch).  The row stage's
 * results pass through a scratch buffer the library keeps and grows on demand
 * (the only part of a call that cannot be captured into a graph: call once
 * at the largest num_seqs first); calls on different streams must not overlap. */
int beam_select_rows(const float* logits, const float* score_in, int num_seqs, int W, int V,
                     float* cand_score, int32_t* cand_parent, int32_t* cand_token, void* stream);
/* Log-probabilities.  For a logits row x of V entries, m = max x and
 * s = sum_v exp(x_v - m) in fp32:
 *   lse = log(s + 1e-6),   logprob(t) = (x_t - m) - lse
 * -- beam_select_rows' term, so a hypothesis's sum_logprob and the score of
 * the same ids mean the same thing.  Always of the raw logits: temperature 1,
 * before top-k / top-p.
 *
 * lm_head_logprobs: the LM head with a log-softmax epilogue (csrc/lm_head.hip).
 * x, E, M, V, K as lm_head (E is packed once per call); targets int32 [M]
 * device.  logprob[r] = logprob(targets[r]) of row r's logits; a target outside
 * [0, V) is an ignore index: logprob[r] = 0 and a target logit of 0.  stats
 * (may be NULL) fp32 [M][3] = {m, lse, x_target}.  No [M][V] logits are written
 * anywhere: the MFMA sequence is lm_head's (the same logits in registers, bit
 * for bit), reduced per (row, workgroup) to {max, sum exp(x - max), target
 * logit}, and a merge launch combines the partials per row in a fixed order.
 * Two launches, no atomics, the same bits on every run.  LLM_ERR_INVALID, on
 * the host before any launch, for a NULL operand (stats excepted),
 * K % 32 != 0, or a packed E past 32-bit offsets; M == 0 is a no-op. */
int lm_head_logprobs(const float* x, const void* E, const int32_t* targets, float* logprob,
                     float* stats, int M, int V, int K, void* stream);
/* logprob_rows: chosen and top-n log-probabilities of materialised rows
 * (csrc/logprobs.hip; one workgroup per row, one launch).  logits fp32
 * [rows][V] device.  chosen (int32 [rows] device, may be NULL): chosen_lp[r] =
 * logprob(chosen[r]); an id outside [0, V) is an ignore index and writes 0.
 * top_n in 0 .. LLM_MAX_TOP_LOGPROBS: top_id[r][j] / top_lp[r][j], j < top_n
 * (stride top_n), are the row's top_n largest RAW logits ordered by (logit
 * descending, token id ascending) with their log-probabilities.  stats (may be
 * NULL) fp32 [rows][2] = {m, lse}.  LLM_ERR_INVALID on the host for top_n
 * outside 0..8, V < max(1, top_n), V > 65536, or a NULL output that the
 * arguments require (chosen_lp with chosen; top_lp / top_id with top_n > 0). */
#define LLM_MAX_TOP_LOGPROBS 8
int logprob_rows(const float* logits, int rows, int V, const int32_t* chosen, int top_n,
                 float* chosen_lp, float* top_lp, int32_t* top_id, float* stats, void* stream);
/* The uniform draw sample_rows uses for (seed, row, counter): splitmix64 of
 * seed ^ (row << 32) ^ counter, top 24 bits / 2^24. */
float sample_uniform_host(uint64_t seed, int row, int counter);

/* The standard rotary table (layout of attention/attention_kernel_utils.cuh:20-35,
 * table[t * head_dim + d] = cos, [.. + d + 1] = sin for even d): for pair
 * i = d / 2, angle = t * theta^(-2 i / head_dim), computed in double and
 * rounded to fp32.  Host only.  theta > 0, head_dim even and > 0,
 * num_pos >= 1, table float [num_pos][head_dim]. */
int llm_rope_table(double theta, int head_dim, int num_pos, float* table);

/* Rotary embedding in place (the per-position interleaved rotation of
 * attention/attention_kernel_utils.cuh:20-35) of x fp32 [rows][H][D], row r at
 * x + r * x_stride (x_stride >= H * D floats), by position pos[r]: with
 * c = table[pos[r] * D + d], s = table[pos[r] * D + d + 1] for even d,
 *   x'[d] = x[d] c - x[d+1] s,   x'[d+1] = x[d] s + x[d+1] c,
 * every product rounded to fp32 on its own, then one add (no fma).  A row
 * whose position is outside [0, num_pos) is left as it is and the table is not
 * read for it.  For callers of pa_decode / pa_prefill who project q and K
 * themselves; the decoder's qkv projection applies the same rotation in its
 * epilogue (llm_decoder_set_rope).  D even; table device float [num_pos][D]. */
int rope_rows(float* x, int x_stride, const int32_t* pos, int rows, int H, int D,
              const float* table, int num_pos, void* stream);

/* Per-row dynamic int8 quantisation (attention_cpu/int8_quant.cpp:5-13,59-64):
 * scale_r = 127/(absmax_r + 1e-6); q = clamp(round(x*scale_r)); inv_scale[r] = 1/scale_r. */
int quantize_rows(const float* x, int rows, int cols, int8_t* q, float* inv_scale, void* stream);

/* LayerNorm (decoder/layer_norm.hpp:20-37) fused with per-row int8 quantisation
 * (q/inv_scale may be NULL: then only `out` fp32 is written; out may be NULL). */
int layernorm_quant(const float* x, int rows, int cols, const float* gamma, const float* beta,
                    float eps, float* out, int8_t* q, float* inv_scale, void* stream);

/* ------------------------------------------------------------------------ */
/* KV cache: page pools + page table (kv_cache/page_table.hpp:5-37,          */
/* kv_cache/kv_tile_cache.hpp:9-80) with a layer dimension, a free-list page */
/* allocator (replacing the map.size() ids of kv_tile_cache.cpp:71) and a    */
/* single host source of truth synchronised to the device.                   */
/* ------------------------------------------------------------------------ */
typedef struct kv_cache kv_cache;

int kv_cache_create(int num_layers, int num_beams, int num_heads, int head_dim, int page_size,
                    int max_tiles, long long num_pages, kv_cache** out);
/* kv_cache_create with pools of kv_dtype elements (KVTileCache<T>,
 * kv_cache/kv_tile_cache.hpp:9 with T in {__half, bf16, int8_t, float}, or
 * LLM_FP8: one byte per element; kv_cache_write_tokens takes the raw bytes, and
 * no file written from the cache holds scales -- the caller keeps them, as the
 * reference's pool dumps keep no page table). */
int kv_cache_create_typed(int num_layers, int num_beams, int num_heads, int head_dim,
                          int page_size, int max_tiles, long long num_pages, int kv_dtype,
                          kv_cache** out);
void kv_cache_destroy(kv_cache* c);
int kv_cache_view(const kv_cache* c, int layer, pa_kv_view* out);
long long kv_cache_num_pages(const kv_cache* c);
long long kv_cache_free_pages(const kv_cache* c);
/* Pages copied on write since kv_cache_create (a running count, for measurements). */
long long kv_cache_cow_copies(const kv_cache* c);
/* PageTable::assign (page_table.cpp:49-53) / lookup / remove (:64-66), host mirror. */
int kv_cache_assign(kv_cache* c, int layer, int beam, int head, int tile, int page);
int kv_cache_lookup(const kv_cache* c, int layer, int beam, int head, int tile);
int kv_cache_remove(kv_cache* c, int layer, int beam, int head, int tile);
/* KVTileCache::register_tile (kv_tile_cache.cpp:64-77): allocate a free page
 * for (layer, beam, head, tile) if it has none; returns the page id in *page. */
int kv_cache_register_tile(kv_cache* c, int layer, int beam, int head, int tile, int* page);
/* Page-pool exhaustion policy of kv_cache_register_tile.  LLM_EVICT_NONE (the
 * default): LLM_ERR_OOM.  LLM_EVICT_LRU: KVTileCache's policy
 * (kv_cache/kv_tile_cache.cpp:64-98, update_lru / evict_if_needed): every
 * register_tile call makes its tile the most recently used, and a tile that
 * needs a page when none is free takes one by removing the least recently
 * registered tile whose page that frees (an entry on a page a forked beam
 * still shares is kept) -- the reference's semantics, so an evicted tile of a
 * live sequence reads as missing (masked) afterwards.  Only entries whose
 * page kv_cache_register_tile mapped are candidates: any other call that
 * writes an entry (reserve / the decoder's append, assign -- even with its
 * current page --, remove, release, fork, copy-on-write, a snapshot load)
 * takes it off the recency list, so the decoder's own pages never are.
 * Switching the policy keeps the recency list. */
#define LLM_EVICT_NONE 0
#define LLM_EVICT_LRU 1
int kv_cache_set_eviction(kv_cache* c, int policy);
/* Ensure pages exist for tiles covering tokens [0, n_tokens) of `beam`, all layers/heads. */
int kv_cache_reserve(kv_cache* c, int beam, int n_tokens);
/* Beam fork: dst's page-table rows := src's (all layers, heads), shared pages
 * refcounted; pages of dst are copied-on-write by kv_cache_append/write. */
int kv_cache_fork(kv_cache* c, int src_beam, int dst_beam);
/* Beam re-parenting after a beam-search step: row first_beam + i := what row
 * first_beam + parent[i] held BEFORE the call (parent[i] in [0, n), host array),
 * for the tiles covering tokens [0, n_tokens), all layers and heads.  Shared
 * pages are refcounted as by kv_cache_fork (the next append copies on write);
 * the pages of a row no child names are released.  A row that names itself
 * gets no table writes; every entry is read before any entry of its tile is
 * written, so a permutation (e.g. a swap) is safe.  Only tiles below
 * ceil(n_tokens / page_size) are walked and equal entries are skipped, where
 * kv_cache_fork walks all max_tiles: cheap enough to run once per step.
 * Tiles past n_tokens are left as they are. */
int kv_cache_reorder(kv_cache* c, int first_beam, int n, const int32_t* parent, int n_tokens);
/* Release every page of `beam` (refcount-aware). */
int kv_cache_release(kv_cache* c, int beam);
/* Blocks that outlive a row (what a prefix cache is made of).  A block is
 * tile `tile` of a beam across all layers and heads: num_layers * num_heads
 * pages, listed layer-major, head-minor (pages[layer * num_heads + head]).
 *   hold    every (layer, head) entry of the tile must be mapped, else
 *           LLM_ERR_INVALID with nothing changed.  Writes the page ids and
 *           takes one more reference on each page: they stay allocated, with
 *           their contents, after kv_cache_release(beam).
 *   attach  every (layer, head) entry of the tile must be -1 and every page
 *           allocated, else LLM_ERR_INVALID with nothing changed.  The entries
 *           become those pages, plus one reference each, as any other table
 *           write (pushed by the next kv_cache_sync; a release mark above the
 *           tile falls to it; the entries are no LRU candidates).  A later
 *           append into the tile copies on write, as after kv_cache_fork.
 *   drop    one reference less on each page; a page whose count reaches 0
 *           returns to its zone's free list.  LLM_ERR_INVALID with nothing
 *           changed if a page is not allocated.
 * kv_cache_clear (and a snapshot load) resets every count: a holder must
 * forget its page lists then, and never drop them afterwards. */
int kv_cache_hold_tile(kv_cache* c, int beam, int tile, int32_t* pages);
int kv_cache_attach_tile(kv_cache* c, int beam, int tile, const int32_t* pages);
int kv_cache_drop_pages(kv_cache* c, const int32_t* pages);
/* Release the pages of `beam` that lie wholly below token n_tokens: tiles
 * < n_tokens / page_size, all layers and heads (refcount-aware: a page a
 * forked beam still shares stays allocated until its last owner lets go).
 * The entries become -1 (dirty: the next kv_cache_sync pushes them; no
 * longer LRU candidates), which attention reads as missing.  What a
 * sliding-window decoder calls as its rows advance.  Idempotent, and cheap
 * when repeated: a per-beam mark of the tiles already released is kept, so a
 * call walks the newly dead tiles only (any later write of a page below the
 * mark -- reserve, assign, fork into the beam, a snapshot load -- lowers it
 * again).  n_tokens <= 0 is a no-op; a beam out of range LLM_ERR_INVALID. */
int kv_cache_release_before(kv_cache* c, int beam, int n_tokens);
/* PageTable::clear (page_table.cpp:39-44): all entries -1, all pages free. */
int kv_cache_clear(kv_cache* c);
/* PageTable::sync_to_gpu (page_table.cpp:59-62): push dirty host entries.
 * Pending copy-on-write page copies go first: two or more of them in ONE
 * launch (one workgroup per page pair, the pairs staged through pinned
 * memory), a single one as a device memcpy. */
int kv_cache_sync(kv_cache* c, void* stream);
/* Copy n tokens of K and V (host, [n][H][D] in the cache's kv_dtype) for
 * `beam` starting at token position pos into the pools of `layer`. */
int kv_cache_write_tokens(kv_cache* c, int layer, int beam, int pos, int n, const void* k_host,
                          const void* v_host);
/* Device pointers of the pools / table (for tests and custom kernels).  Page
 * p of the K (V) pool starts at kv_cache_k_pool (v_pool) + p * page_stride. */
void* kv_cache_k_pool(kv_cache* c);
void* kv_cache_v_pool(kv_cache* c);
long long kv_cache_page_stride(const kv_cache* c);
int32_t* kv_cache_page_table(kv_cache* c, int layer);
/* Snapshot of the whole cache ("APPIMKV2": geometry, layered page table, used
 * pages K then V) — this build's own format, the one that restores the page
 * table too.  kv_cache_load validates the whole file (geometry, every table
 * entry and page id in [-1, num_pages), exact size) before it changes the
 * cache; on a failure after that point the cache is left cleared. */
int kv_cache_save(const kv_cache* c, const char* path);
int kv_cache_load(kv_cache* c, const char* path);
/* Validate a snapshot on the host (no device needed): geometry[9] receives
 * {L, beams, H, D, page_size, max_tiles, num_pages, kv_dtype, used_pages}. */
int kv_cache_inspect(const char* path, long long* geometry);
/* KVTileCache<T>::save_to_file / load_from_file (kv_cache/kv_tile_cache.cpp:
 * 105-125), byte for byte: the raw K pool [num_pages][page_size][head_dim]
 * then the raw V pool, no header, no page table (the reader keeps its own).
 * load_pools refuses a file whose size is not 2 * num_pages * page bytes. */
int kv_cache_save_pools(const kv_cache* c, const char* path);
int kv_cache_load_pools(kv_cache* c, const char* path);
/* KVTileCacheCPU<T>::save / load (kv_cache/kv_tile_cache_cpu.cpp:89-123), byte
 * for byte: int32 count, then per tile {int32 batch_id, head_id, tile_id} and
 * page_size * head_dim elements.  One file holds the K (kind 0) or V (kind 1)
 * tiles of one layer (the reference keeps K and V in two caches); batch_id is
 * the beam.  save writes every mapped tile in (beam, head, tile) order (the
 * reference's order is its hash map's).  load maps each record's tile (a new
 * page, or copy-on-write of a shared one) and writes its data; a later record
 * of the same tile wins, as in the reference; records outside this cache's
 * (beam, head, tile) range are refused before anything changes. */
int kv_cache_save_tiles(const kv_cache* c, int layer, int kind, const char* path);
int kv_cache_load_tiles(kv_cache* c, int layer, int kind, const char* path);
/* Validate a tile-record file of tile_bytes-byte tiles on the host (no device
 * needed); *count receives its record count. */
int kv_tiles_inspect(const char* path, long long tile_bytes, int* count);

/* ------------------------------------------------------------------------ */
/* Decoder (CUDADecoder / INT8Decoder, decoder/cuda_decoder.hpp:7-21,        */
/* decoder/int8_decoder.hpp:6-17)                                            */
/* ------------------------------------------------------------------------ */
typedef struct llm_decoder llm_decoder;

typedef struct llm_decoder_config {
  int num_layers, num_heads, head_dim, hidden_dim, vocab_size, max_seq_len; /* ctor args, bindings.cpp:6 */
  int inter_dim;        /* 0 -> 4*hidden_dim (decoder_block.hpp:28) */
  int page_size;        /* 0 -> 16 */
  int weight_dtype;     /* LLM_I8 (INT8Decoder) or LLM_F16 (CUDADecoder) */
  int max_batch;        /* rows decoded together (0 -> 1) */
  float attn_scale;     /* score multiplier; 1.0 = reference (no 1/sqrt(D)) */
  long long num_pages;  /* KV page-pool size; 0 -> enough for max_batch * max_seq_len */
} llm_decoder_config;

int llm_decoder_create(const llm_decoder_config* cfg, llm_decoder** out);
/* llm_decoder_create with KV pools of kv_dtype: LLM_F16 (identical to
 * llm_decoder_create) or LLM_FP8 (the qkv projection appends e4m3 bytes, the
 * attention reads them; the default num_pages is the same number of pages, so
 * the pool is half the bytes).  Any other element type is LLM_ERR_UNSUPPORTED,
 * an unknown one LLM_ERR_INVALID, decided before any device allocation.
 * Prompt chunks of an LLM_FP8 decoder run their attention on the MFMA prefill
 * kernel for the shapes an fp16-KV decoder does (llm_decoder_prefill_kernel). */
int llm_decoder_create_kv(const llm_decoder_config* cfg, int kv_dtype, llm_decoder** out);
/* Per-layer scales of an LLM_FP8 decoder: host arrays [num_layers], NULL = all
 * 1.0 (the default), every value finite and > 0.  Allowed only while no rows
 * are active (before begin_* / generate / prefill), else LLM_ERR_INVALID; on
 * an fp16-KV decoder LLM_ERR_INVALID.  k_scale is folded into the attention's
 * score multiplier and v_scale multiplies the normalised attention output
 * once per (row, head), before anything downstream rounds it.  Scales are
 * stored in no file. */
int llm_decoder_set_kv_scales(llm_decoder* d, const float* k_scale, const float* v_scale);
/* LLM_F16 or LLM_FP8. */
int llm_decoder_kv_dtype(const llm_decoder* d);
/* Rotary position embedding of the decoder (the per-position interleaved
 * rotation of attention/attention_kernel_utils.cuh:20-35, see rope_rows):
 * table is a host array [max_seq_len][head_dim] in llm_rope_table's layout,
 * copied to the device; NULL turns rotation off (the default).  The qkv
 * projection then rotates q and K by each row's position in its epilogue,
 * before q is stored and before K is rounded into the pages (fp16 or e4m3,
 * after the multiplication by 1 / k_scale); V is not rotated.  Decode steps,
 * prompt chunks and packed prefill passes alike.  Allowed only while no rows
 * are active, else LLM_ERR_INVALID; LLM_ERR_INVALID too for an odd head_dim
 * or a non-finite entry.  The table is stored in no file: a KV snapshot
 * written with rotation on holds rotated K and must be loaded into a decoder
 * with the same table. */
int llm_decoder_set_rope(llm_decoder* d, const float* table);
/* 1: a rotary table is set, 0: none, -1 for NULL
 * (attention/attention_kernel_utils.cuh:20-35). */
int llm_decoder_rope(const llm_decoder* d);
/* Sliding-window attention of the decoder: every layer's attention at
 * position p reads positions max(0, p - window + 1) .. p only -- decode steps
 * (pa_decode_window), prompt chunks and packed prefill passes
 * (pa_prefill_window / pa_prefill_packed_window, or the decode kernel where
 * llm_decoder_prefill_kernel says LLM_PREFILL_DECODE).  window 0 (the default)
 * is off.  As a row advances, the pages wholly below its window are released
 * (kv_cache_release_before) before each step and each prefill pass, so a pool
 * of about ceil((window + 512) / page_size) + 1 tiles per (row, layer, head)
 * carries a row to max_seq_len, which still bounds positions.  Allowed only
 * while no rows are active, else LLM_ERR_INVALID; window < 0 LLM_ERR_INVALID.
 * With a window set, llm_decoder_begin_beams and llm_decoder_beam_search
 * return LLM_ERR_UNSUPPORTED (any beam width).  The window is stored in no
 * file. */
int llm_decoder_set_window(llm_decoder* d, int window);
/* The decoder's window (0: off), -1 for NULL. */
int llm_decoder_window(const llm_decoder* d);
/* The attention kernel prompt chunks (llm_decoder_prefill, the prompts of
 * llm_decoder_generate) of this decoder's pools take: LLM_PREFILL_MFMA
 * (pa_prefill: fp16 or LLM_FP8 pools, head_dim 64 or 128, page_size 16 or 32)
 * or LLM_PREFILL_DECODE (every other shape: the decode kernel, one row per
 * prompt token).  -1 for NULL. */
enum { LLM_PREFILL_DECODE = 0, LLM_PREFILL_MFMA = 1 };
int llm_decoder_prefill_kernel(const llm_decoder* d);
void llm_decoder_destroy(llm_decoder* d);

/* Host weights (row-major reference layouts), uploaded and packed on device.
 * INT8: wqkv [L][hid][3hid] (q|k|v, heads contiguous), wo [L][hid][hid],
 * w1 [L][hid][inter], w2 [L][inter][hid] int8 + per-output-column fp32 dequant
 * scales; biases b1 [L][inter], b2 [L][hid]; LayerNorm gamma/beta [L][hid];
 * emb fp16 [V][hid] (embedding and tied LM head). */
typedef struct llm_int8_weights {
  const uint16_t* emb;
  const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
  const int8_t* wqkv; const float* sw_qkv;
  const int8_t* wo;   const float* sw_o;
  const int8_t* w1;   const float* sw1; const float* b1;
  const int8_t* w2;   const float* sw2; const float* b2;
} llm_int8_weights;
int llm_decoder_set_int8_weights(llm_decoder* d, const llm_int8_weights* w);

typedef struct llm_f16_weights {
  const uint16_t* emb;
  const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
  const uint16_t *wqkv, *wo, *w1, *w2;   /* fp16, same [K][N] layouts */
  const float *b1, *b2;
} llm_f16_weights;
int llm_decoder_set_f16_weights(llm_decoder* d, const llm_f16_weights* w);

/* CUDADecoder::load_weights (decoder/cuda_decoder.cu:35-45) / INT8Decoder::
 * load_quantized_weights (decoder/int8_decoder.cpp:91-95) / quantize_weights
 * (:43-89) over the raw little-endian .bin layout of weights/README.md:26-38. */
int llm_decoder_load_weights(llm_decoder* d, const char* dir);
int llm_decoder_load_quantized_weights(llm_decoder* d, const char* dir);
int llm_quantize_weights(const char* fp32_dir, const char* int8_dir, int num_layers,
                         int hidden_dim, int inter_dim, int vocab_size);

/* Batched generate (CUDADecoder<T>::generate, decoder/cuda_decoder.cu:48-61,
 * batched): for each row, prompt tokens are consumed one per step (KV is
 * appended), then max_gen_len tokens are produced by greedy argmax.  out
 * [batch][max_gen_len] receives the generated ids (prompt excluded).  A step
 * whose fused o_proj clamped does not stop generation: `out` is filled to the
 * end and LLM_ERR_RANGE is returned afterwards. */
int llm_decoder_generate(llm_decoder* d, const int32_t* prompts, const int32_t* prompt_lens,
                         int prompt_stride, int batch, int max_gen_len, float temperature,
                         int32_t* out);

/* Beam search over shared prompts (what the reference's stream_chat_beam,
 * api/router.py, and enable_beam_search stand for: they call greedy generate
 * beam_width times and get one text beam_width times).  num_seqs prompts, W =
 * beam_width beams each, rows seq * W + beam; num_seqs * W <= max_batch.
 * Set-up: prompt[:-1] is prefilled into beam 0's row and forked to the other
 * beams (shared pages, kv_cache_fork); scores start {0, -inf, ...}.
 * Each step: the step graph in beam mode (the LM head, then beam_select_rows'
 * two launches in place of argmax / sampling), the 2W candidates per sequence
 * copied to the host, the bookkeeping below, kv_cache_reorder per sequence (the
 * next step's append copies the shared tail page on write), new scores and
 * tokens uploaded.
 * Bookkeeping, per sequence, candidates walked in rank order: a candidate whose
 * token is eos_token joins the finished set if its rank is < W and is ignored
 * otherwise; any other candidate becomes the next live beam (slot = order of
 * appearance) until W are live.  A sequence with >= W finished hypotheses is
 * done: it keeps stepping the same way but records nothing more, and its live
 * beams are not results.  The search ends when every sequence is done or after
 * max_new_tokens steps; the live beams of a sequence that is not done then
 * join its finished set (in beam order) as unterminated hypotheses.  Final
 * score = sum_logprob / len^length_penalty (len = generated tokens, EOS
 * included; computed in double, stored as float); the best W by final score
 * (equal scores: the earlier entry) are returned best first.
 * out_ids [num_seqs][W][max_new_tokens] (padded with -1), out_len / out_sum_logprob /
 * out_score [num_seqs][W].  Traces (any may be NULL) hold, per step, the device's
 * candidates, the live beams chosen (parent slot and token) and the step's logits.
 * Afterwards the W rows of every sequence stay active (the last live beams,
 * row_group = W), so llm_decoder_context_len / attention_plan / kv apply.
 * Both weight types, fp16 and LLM_FP8 pools; vocab_size in [2W, 65536].
 * A set sampling mode is suspended as in llm_decoder_generate; LLM_ERR_RANGE
 * as there (results complete). */
typedef struct llm_beam_options {
  int beam_width;        /* 1..4 */
  int max_new_tokens;    /* >= 1 */
  int eos_token;         /* -1: none */
  float length_penalty;  /* alpha >= 0; final score = sum_logprob / len^alpha, len = generated tokens incl. EOS */
  /* optional traces, host unless noted; NULL = off */
  int32_t* trace_cand_parent; int32_t* trace_cand_token; float* trace_cand_score; /* [steps][num_seqs][2W] */
  int32_t* trace_live_parent; int32_t* trace_live_token;                          /* [steps][num_seqs][W]  */
  float* trace_logits_dev;                                                         /* device [steps][rows][V] */
  int* steps_run;
} llm_beam_options;

int llm_decoder_beam_search(llm_decoder* d, const int32_t* prompts, const int32_t* prompt_lens,
                            int prompt_stride, int num_seqs, const llm_beam_options* opt,
                            int32_t* out_ids, int32_t* out_len, float* out_sum_logprob,
                            float* out_score);

/* Chunked prefill (the is_prefill pass of AttentionCUDA::forward,
 * attention/attention_cuda.hpp:21): append the n tokens (host ids) of active
 * row `row` at its next positions in one layer pass per chunk of <= 512 tokens
 * (M = chunk weight GEMMs; causal paged attention per token), then set the
 * row's next token from the last token's logits, so llm_decoder_step(tokens =
 * NULL) continues decoding.  llm_decoder_generate uses it for every prompt. */
int llm_decoder_prefill(llm_decoder* d, int row, const int32_t* tokens, int n);

/* Packed prefill: llm_decoder_prefill of several rows at once.  Row rows[i]
 * (active, distinct) gets the next lens[i] >= 0 ids of `tokens` (host, the
 * rows' ids concatenated; 0 skips the row).  The tokens go through layer
 * passes of <= 512 PACKED tokens, filled greedily in row order: a pass holds
 * segments of several rows (every weight GEMM at M = the pass, one
 * pa_prefill_packed launch per layer; the decode kernel where
 * llm_decoder_prefill_kernel is LLM_PREFILL_DECODE), a long prompt continues
 * in the next pass and a row is never in one pass twice.  Each row ends as
 * after llm_decoder_prefill: its next token chosen from its last token's
 * logits.  Every argument is checked before the first launch (rows active and
 * distinct, ids in range, position + len < max_seq_len): on LLM_ERR_INVALID no
 * row has moved. */
int llm_decoder_prefill_rows(llm_decoder* d, const int32_t* rows, const int32_t* tokens,
                             const int32_t* lens, int nrows);
/* on != 0: llm_decoder_generate and the prompt set-up of
 * llm_decoder_beam_search prefill all their rows through
 * llm_decoder_prefill_rows; 0 (the default): row by row, exactly as before.
 * llm_decoder_prefill is unaffected.  The getter returns the switch (-1: NULL). */
int llm_decoder_set_packed_prefill(llm_decoder* d, int on);
int llm_decoder_packed_prefill(const llm_decoder* d);

/* Teacher-forced scoring through the prefill passes: tokens host
 * [nseq][stride], lens[s] >= 1 ids each; out_logprob host [nseq][stride]:
 *   out[s][i] = log p(tokens[s][i] | tokens[s][0 .. i-1])   for 1 <= i < lens[s]
 * (logprob() of lm_head_logprobs), out[s][0] = 0, entries from lens[s] on are
 * untouched.  Sequences are taken in order in groups of at most max_batch rows
 * whose page needs -- per sequence the pages of lens[s] - 1 positions, by the
 * rule a served request is charged (window-aware) -- fit the pool together.
 * Each group's tokens[:len-1] go through llm_decoder_prefill_rows' packed
 * passes if packed prefill is on, else row by row; after the layers of each
 * pass ONE lm_head_logprobs launch pair runs over all packed rows against
 * their next tokens, and only one value per row is copied back: no logits are
 * materialised and the pass's own token choice is skipped.  lens[s] == 1
 * produces nothing.  LLM_ERR_INVALID with nothing run: lens[s] < 1 or > stride,
 * an id out of range, lens[s] - 1 >= max_seq_len, a sequence whose need
 * exceeds the pool, or while serving.  Works with both weight types, fp16 /
 * LLM_FP8 pages, rope, a window and packed prefill.  On return no rows are
 * active and the cache is clear, as after llm_decoder_serve_end.  (Prefill
 * passes never run the fused o_proj, so LLM_ERR_RANGE does not arise here.) */
int llm_decoder_score(llm_decoder* d, const int32_t* tokens, const int32_t* lens, int stride,
                      int nseq, float* out_logprob);

/* Token choice of every following step: greedy argmax (temperature <= 0 or
 * top_k == 1; the default, sample_from_logits, decoder/cuda_decoder.cu:7-14)
 * or device sampling with temperature / top_k / top_p (sample_rows; the draw
 * counter of a row is its position, so runs are replayable for a seed). */
int llm_decoder_set_sampling(llm_decoder* d, float temperature, int top_k, float top_p,
                             uint64_t seed);

/* ------------------------------------------------------------------------ */
/* Continuous batching (serving mode)                                        */
/* ------------------------------------------------------------------------ */
/* Requests are submitted at any time; each llm_decoder_serve_step admits
 * waiting requests into free rows, prefills them, runs ONE decode step over
 * all live rows and hands back one token per live request; a row whose request
 * ended is retired at once and its pages return to the pool.  Policy
 * (csrc/serve_plan.hpp):
 *   pages   a request appends at most T = prompt_len + max_new_tokens - 1
 *           positions (llm_decoder_generate's bound) and is charged
 *           num_layers * num_heads * tiles pages while it lives, tiles =
 *           ceil(T / page_size), on a windowed decoder min(tiles,
 *           ceil((window + 512) / page_size) + 1) (llm_decoder_set_window);
 *   admit   strict FIFO at the start of a step: the head of the queue enters
 *           while a row is free and committed + need(head) <= num_pages; a
 *           head that does not fit is not skipped.  So no step of an admitted
 *           request returns LLM_ERR_OOM; nothing is preempted;
 *   rows    live rows are dense, 0 .. live - 1: a new request takes row
 *           `live`; after a step the finished rows retire in descending row
 *           order, and a retired row that is not the last live row receives
 *           the last one (a page-table re-parenting: no page is copied).  A
 *           request's row therefore changes over its life; events carry ids;
 *   finish  LLM_FINISH_EOS when the chosen token is the request's eos_token
 *           (the token is delivered, as llm_decoder_beam_search counts it),
 *           LLM_FINISH_LENGTH after max_new_tokens tokens; EOS wins.
 * Every decoder mode but beams composes: both weight types, fp16 / LLM_FP8
 * pages, rope, a sliding window, packed prefill.  Nothing outside serving
 * mode changes. */
#define LLM_FINISH_EOS 1
#define LLM_FINISH_LENGTH 2
typedef struct llm_request_options {
  int max_new_tokens;            /* >= 1 */
  int eos_token;                 /* -1: none */
  float temperature; int top_k; float top_p;  /* as llm_decoder_set_sampling; greedy if temperature <= 0 or top_k == 1 */
  uint64_t seed;
} llm_request_options;
typedef struct llm_serve_event {
  long long id; int32_t token; int32_t index;  /* 0-based generated index */
  int32_t row;                                 /* the row it held during this step */
  int32_t finish;                              /* 0, LLM_FINISH_EOS, LLM_FINISH_LENGTH */
} llm_serve_event;
/* Enter serving mode: the cache and the rows are cleared (row_group 1), ids
 * count up from 0 again.  LLM_ERR_UNSUPPORTED in beam mode or with
 * vocab_size > 65536 (every row's token is chosen by sample_rows_each),
 * LLM_ERR_INVALID if already serving or without weights.  While serving,
 * llm_decoder_generate, _beam_search, _begin_synthetic, _begin_beams,
 * _prefill, _prefill_rows, _step and the setters _set_sampling, _set_window,
 * _set_rope, _set_kv_scales, _set_packed_prefill and _set_taps return
 * LLM_ERR_INVALID. */
int llm_decoder_serve_begin(llm_decoder* d);
/* llm_decoder_serve_begin with options (llm_decoder_serve_begin is this call
 * with every option 0).
 * prefix_cache != 0: for the length of this session -- until
 * llm_decoder_serve_end -- prompt blocks outlive the rows that computed them,
 * and a request whose prompt begins with cached blocks is not prefilled over
 * them (csrc/serve_plan.hpp, csrc/prefix_cache.hpp).  A block is page_size
 * consecutive prompt positions from a multiple of page_size on, over all
 * layers and heads (kv_cache_hold_tile); two prompts share it exactly when
 * they agree on every token id up to its end.
 *   hit      a prompt of n tokens prefills n - 1 positions and hits at most
 *            floor((n - 1) / page_size) blocks: the longest cached chain from
 *            its start.  At admission those pages are attached to its row
 *            (kv_cache_attach_tile), the row starts at hit_blocks * page_size
 *            and prompt[hit_blocks * page_size : n - 1] is prefilled -- maybe
 *            nothing.  Nothing ever appends into a shared tile, so no page is
 *            copied on write;
 *   publish  after its admission prefill a new row publishes the full tiles
 *            it computed, up to the first whose block is cached already.
 *            Generated tokens are not published;
 *   step     admission ends before a head whose first uncached block a
 *            request admitted earlier in the same step will publish; it
 *            enters at the next step with the hit (counted as a deferral);
 *   pages    committed_pages = the live requests' private needs +
 *            num_layers * num_heads per block in use; a request's private
 *            need is its need less its hit blocks', less what it published.
 *            Cached blocks nobody uses hold idle_pages.  committed_pages +
 *            idle_pages <= num_pages at all times: before the head is
 *            admitted, idle blocks are evicted (those without a cached child,
 *            least recently used first; kv_cache_drop_pages) until that
 *            holds with it, and it waits if evicting all would not do.  So no
 *            step of an admitted request returns LLM_ERR_OOM.  A submit is
 *            still checked against the whole pool with its full need.
 * Composes with both weight types, fp16 / LLM_FP8 pages, rope and packed
 * prefill; LLM_ERR_UNSUPPORTED with a sliding window set (its page release
 * and its charge do not compose with held blocks).  LLM_ERR_INVALID for an
 * option that is neither 0 nor 1. */
typedef struct llm_serve_options {
  int prefix_cache;  /* 0 (off) or 1 */
} llm_serve_options;
int llm_decoder_serve_begin_opts(llm_decoder* d, const llm_serve_options* opt);
/* The prefix cache's counters for the current session; all 0 outside a
 * session begun with prefix_cache. */
typedef struct llm_prefix_stats {
  long long positions_due;   /* the sum of n - 1 over the admitted requests */
  long long positions_hit;   /* ... of which served from cached blocks */
  long long cached_blocks;   /* blocks cached now, used or idle */
  long long idle_pages;      /* pages of the cached blocks nobody uses */
  long long evicted_blocks;  /* blocks evicted so far */
  long long deferrals;       /* admissions ended by the same-step rule */
} llm_prefix_stats;
int llm_decoder_serve_prefix_stats(const llm_decoder* d, llm_prefix_stats* out);
/* Leave serving mode: every request, waiting or live, is dropped without an
 * event, the cache is cleared (a prefix cache's blocks with it) and no rows
 * stay active (batch 0).
 * LLM_ERR_INVALID if not serving. */
int llm_decoder_serve_end(llm_decoder* d);
/* Queue a request of n >= 1 prompt ids (host; copied); *id receives its id
 * (64-bit, counting up from 0 per llm_decoder_serve_begin).  Launches nothing.
 * LLM_ERR_INVALID, with nothing queued, for a token id or eos_token out of
 * range, top_k < 0, top_p outside (0, 1], a temperature that is not finite,
 * T > max_seq_len, or a need above the pool's num_pages. */
int llm_decoder_submit(llm_decoder* d, const int32_t* prompt, int n,
                       const llm_request_options* opt, long long* id);
/* llm_decoder_submit for a request that wants log-probabilities: top_logprobs
 * 0 asks for the chosen token's only, 1 .. LLM_MAX_TOP_LOGPROBS for that many
 * top alternatives beside it; < 0 or > 8 is LLM_ERR_INVALID.  (llm_decoder_submit
 * asks for nothing.)  A step whose live rows include at least one asking request
 * carries one more launch after sample_rows_each: logprob_rows over ALL live
 * rows with chosen = the step's ids and top_n = 8 -- constants that do not
 * depend on the request mix -- and device-to-host copies that complete with
 * the step's own synchronisation.  Whether the launch is in the step graph is
 * part of the graph's identity: a change re-instantiates it and counts in
 * graph_instantiations.  A run in which nobody asks executes exactly the graph
 * of llm_decoder_submit-only serving. */
int llm_decoder_submit_logprobs(llm_decoder* d, const int32_t* prompt, int n,
                                const llm_request_options* opt, int top_logprobs, long long* id);
/* The last llm_decoder_serve_step's log-probabilities, in event (row) order:
 * host arrays chosen_lp [max_batch], top_lp / top_id [max_batch][8], top_n
 * [max_batch].  top_n[r] is event r's request's count (its first top_n[r]
 * entries of row r are valid, ordered as logprob_rows orders them), or -1 for a
 * request that did not ask: its entries are then unspecified.  Any array may
 * be NULL.  LLM_ERR_INVALID if not serving. */
int llm_decoder_serve_logprobs(llm_decoder* d, float* chosen_lp, float* top_lp, int32_t* top_id,
                               int32_t* top_n);
/* Drop a request: a waiting one leaves the queue, a live one is retired at
 * once by the row move of a retirement (nothing is in flight between steps)
 * and its pages return.  No event is emitted.  Unknown or finished id:
 * LLM_ERR_INVALID. */
int llm_decoder_cancel(llm_decoder* d, long long id);
/* One serving step, in this order: (1) admit; (2) prefill prompt[:-1] of
 * every newly admitted row (llm_decoder_prefill_rows' passes if packed
 * prefill is on, else row by row -- as llm_decoder_generate; live rows wait
 * for it); (3) one decode step of all live rows, fed the last prompt token
 * (new rows) or the previous chosen id, so a request's first token is
 * produced exactly as llm_decoder_generate produces it; every row's token is
 * chosen on the device by ONE sample_rows_each launch over the rows' own
 * settings, the draw counter being the row's position; (4) one event per live
 * row, in ascending row order; (5) finished rows retire.  logits_dev (device,
 * may be NULL) receives the step's fp32 logits, row r of the events at
 * logits_dev + r * vocab_size.  events has room for cap >= max_batch entries;
 * *n_events receives the count.  With nothing live and nothing admissible the
 * call launches nothing and returns *n_events = 0.  The decoder keeps one
 * instantiated step graph, as llm_decoder_step does: a step whose live-row
 * count differs from the last one's re-instantiates it
 * (llm_decoder_serve_stats counts these).
 * LLM_ERR_RANGE as llm_decoder_generate: the events are complete.  After any
 * other error of a step the rows are in no defined state: leave the mode
 * with llm_decoder_serve_end. */
int llm_decoder_serve_step(llm_decoder* d, float* logits_dev, llm_serve_event* events, int cap,
                           int* n_events);
/* *live / *waiting requests, *committed_pages (the sum of the live requests'
 * needs; with a prefix cache, of their private needs and the blocks in use) and *graph_instantiations (step graphs instantiated by serving
 * steps since the decoder was created).  Any pointer may be
 * NULL; valid outside serving mode too (0 live, 0 waiting). */
int llm_decoder_serve_stats(const llm_decoder* d, int* live, int* waiting,
                            long long* committed_pages, long long* graph_instantiations);

/* Low-level stepping (bench / multi-GPU driver). */
/* Start `batch` rows whose first context_len tokens are synthetic: every page
 * is allocated (shuffled order when shuffle != 0) and filled with seeded
 * random fp16 K/V on device (LLM_FP8 decoders: the same seeded values encoded
 * at scale 1, whatever the layers' scales -- the pool bytes depend on the
 * seed only, and a layer reads them times its scales). */
int llm_decoder_begin_synthetic(llm_decoder* d, int batch, int context_len, uint64_t seed,
                                int shuffle);
/* Start num_seqs * beam_width rows (row = seq * beam_width + beam) for beam
 * decode: each sequence's first shared_len tokens live in beam 0's pages and
 * are shared by the other beams through kv_cache_fork (refcounted, copy-on-
 * write on append); every beam then holds beam_len private tokens.  Pages hold
 * seeded random fp16 K/V.  Attention runs beam-aware (pa_decode_grouped with
 * row_group = beam_width, 1..4). */
int llm_decoder_begin_beams(llm_decoder* d, int num_seqs, int beam_width, int shared_len,
                            int beam_len, uint64_t seed, int shuffle);
/* One decode step for all active rows: tokens (host [batch], or NULL to feed
 * back the previous argmax) at each row's next position; writes fp32 logits
 * to logits_dev ([batch][V] device, may be NULL) and copies next ids to
 * next_host (may be NULL; a NULL next_host keeps the step asynchronous).
 * stream NULL -> the decoder's own stream. */
int llm_decoder_step(llm_decoder* d, const int32_t* tokens, float* logits_dev,
                     int32_t* next_host, void* stream);
/* Wait for the device.  LLM_ERR_RANGE if, since the last report, a step's
 * fused o_proj (FP16 decoders, LLM_PA_FORM_OPROJ) met a head product outside
 * its fixed-point range ((2^23 - 1) / num_heads in magnitude, or not finite):
 * that product was clamped, so the affected x values are wrong, but the
 * accumulator columns stayed consistent and later steps are unaffected by it.
 * A step with next_host reports the same.  Each clamp is reported once: the
 * report clears the device flag, so later steps and syncs succeed unless they
 * clamp again.  llm_decoder_run_attention launches carry a flag of their own
 * and never make a step or a sync fail. */
int llm_decoder_sync(llm_decoder* d);
/* Health of the fused o_proj after waiting for the device: *clamped = 1 if a
 * step's term was clamped since the last begin / generate, reported or not
 * (see llm_decoder_sync),
 * *nonzero_columns = accumulator columns not back at zero (0 between steps
 * unless a launch was interrupted).  Either pointer may be NULL.  Decoders
 * without the fused o_proj report 0 / 0. */
int llm_decoder_oproj_status(llm_decoder* d, int* clamped, long long* nonzero_columns);
/* Enqueue on `stream` (NULL: the decoder's) a device copy of the last step's
 * next ids (int32 [batch], the greedy argmax or the sampled ids) to dst_dev:
 * the ids-only gather of the multi-GPU path without a host sync. */
int llm_decoder_copy_next(llm_decoder* d, int32_t* dst_dev, void* stream);
/* Activation taps for parity checks: every following
 * llm_decoder_step also copies, per layer l and stage s (0: LN1 output, 1:
 * attention output, 2: LN2 output, 3: fc1 output -- the four int8 GEMM inputs
 * of DecoderBlock::forward, decoder/decoder_block.hpp:43-61), the rows' int8
 * activations in packed-A order (common.hpp a_frag_off_i8) to
 *   q_dev + ((l*4 + s) * ceil(max_batch/16)*16 + row) * K   (K = hidden_dim, or
 *                                                           inter_dim at s = 3;
 *   slot stride ceil(max_batch/16)*16 * max(hidden_dim, inter_dim) bytes)
 * and their fp32 dequantisation scales to s_dev[(l*4 + s) * max_batch + row].
 * FP16 decoders (CUDADecoder) tap their four fp16 GEMM inputs in packed-A
 * order (a_frag_off_f16), at the same slot layout with 2 bytes per element;
 * s_dev is not written (give any device buffer).
 * Both NULL switches the taps off.  Prefill chunks are not tapped. */
int llm_decoder_set_taps(llm_decoder* d, int8_t* q_dev, float* s_dev);
/* The attention launch of the decoder's step at its current batch and row
 * group (pa_decode_plan of layer 0's view, T = max_seq_len: the step graph's
 * launch, whose split lengths follow each row's live context).  INT8 decoders
 * whose o_proj quantises its own input (decode rows <= 64, hidden <= 2048, no
 * beam groups) report the fp32-row forms (LLM_PA_FORM_WG_MERGE up to 8
 * splits, else LLM_PA_FORM_SPLIT_MERGE, LLM_PA_FORM_DIRECT); wider models
 * LLM_PA_FORM_WG_MERGE when their fp32-row plan is one (a quantise launch
 * follows it), else LLM_PA_FORM_SPLIT_MERGE_ROW; beam groups
 * LLM_PA_FORM_SPLIT_MERGE_ROW | LLM_PA_FORM_BEAM.  FP16
 * decoders whose launch merges in the workgroup (2..8 splits, head_dim <= 128,
 * <= 64 heads) run o_proj inside it: LLM_PA_FORM_WG_MERGE | LLM_PA_FORM_OPROJ. */
int llm_decoder_attention_plan(llm_decoder* d, int* nsplit, int* form);
/* Enqueue layer `layer`'s attention launch of the decoder's step on `stream`
 * (NULL: the decoder's) -- the same kernels, grid and outputs as inside the
 * step graph (q from the last step's projection, each row's live context, the
 * o_proj input written), for timing the step's own launch in isolation.  The
 * fused o_proj of an FP16 decoder accumulates into a scratch set of columns of
 * its own here (not the step's), so a run may overlap an in-flight step; two
 * runs of one decoder must not overlap each other. */
int llm_decoder_run_attention(llm_decoder* d, int layer, void* stream);
int llm_decoder_context_len(const llm_decoder* d, int row);
kv_cache* llm_decoder_kv(llm_decoder* d);

#ifdef __cplusplus
}
#endif

#endif /* LLM_DECODER_H_ */
