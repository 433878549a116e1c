// Decoder runtime (host side, compiled as HIP): CUDADecoder / INT8Decoder
// (decoder/cuda_decoder.{hpp,cu}, decoder/int8_decoder.{hpp,cpp}) re-designed
// for batched incremental decode on one MI355X.
//
// One decode step for all rows (reference layer order of
// DecoderBlock<T>::forward, decoder/decoder_block.hpp:41-62 — no residuals —
// plus the BUILD DECISION projections):
//   embed -> per layer { LN1+quant -> qkv GEMM -> KV append -> paged attention
//   -> quant -> o GEMM -> LN2+quant -> fc1 GEMM (+b1, ReLU) -> quant -> fc2 GEMM
//   (+b2) } -> LM head (tied fp16 embedding) -> argmax -> advance positions.
// The reference re-embeds and recomputes the whole prefix every step
// (decoder/cuda_decoder.cu:52-57) and runs B = 1; here the KV cache is
// appended in place and the step is O(T) per row.
//
// The device part of a step is captured once per batch size into a hipGraph
// and replayed; per-step state (positions, context lengths, tokens) lives in
// device memory, so replays need no re-capture.  Only page allocation (a new
// page every page_size tokens, copy-on-write of forked pages) happens on the
// host between replays and is pushed with kv_cache_sync().
// Beam search (llm_decoder_beam_search) replays the same graph in beam mode:
// the token choice is beam_select_rows' two launches, and between replays the
// host ranks the hypotheses and re-parents the rows' pages (kv_cache_reorder).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <mutex>
#include <numeric>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "gemm.hpp"
#include "kv_cache_impl.hpp"
#include "pa_decode.hpp"
#include "prefill_pack.hpp"
#include "row_ops.hpp"
#include "serve_plan.hpp"

using namespace llm;

// f[1] = f[0], f[0] = 0 in one device atomic: the fused o_proj's range flag
// read and cleared (llm_decoder::report_range)
__global__ void take_flag_kernel(int* f) { f[1] = atomicExch(f, 0); }

namespace {

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int alloc(size_t count) {
    if (p) { (void)hipFree(p); p = nullptr; }
    n = count;
    if (count == 0) return LLM_OK;
    if (hipMalloc(&p, count * sizeof(T)) != hipSuccess) {
      (void)hipGetLastError();
      return fail(LLM_ERR_OOM, "decoder: device allocation of " + std::to_string(count * sizeof(T)) +
                                   " bytes failed");
    }
    return LLM_OK;
  }
};

#define RET_IF(x) do { int _rc = (x); if (_rc) return _rc; } while (0)

}  // namespace

struct llm_decoder {
  llm_decoder_config cfg{};
  int L = 0, H = 0, D = 0, hid = 0, inter = 0, V = 0, TS = 0, max_tiles = 0, maxB = 0;
  int wdtype = LLM_I8;
  int pps = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;

  // weights
  DevBuf<uint16_t> emb;
  DevBuf<uint8_t> emb_packed;  // LM-head copy of emb in B-fragment order
  DevBuf<float> ln1_g, ln1_b, ln2_g, ln2_b, b1, b2, sw_qkv, sw_o, sw1, sw2;
  DevBuf<uint8_t> wqkv, wo, w1, w2;  // packed, L consecutive blocks
  // FP16: W_o again as per-head column slices for the fused o_proj,
  // [L][H][D/8][hid][8] (PaRowOutputs::wo_heads)
  DevBuf<uint16_t> wo_heads;
  size_t sz_qkv = 0, sz_o = 0, sz_1 = 0, sz_2 = 0;
  bool weights_ready = false;
  int w_keep = 0;  // the GEMM weights fit the Infinity Cache: keep them there (w_keep_for)

  // KV: fp16 pools, or LLM_FP8 bytes (csrc/fp8.hpp) with one K and one V
  // scale per layer (llm_decoder_set_kv_scales; host copies: the step graph
  // carries them as kernel arguments and is re-captured when they change)
  kv_cache* kv = nullptr;
  int kvt = LLM_F16;
  std::vector<float> k_scale, v_scale;
  // rotary table [max_seq_len][D] (llm_decoder_set_rope; device copy, kept
  // once allocated): the qkv projection's epilogue rotates q and K by it
  // (layer_pre).  Like the scales it is a kernel argument of the step graph
  // and is stored in no file.
  DevBuf<float> rope;
  bool rope_on = false;
  // sliding-window attention (llm_decoder_set_window; 0: off): every attention
  // launch takes it, and the pages wholly below a row's window are released
  // before each step / prefill pass
  int window = 0;

  // activations / state
  DevBuf<float> x, qkv, o, h1, logits, sa;
  DevBuf<float> lm_pv;    // [max_batch][lm_nwg] LM-head argmax partials
  DevBuf<int32_t> lm_pi;
  int lm_nwg = 0;
  DevBuf<int8_t> qa;
  DevBuf<uint16_t> a16;
  // FP16: the fused o_proj's int64 columns [max_batch][hid] (zero between
  // attention launches: the adder completing a column clears it); oacc_run:
  // llm_decoder_run_attention's own set (allocated on first use), so a timed
  // run never mixes its arrivals with an in-flight step's; oflag: the range
  // guard's device flag of the steps (common.hpp oacc_term), h_oflag its pinned
  // host copy (written and read under mu only); oflag_run: run_attention's own
  // flag, so a clamp in a timing re-run is never blamed on a step.
  // range_clamped: a clamp was reported since the last begin / generate (what
  // llm_decoder_oproj_status returns; the device flag is cleared on report)
  DevBuf<long long> oacc, oacc_run;
  DevBuf<int> oflag, oflag_run;
  int* h_oflag = nullptr;
  int range_clamped = 0;
  // beam-group attention (row_group 4): the dynamic tile counters
  // (PaRowOutputs::beam_ctr), zero at create and left at zero by every launch
  DevBuf<unsigned> beam_ctr;
  int oproj_range_status();
  int report_range(int flag);
  DevBuf<int32_t> tokens, pos, ctx;
  DevBuf<uint8_t> attn_ws;
  size_t attn_ws_bytes = 0;

  int batch = 0;
  std::vector<int> h_pos;  // host mirror of the next position of each row

  hipGraphExec_t graph = nullptr;
  int graph_batch = -1;

  // activation taps (llm_decoder_set_taps): the int8 GEMM inputs and row scales
  // of every layer, copied out by the step for teacher-forced parity checks
  int8_t* tap_q = nullptr;
  float* tap_s = nullptr;
  int tap(int l, int stage, const struct Rows& R, int K, hipStream_t st);
  int layer_norm_into(WeightGemm& g, const struct Rows& R, const float* gamma, const float* beta,
                      hipStream_t st, float* zero_x = nullptr, const LnSource* emb = nullptr);

  ~llm_decoder() {
    if (h_oflag) (void)hipHostFree(h_oflag);
    if (graph) (void)hipGraphExecDestroy(graph);
    if (kv) kv_cache_destroy(kv);
    if (stream) (void)hipStreamDestroy(stream);
  }

  int row_group = 1;  // beam width of llm_decoder_begin_beams (beam-aware attention)
  // sampling (llm_decoder_set_sampling); greedy argmax by default, as the
  // reference's sample_from_logits (decoder/cuda_decoder.cu:7-14)
  float temperature = 0.f;
  int top_k = 0;
  float top_p = 1.f;
  uint64_t sample_seed = 0;
  bool use_graph = true;  // LLM_GRAPH=0: eager launches (per-kernel profiling)
  // beam search (llm_decoder_beam_search): in beam mode the step's token choice
  // is beam_select_rows' two launches over the rows' cumulative scores
  // (beam_score, uploaded by the search between steps), whose 2W candidates
  // per sequence run_step copies to h_cand: [score | parent | token] blocks of
  // 2 * batch 4-byte items each.  Entering / leaving the mode re-captures the graph.
  bool beam_mode = false;
  DevBuf<float> beam_score, beam_ws, cand_score;
  DevBuf<int32_t> cand_parent, cand_token;
  std::vector<int32_t> h_cand;
  int qa_ld = 0;
  size_t b16 = 0;  // max_batch rounded up to 16-row tiles

  int layer_pre(int l, hipStream_t st, const struct Rows& R, const LnSource* emb = nullptr);
  int layer_attn(int l, hipStream_t st, const struct Rows& R);
  int attn_request(const struct Rows& R, pa_kv_view* view, PaRequest* rq, int l = 0);
  bool quant_prologue(const struct Rows& R) const;
  bool oproj_fusable(const struct Rows& R);
  bool wgm_quant_ok(const struct Rows& R);
  bool fc2_split(const struct Rows& R) const;
  int layer_post(int l, hipStream_t st, const struct Rows& R);
  int decode_rows(struct Rows* R, bool scratch_oproj = false);
  int next_tokens(const float* xr, int n, int r0, const int32_t* ctr, hipStream_t st,
                  int32_t* adv_pos = nullptr, int32_t* adv_ctx = nullptr);
  int enqueue_step(hipStream_t st);
  int run_step(const int32_t* tokens_host, float* logits_dev, int32_t* next_host, hipStream_t st);

  // chunked prefill (llm_decoder_prefill): buffers for one chunk of tokens
  static constexpr int kPrefillChunk = 512;
  DevBuf<float> px, pq, po, ph1, psa;
  DevBuf<uint8_t> pact, pws;
  DevBuf<int32_t> pmeta;  // [4][chunk]: pos, ctx, page-table row, token; then the
                          // packed passes' tile table [<= chunk][4]
  size_t pws_bytes = 0;
  int pf_cap = 0;
  int prefill_reserve(int C);
  struct PassSeg;
  int prefill_pass(const std::vector<PassSeg>& segs, bool packed, hipStream_t st);
  int prefill_run(const int32_t* rows, const int32_t* toks, const int32_t* lens, int nrows,
                  long long total, bool packed, hipStream_t st);
  int prefill(int row, const int32_t* toks, int n, hipStream_t st);
  // llm_decoder_set_packed_prefill: generate / beam_search prefill all their
  // rows through prefill_rows
  bool packed_prefill = false;
  int prefill_rows(const int32_t* rows, const int32_t* toks, const int32_t* lens, int nrows,
                   hipStream_t st);
  int prefill_prompts(const int32_t* prompts, const int32_t* prompt_lens, int prompt_stride, int n,
                      int row_step);

  // Continuous batching (llm_decoder_serve_*).  `plan` (serve_plan.hpp) owns
  // the policy -- who is admitted, which row a request holds, which row moves
  // at a retirement -- and the functions below execute its decisions: the
  // active rows are plan's live rows, batch == plan.live() between calls.
  // Every row's token is chosen by one launch_sample_each over the rows'
  // settings in sv_* (device [max_batch], written from the requests when the
  // rows changed: serve_dirty), so the step graph holds no request's setting.
  struct ServeRequest {
    std::vector<int32_t> prompt;
    llm_request_options opt;
    int32_t feed;  // the token its next step takes: prompt's last, then the chosen id
  };
  bool serving = false;
  ServePlan plan;
  std::unordered_map<long long, ServeRequest> requests;  // waiting and live, by id
  DevBuf<float> sv_temp, sv_topp;
  DevBuf<int32_t> sv_topk;
  DevBuf<uint64_t> sv_seed;
  std::vector<float> hs_temp, hs_topp;  // the uploads' staging (a step ends synchronised)
  std::vector<int32_t> hs_topk, hs_pos, hs_ctx, hs_tok, hs_next;
  std::vector<uint64_t> hs_seed;
  bool serve_dirty = false;
  long long graph_instantiations = 0;  // by serving steps (llm_decoder_serve_stats)
  int serve_upload();
  int serve_release(int row, long long id, const ServeMove* mv);
  int serve_step(float* logits_dev, llm_serve_event* events, int* n_events);
};

#define NOT_SERVING(d, who) \
  LLM_REQUIRE(!(d)->serving, who ": the decoder is serving (llm_decoder_serve_end first)")

static int check_cfg(const llm_decoder_config& c) {
  LLM_REQUIRE(c.num_layers > 0 && c.num_heads > 0 && c.head_dim > 0 && c.vocab_size > 0 &&
                  c.max_seq_len > 0,
              "decoder: num_layers/num_heads/head_dim/vocab_size/max_seq_len must be positive");
  LLM_REQUIRE(c.hidden_dim == c.num_heads * c.head_dim,
              "decoder: hidden_dim must equal num_heads * head_dim");
  LLM_REQUIRE(c.weight_dtype == LLM_I8 || c.weight_dtype == LLM_F16, "decoder: weight_dtype");
  return LLM_OK;
}

static int create_decoder(const llm_decoder_config* cfg_in, int kv_dtype, llm_decoder** out) {
  LLM_REQUIRE(cfg_in && out, "llm_decoder_create: NULL");
  LLM_REQUIRE(kv_elem_size(kv_dtype) > 0, "llm_decoder_create_kv: unknown kv_dtype");
  if (kv_dtype != LLM_F16 && kv_dtype != LLM_FP8)
    return fail(LLM_ERR_UNSUPPORTED, "llm_decoder_create_kv: the decoder's KV pools are LLM_F16 "
                                     "or LLM_FP8");
  llm_decoder_config c = *cfg_in;
  if (c.inter_dim <= 0) c.inter_dim = 4 * c.hidden_dim;
  if (c.page_size <= 0) c.page_size = 16;
  if (c.max_batch <= 0) c.max_batch = 1;
  if (c.attn_scale == 0.f) c.attn_scale = 1.f;
  RET_IF(check_cfg(c));
  LLM_REQUIRE(c.hidden_dim % 64 == 0 && c.inter_dim % 64 == 0 && c.inter_dim <= 16384,
              "decoder: hidden_dim and inter_dim must be multiples of 64 (packed GEMM "
              "activations), inter_dim <= 16384");
  std::unique_ptr<llm_decoder> d(new llm_decoder());
  d->cfg = c;
  d->L = c.num_layers; d->H = c.num_heads; d->D = c.head_dim; d->hid = c.hidden_dim;
  d->inter = c.inter_dim; d->V = c.vocab_size; d->TS = c.page_size;
  d->max_tiles = (c.max_seq_len + c.page_size - 1) / c.page_size;
  d->maxB = c.max_batch;
  d->wdtype = c.weight_dtype;
  LLM_HIP_RET(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
  long long pages = c.num_pages > 0 ? c.num_pages
                                     : (long long)d->maxB * d->L * d->H * d->max_tiles;
  d->kvt = kv_dtype;
  d->k_scale.assign(d->L, 1.f);
  d->v_scale.assign(d->L, 1.f);
  RET_IF(kv_cache_create_typed(d->L, d->maxB, d->H, d->D, d->TS, d->max_tiles, pages, kv_dtype,
                               &d->kv));
  const int B = d->maxB, hid = d->hid, inter = d->inter;
  RET_IF(d->x.alloc((size_t)B * hid));
  RET_IF(d->qkv.alloc((size_t)B * 3 * hid));
  RET_IF(d->o.alloc((size_t)B * hid));
  RET_IF(d->h1.alloc((size_t)B * inter));
  RET_IF(d->logits.alloc((size_t)B * d->V));
  d->lm_nwg = lm_head_workgroups(d->V);
  RET_IF(d->lm_pv.alloc((size_t)B * d->lm_nwg));
  RET_IF(d->lm_pi.alloc((size_t)B * d->lm_nwg));
  RET_IF(d->sa.alloc((size_t)B));
  const size_t B16 = ((size_t)B + 15) / 16 * 16;  // packed-A tiles are 16 rows
  RET_IF(d->qa.alloc(B16 * std::max(hid, inter)));
  if (d->wdtype == LLM_F16) {
    RET_IF(d->a16.alloc(2 * B16 * std::max(hid, inter)));  // act, act2
    RET_IF(d->oacc.alloc((size_t)B * hid));
    LLM_HIP_RET(hipMemset(d->oacc.p, 0, sizeof(long long) * B * hid));
    RET_IF(d->oflag.alloc(2));  // [0] the flag, [1] take_flag_kernel's result
    LLM_HIP_RET(hipMemset(d->oflag.p, 0, 2 * sizeof(int)));
    LLM_HIP_RET(hipHostMalloc(reinterpret_cast<void**>(&d->h_oflag), sizeof(int)));
    *d->h_oflag = 0;
  }
  RET_IF(d->beam_ctr.alloc(2 * (((size_t)B + 3) / 4) * d->H));
  LLM_HIP_RET(hipMemset(d->beam_ctr.p, 0, sizeof(unsigned) * d->beam_ctr.n));
  d->b16 = B16;
  RET_IF(d->tokens.alloc((size_t)B));
  RET_IF(d->beam_score.alloc((size_t)B));
  RET_IF(d->beam_ws.alloc(beam_select_ws_floats(B, 4)));  // (>= any num_seqs * W <= B)
  RET_IF(d->cand_score.alloc((size_t)2 * B));
  RET_IF(d->cand_parent.alloc((size_t)2 * B));
  RET_IF(d->cand_token.alloc((size_t)2 * B));
  RET_IF(d->pos.alloc((size_t)B));
  RET_IF(d->ctx.alloc((size_t)B));
  d->pps = 0;  // balanced splits derived on device from each row's context
  d->attn_ws_bytes = 16;
  for (int b = 1; b <= B; ++b)  // any batch size up to max_batch
    d->attn_ws_bytes = std::max(d->attn_ws_bytes,
                                pa_decode_workspace_bytes(b, d->H, d->D, d->max_tiles, 0));
  RET_IF(d->attn_ws.alloc(std::max<size_t>(d->attn_ws_bytes, 16)));
  d->qa_ld = std::max(hid, inter);
  // Splitting the rows into two micro-batches on two streams was measured and
  // removed: one graph with two branches, two graphs on two
  // streams, ping-pong attention and a CU partition all lose (C2 -11..-13 %,
  // C4 -5 %, C3 -0.5..+1 %: the branches do not overlap usefully, and a
  // saturating KV scan slows the other half's glue 4-8x).
  d->use_graph = env_int("LLM_GRAPH", 1) != 0;
  d->h_pos.assign(B, 0);
  *out = d.release();
  return LLM_OK;
}

extern "C" int llm_decoder_create(const llm_decoder_config* cfg, llm_decoder** out) {
  return create_decoder(cfg, LLM_F16, out);
}

extern "C" int llm_decoder_create_kv(const llm_decoder_config* cfg, int kv_dtype,
                                     llm_decoder** out) {
  return create_decoder(cfg, kv_dtype, out);
}

extern "C" int llm_decoder_kv_dtype(const llm_decoder* d) { return d ? d->kvt : -1; }

extern "C" int llm_decoder_prefill_kernel(const llm_decoder* d) {
  if (!d) return -1;
  pa_kv_view view;  // layer_attn's own test, on the same view
  if (kv_cache_view(d->kv, 0, &view) != LLM_OK) return -1;
  return pa_prefill_supported(&view) ? LLM_PREFILL_MFMA : LLM_PREFILL_DECODE;
}

extern "C" int llm_decoder_set_kv_scales(llm_decoder* d, const float* k_scale,
                                         const float* v_scale) {
  LLM_REQUIRE(d, "llm_decoder_set_kv_scales: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  NOT_SERVING(d, "llm_decoder_set_kv_scales");
  LLM_REQUIRE(d->kvt == LLM_FP8, "llm_decoder_set_kv_scales: the decoder's KV pools are not LLM_FP8");
  LLM_REQUIRE(d->batch == 0, "llm_decoder_set_kv_scales: rows are active (set the scales before "
                             "begin_* / generate / prefill)");
  for (const float* s : {k_scale, v_scale})
    for (int l = 0; s && l < d->L; ++l)
      LLM_REQUIRE(std::isfinite(s[l]) && s[l] > 0.f,
                  "llm_decoder_set_kv_scales: every scale must be finite and > 0");
  for (int l = 0; l < d->L; ++l) {
    d->k_scale[l] = k_scale ? k_scale[l] : 1.f;
    d->v_scale[l] = v_scale ? v_scale[l] : 1.f;
  }
  d->graph_batch = -1;  // the step graph carries the scales as kernel arguments
  return LLM_OK;
}

// attention/attention_kernel_utils.cuh:20-35 (the rotation), see rope_rows
extern "C" int llm_decoder_set_rope(llm_decoder* d, const float* table) {
  LLM_REQUIRE(d, "llm_decoder_set_rope: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  NOT_SERVING(d, "llm_decoder_set_rope");
  LLM_REQUIRE(d->batch == 0, "llm_decoder_set_rope: rows are active (set the table before "
                             "begin_* / generate / prefill)");
  if (table) {
    LLM_REQUIRE(d->D % 2 == 0, "llm_decoder_set_rope: head_dim must be even");
    const size_t n = (size_t)d->cfg.max_seq_len * d->D;
    for (size_t i = 0; i < n; ++i)
      LLM_REQUIRE(std::isfinite(table[i]), "llm_decoder_set_rope: every entry must be finite");
    LLM_HIP_RET(hipStreamSynchronize(d->stream));  // nothing in flight reads the old table
    if (!d->rope.p) RET_IF(d->rope.alloc(n));
    LLM_HIP_RET(hipMemcpy(d->rope.p, table, n * sizeof(float), hipMemcpyHostToDevice));
  }
  d->rope_on = table != nullptr;
  d->graph_batch = -1;  // the step graph carries the table as a kernel argument
  return LLM_OK;
}

extern "C" int llm_decoder_rope(const llm_decoder* d) { return d ? (d->rope_on ? 1 : 0) : -1; }

extern "C" int llm_decoder_set_window(llm_decoder* d, int window) {
  LLM_REQUIRE(d, "llm_decoder_set_window: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  NOT_SERVING(d, "llm_decoder_set_window");
  LLM_REQUIRE(d->batch == 0, "llm_decoder_set_window: rows are active (set the window before "
                             "begin_* / generate / prefill)");
  LLM_REQUIRE(window >= 0, "llm_decoder_set_window: window must be >= 0 (0: off)");
  d->window = window;
  d->graph_batch = -1;  // the step graph carries the window as a kernel argument
  return LLM_OK;
}

extern "C" int llm_decoder_window(const llm_decoder* d) { return d ? d->window : -1; }

extern "C" void llm_decoder_destroy(llm_decoder* d) {
  if (!d) return;
  if (d->stream) (void)hipStreamSynchronize(d->stream);
  delete d;
}

extern "C" kv_cache* llm_decoder_kv(llm_decoder* d) { return d ? d->kv : nullptr; }

// ---------------------------------------------------------------------------
// weights
// ---------------------------------------------------------------------------
template <typename T>
static int upload(DevBuf<T>& dst, const T* src, size_t n, const char* what) {
  LLM_REQUIRE(src != nullptr, std::string("decoder weights: ") + what + " is NULL");
  RET_IF(dst.alloc(n));
  LLM_HIP_RET(hipMemcpy(dst.p, src, n * sizeof(T), hipMemcpyHostToDevice));
  return LLM_OK;
}

// Upload L row-major [K][N] matrices and pack each into MFMA fragment order.
static int upload_packed(DevBuf<uint8_t>& dst, size_t& per_layer, const void* src, int L, int K,
                         int N, int dtype, const char* what) {
  LLM_REQUIRE(src != nullptr, std::string("decoder weights: ") + what + " is NULL");
  const size_t esz = dtype == LLM_I8 ? 1 : 2;
  per_layer = gemm_packed_bytes(dtype, K, N);
  RET_IF(dst.alloc(per_layer * L));
  void* tmp = nullptr;
  LLM_HIP_RET(hipMalloc(&tmp, (size_t)K * N * esz));
  int rc = LLM_OK;
  for (int l = 0; l < L && rc == LLM_OK; ++l) {
    const char* s = static_cast<const char*>(src) + (size_t)l * K * N * esz;
    if (hipMemcpy(tmp, s, (size_t)K * N * esz, hipMemcpyHostToDevice) != hipSuccess) {
      rc = fail(LLM_ERR_HIP, "decoder weights: upload failed");
      break;
    }
    rc = gemm_pack_weights(dtype, tmp, dst.p + per_layer * l, K, N, nullptr);
  }
  (void)hipDeviceSynchronize();
  (void)hipFree(tmp);
  return rc;
}

static int upload_common(llm_decoder* d, const uint16_t* emb, const float* ln1_g,
                         const float* ln1_b, const float* ln2_g, const float* ln2_b) {
  const size_t Lh = (size_t)d->L * d->hid;
  RET_IF(upload(d->emb, emb, (size_t)d->V * d->hid, "emb"));
  RET_IF(d->emb_packed.alloc(lm_head_packed_bytes(d->V, d->hid)));
  LLM_HIP_RET(launch_lm_pack(d->emb.p, d->emb_packed.p, d->V, d->hid, nullptr));
  LLM_HIP_RET(hipDeviceSynchronize());
  RET_IF(upload(d->ln1_g, ln1_g, Lh, "ln1_g"));
  RET_IF(upload(d->ln1_b, ln1_b, Lh, "ln1_b"));
  RET_IF(upload(d->ln2_g, ln2_g, Lh, "ln2_g"));
  RET_IF(upload(d->ln2_b, ln2_b, Lh, "ln2_b"));
  return LLM_OK;
}

// The weight GEMMs load with the default cache policy (lines stay in the
// 256 MiB Infinity Cache, so the next step's GEMMs hit there) when the whole
// weight set fits well inside it; the KV stream is loaded non-temporal and
// does not displace them.  Larger models stream their weights nt (read once
// per step: keeping them would only churn the cache).  Same-box A/B, two
// runs each (profiles/r03/wkeep_ab.txt): C2 (170 MB of weights) +1.7 / +2.1 %
// kept; C4 (1.2 GB) -2.3 / -2.6 % kept, so nt there.
static int w_keep_for(const llm_decoder* d) {
  const size_t bytes = (d->sz_qkv + d->sz_o + d->sz_1 + d->sz_2) * (size_t)d->L;
  return bytes <= (size_t)192 << 20;
}

extern "C" int llm_decoder_set_int8_weights(llm_decoder* d, const llm_int8_weights* w) {
  LLM_REQUIRE(d && w, "llm_decoder_set_int8_weights: NULL");
  LLM_REQUIRE(d->wdtype == LLM_I8, "llm_decoder_set_int8_weights: decoder is not INT8");
  std::lock_guard<std::mutex> g(d->mu);
  LLM_HIP_RET(hipStreamSynchronize(d->stream));
  const int L = d->L, hid = d->hid, inter = d->inter;
  RET_IF(upload_common(d, w->emb, w->ln1_g, w->ln1_b, w->ln2_g, w->ln2_b));
  RET_IF(upload_packed(d->wqkv, d->sz_qkv, w->wqkv, L, hid, 3 * hid, LLM_I8, "wqkv"));
  RET_IF(upload_packed(d->wo, d->sz_o, w->wo, L, hid, hid, LLM_I8, "wo"));
  RET_IF(upload_packed(d->w1, d->sz_1, w->w1, L, hid, inter, LLM_I8, "w1"));
  RET_IF(upload_packed(d->w2, d->sz_2, w->w2, L, inter, hid, LLM_I8, "w2"));
  RET_IF(upload(d->sw_qkv, w->sw_qkv, (size_t)L * 3 * hid, "sw_qkv"));
  RET_IF(upload(d->sw_o, w->sw_o, (size_t)L * hid, "sw_o"));
  RET_IF(upload(d->sw1, w->sw1, (size_t)L * inter, "sw1"));
  RET_IF(upload(d->sw2, w->sw2, (size_t)L * hid, "sw2"));
  RET_IF(upload(d->b1, w->b1, (size_t)L * inter, "b1"));
  RET_IF(upload(d->b2, w->b2, (size_t)L * hid, "b2"));
  d->w_keep = w_keep_for(d);
  d->graph_batch = -1;
  d->weights_ready = true;
  return LLM_OK;
}

extern "C" int llm_decoder_set_f16_weights(llm_decoder* d, const llm_f16_weights* w) {
  LLM_REQUIRE(d && w, "llm_decoder_set_f16_weights: NULL");
  LLM_REQUIRE(d->wdtype == LLM_F16, "llm_decoder_set_f16_weights: decoder is not FP16");
  std::lock_guard<std::mutex> g(d->mu);
  LLM_HIP_RET(hipStreamSynchronize(d->stream));
  const int L = d->L, hid = d->hid, inter = d->inter;
  RET_IF(upload_common(d, w->emb, w->ln1_g, w->ln1_b, w->ln2_g, w->ln2_b));
  RET_IF(upload_packed(d->wqkv, d->sz_qkv, w->wqkv, L, hid, 3 * hid, LLM_F16, "wqkv"));
  RET_IF(upload_packed(d->wo, d->sz_o, w->wo, L, hid, hid, LLM_F16, "wo"));
  // the fused o_proj's head slices: [h][kg][n][j] = W_o[h D + 8 kg + j][n] (a
  // second copy of W_o, L * hid^2 fp16), only where the fused o_proj can run
  // (oproj_fusable); the step then reads these instead of the packed W_o, so
  // the bytes a step streams (w_keep_for) are unchanged
  d->wo_heads.alloc(0);
  if (d->D % 8 == 0 && d->D <= 128 && d->H <= 64 && oproj_fuse_on()) {
    const int D = d->D, KG = D / 8;
    const uint16_t* src = static_cast<const uint16_t*>(w->wo);
    std::vector<uint16_t> sl((size_t)hid * hid);
    RET_IF(d->wo_heads.alloc((size_t)L * hid * hid));
    for (int l = 0; l < L; ++l) {
      const uint16_t* wl = src + (size_t)l * hid * hid;
      for (int h = 0; h < d->H; ++h)
        for (int kg = 0; kg < KG; ++kg)
          for (int n = 0; n < hid; ++n)
            for (int j = 0; j < 8; ++j)
              sl[(((size_t)h * KG + kg) * hid + n) * 8 + j] = wl[(size_t)(h * D + 8 * kg + j) * hid + n];
      LLM_HIP_RET(hipMemcpy(d->wo_heads.p + (size_t)l * hid * hid, sl.data(),
                            sizeof(uint16_t) * hid * hid, hipMemcpyHostToDevice));
    }
  }
  RET_IF(upload_packed(d->w1, d->sz_1, w->w1, L, hid, inter, LLM_F16, "w1"));
  RET_IF(upload_packed(d->w2, d->sz_2, w->w2, L, inter, hid, LLM_F16, "w2"));
  RET_IF(upload(d->b1, w->b1, (size_t)L * inter, "b1"));
  RET_IF(upload(d->b2, w->b2, (size_t)L * hid, "b2"));
  d->w_keep = w_keep_for(d);
  d->graph_batch = -1;
  d->weights_ready = true;
  return LLM_OK;
}

// ---------------------------------------------------------------------------
// step
// ---------------------------------------------------------------------------
// The rows one layer pass works on: the decode rows (the active batch in the
// step buffers, one token each; decode_rows) or a prefill pass (n prompt
// tokens, beam_rows[m] = the page-table row of token m; prefill_pass).  Every
// buffer is row-indexed.
struct Rows {
  int n = 0;
  float* x = nullptr;   // [n][hid] residual-free hidden state
  float* q = nullptr;   // [n][hid] q of the fused qkv projection
  float* o = nullptr;   // [n][hid] attention output (fp32)
  float* h1 = nullptr;  // [n][inter]
  void* act = nullptr;  // packed-A GEMM input (int8 or fp16), 16-row tiles
  void* act2 = nullptr; // fp16 decoder: fc2's packed input (written by fc1 while act is read)
  float* sa = nullptr;  // [n] int8 row scales
  const int32_t* pos = nullptr;  // [n] position written this pass
  const int32_t* ctx = nullptr;  // [n] context length attended (pos + 1)
  const int32_t* beam_rows = nullptr;  // page-table row per row; NULL: row m
  int row_group = 1;
  // INT8 rows too wide for the o_proj quantising prologue (wgm_quant_ok): the
  // attention writes fp32 rows merged in the workgroup and a quantise launch
  // follows it
  bool wgm_quant = false;
  // prefill chunk (row >= 0): the n rows are positions p0 .. p0+n-1 of page-table
  // row prefill_row, attended causally by the MFMA prefill kernel
  int prefill_row = -1;
  int prefill_p0 = 0;
  // packed prefill pass (prefill_ntile > 0): the n rows are segments of several
  // page-table rows (pos / ctx / beam_rows say which, per row), attended by one
  // pa_prefill_packed launch over the device tile table prefill_tiles (ctx is
  // its context_lens; attn_ws takes the split partials)
  const int32_t* prefill_tiles = nullptr;
  int prefill_ntile = 0;
  int prefill_maxend = 0;  // the longest segment's end
  // a prefill pass of either kind: no LN prologue fusion, no quantising
  // prologue, no fused o_proj, no fc2 split, no taps
  bool is_prefill() const { return prefill_row >= 0 || prefill_ntile > 0; }
  uint8_t* attn_ws = nullptr;
  size_t attn_ws_bytes = 0;
  // FP16 decode rows: the o_proj runs inside the attention's workgroup merge
  // (oproj_fusable) through these int64 columns and writes oproj_out (x, or a
  // scratch row for llm_decoder_run_attention); no o_proj launch
  long long* oacc = nullptr;
  float* oproj_out = nullptr;
  int* oflag = nullptr;  // the range guard's flag for these columns
};

// Activations feeding a weight GEMM (qa int8 / a16 fp16) are kept in packed-A
// order (common.hpp a_frag_off_*): their producers (LayerNorm+quant, the
// attention merge, the row quantiser) write MFMA A-fragments directly, so
// every GEMM A load is one coalesced 1 KiB read.
// emb (optional): the first LayerNorm reads embedding rows, not R.x (the
// decode step's layer 0; prefill rows come from launch_embed).
int llm_decoder::layer_pre(int l, hipStream_t st, const Rows& R, const LnSource* emb) {
  const size_t lh = (size_t)l * hid;
  pa_kv_view view;
  RET_IF(kv_cache_view(kv, l, &view));
  KvAppendView app;
  app.pos = R.pos;
  app.page_table = view.page_table;
  app.rows = R.beam_rows;
  app.k_pool = kv_cache_k_pool(kv);
  app.v_pool = kv_cache_v_pool(kv);
  app.num_beams = view.num_beams;
  app.max_tiles = view.max_tiles;
  app.page_size = TS;
  app.num_pages = view.num_pages;
  app.H = H;
  app.D = D;
  app.page_stride = (size_t)view.page_stride / kv_elem_size(kvt);
  app.kv_dtype = kvt;
  app.k_inv_scale = 1.0f / k_scale[l];
  app.v_inv_scale = 1.0f / v_scale[l];
  if (rope_on) {  // decode rows, prompt chunks and packed passes alike: R.pos is per row
    app.rope = rope.p;
    app.rope_len = cfg.max_seq_len;
  }
  WeightGemm g;
  g.dtype = wdtype;
  g.a_packed = 1;
  g.w_keep = w_keep;
  g.A = R.act;
  g.W_packed = wqkv.p + sz_qkv * l;
  g.M = R.n; g.N = 3 * hid; g.K = hid;
  g.C = R.q; g.c_cols = hid; g.c_ld = hid;  // q only: K and V go straight into the pages
  g.kv = &app;
  if (wdtype == LLM_I8) g.sa = R.sa, g.sw = sw_qkv.p + (size_t)l * 3 * hid;
  RET_IF(layer_norm_into(g, R, ln1_g.p + lh, ln1_b.p + lh, st, nullptr, emb));
  RET_IF(weight_gemm(g, st));
  return tap(l, 0, R, hid, st);
}

// LN(x) as the GEMM's A: fused into the GEMM as its LayerNorm prologue when
// the rows' A image fits in LDS (decode rows), else a LayerNorm (+ quant)
// launch writing the packed A the GEMM reads.  emb (optional): the rows are
// the token embedding rows it names, not R.x; there is no embed launch in a
// decode step (enqueue_step).
int llm_decoder::layer_norm_into(WeightGemm& g, const Rows& R, const float* gamma,
                                 const float* beta, hipStream_t st, float* zero_x,
                                 const LnSource* emb) {
  LnSource src = emb ? *emb : LnSource{};
  src.zero_x = zero_x;  // (the LayerNorm launch only: the caller checks fc2_split)
  if (!R.is_prefill() && ln_fusable(wdtype, R.n, hid)) {
    g.ln_x = R.x; g.ln_g = gamma; g.ln_b = beta; g.ln_eps = 1e-5f;
    g.ln_emb = src.emb; g.ln_tok = src.tok; g.ln_V = src.V;
    if (tap_q) { g.act_out = R.act; g.sa_out = R.sa; }  // the taps read A and the scales back
    return LLM_OK;
  }
  const LnSource* pp = src.emb || src.zero_x ? &src : nullptr;
  if (wdtype == LLM_I8)
    LLM_HIP_RET(launch_layernorm_quant(R.x, R.n, hid, gamma, beta, 1e-5f, nullptr,
                                       static_cast<int8_t*>(R.act), R.sa, st, 1, pp));
  else
    LLM_HIP_RET(launch_layernorm_f16(R.x, R.n, hid, gamma, beta, 1e-5f, R.act, st, 1, pp));
  return LLM_OK;
}

// INT8 decode rows whose o_proj can quantise its own input (gemm.hip
// quant_prologue_ok): the attention writes fp32 rows, merging its splits in
// the workgroup, and the o_proj prologue quantises them per row -- no merge
// launch.  Beam groups keep the merge launch (the beam kernel's workgroups
// are 4 beams of one split), as do prefill chunks.
bool llm_decoder::quant_prologue(const Rows& R) const {
  return wdtype == LLM_I8 && !R.is_prefill() && R.row_group == 1 &&
         quant_prologue_ok(R.n, hid, hid);
}

// FP16 decode rows whose o_proj the attention's workgroup merge can run
// (pa_decode.hip, OPROJ): each (row, head) workgroup multiplies its merged
// head by W_o's rows for that head and adds the products into the int64
// columns R.oacc; the adder completing a column writes x (what the o_proj
// GEMM wrote).  One launch per layer fewer (C2: the 4.9 us o_proj GEMM).
// Needs the workgroup-merge form (2..8 splits), head_dim <= 128 and <= 64
// heads; otherwise the o_proj GEMM runs as before.
bool llm_decoder::oproj_fusable(const Rows& R) {
  if (wdtype != LLM_F16 || kvt != LLM_F16 || R.is_prefill() || R.row_group != 1 ||
      R.beam_rows || !wo_heads.p ||
      D > 128 || H > 64 || !oproj_fuse_on())
    return false;
  Rows r = R;
  r.oacc = oacc.p;
  pa_kv_view view;
  PaRequest rq;
  PaLaunch p;
  return attn_request(r, &view, &rq) == LLM_OK && pa_plan_device(rq, &p) == LLM_OK && p.oproj;
}

// INT8 decode rows whose o_proj cannot quantise its own input (hidden >
// 2048: C5's 4096, 256 KB of fp32 rows per 16-row workgroup): when the plan
// with fp32 rows is the workgroup merge (<= 8 splits), the attention merges
// its splits in the workgroup and one quantise launch writes the packed int8
// o_proj input -- in place of split + pa_merge_row_kernel (C5: 5 splits of
// 103 pages -> 8 of 65 merged in the workgroup).
bool llm_decoder::wgm_quant_ok(const Rows& R) {
  if (wdtype != LLM_I8 || R.is_prefill() || R.row_group != 1 || R.beam_rows ||
      quant_prologue(R))
    return false;
  Rows r = R;
  r.wgm_quant = true;
  pa_kv_view view;
  PaRequest rq;
  PaLaunch p;
  return attn_request(r, &view, &rq) == LLM_OK && pa_plan_device(rq, &p) == LLM_OK && p.wgm;
}

// INT8 decode rows <= 16 (the 4- and 8-GPU points of C3's strong curve): fc2's
// 128 column tiles leave half the CUs idle, so it runs as two k slices that
// each add their dequantised half into x (fp32 atomics; two addends commute,
// so x is the same bits whichever lands first).  x must be zero when fc2
// starts: the LN2 launch, the last reader of the o_proj output in x, writes
// zeros over the rows after loading them.  Standalone (scripts/tune_gemm_sk.py,
// profiles/r05/gemm_small_m.txt): fc2 at M = 8 6.86 -> 5.67 us, M = 16 7.53 ->
// 5.95 us.
// Round 6: also at 33..64 rows when inter >= 16384 (C5's fc2, K 16384): every
// workgroup of the one-slice form reads all of A, 1 MB, the k slices half of
// it (gemm_impl.hpp narrow_decode_tile).
bool llm_decoder::fc2_split(const Rows& R) const {
  return wdtype == LLM_I8 && !R.is_prefill() &&
         (R.n <= 16 || (R.n > 32 && R.n <= 64 && inter >= 16384)) &&
         !ln_fusable(wdtype, R.n, hid) && inter / 64 >= 16;
}

// The decode attention launch of R's rows over layer l's pages: the view of
// the rows' page-table rows and what the launch is to return (pa_plan.hpp).
int llm_decoder::attn_request(const Rows& R, pa_kv_view* view, PaRequest* rq, int l) {
  RET_IF(kv_cache_view(kv, l, view));
  // the split merge also produces the o_proj input (packed int8 + scale, or fp16)
  const PaOut out = quant_prologue(R) || R.wgm_quant ? PaOut::F32_ROWS  // quantised by the o_proj
                    : wdtype == LLM_I8               ? PaOut::ROW_Q     // prologue or layer_attn
                    : R.oacc                         ? PaOut::OPROJ
                                                     : PaOut::ROW_F16;
  *rq = pa_request(view, R.n, H, D, cfg.max_seq_len, pps, R.row_group, out);
  rq->rows16 = out == PaOut::OPROJ && tap_q;  // the taps read the packed o_proj input
  rq->steal_ctr = R.row_group >= 4 && beam_steal_on();
  rq->window = window;
  return LLM_OK;
}

int llm_decoder::layer_attn(int l, hipStream_t st, const Rows& R) {
  pa_kv_view view;
  PaRequest rq;
  RET_IF(attn_request(R, &view, &rq, l));
  // the request's pointers: the o_proj input (packed) that the launch writes
  // besides, or in place of, the fp32 rows (R.o: only needed by a single-split
  // direct launch, and the output of F32_ROWS).  A prefill pass asks for
  // ROW_Q or ROW_F16 (attn_request: none of the fused decode forms).
  PaRowOutputs ro;
  ro.pack = 1;
  ro.keep_out = 0;
  if (rq.out == PaOut::ROW_Q) {
    ro.q = static_cast<int8_t*>(R.act);
    ro.inv_scale = R.sa;
  } else if (rq.out == PaOut::OPROJ) {
    ro.o_acc = R.oacc;
    ro.o_x = R.oproj_out;
    ro.wo_heads = wo_heads.p + (size_t)l * hid * hid;
    ro.o_n = hid;
    ro.o_flag = R.oflag;
    ro.out16 = rq.rows16 ? R.act : nullptr;
  } else if (rq.out == PaOut::ROW_F16) {
    ro.out16 = R.act;
  }
  if (rq.steal_ctr) ro.beam_ctr = beam_ctr.p;
  // LLM_FP8 pages: K's scale folded into the score multiplier, V's applied to
  // the normalised heads by the launch (1 and 1 for fp16 pages)
  ro.out_scale = v_scale[l];
  const float sm = kvt == LLM_FP8 ? cfg.attn_scale * k_scale[l] : cfg.attn_scale;
  if (R.is_prefill() && pa_prefill_supported(&view)) {
    // one MFMA pass over the chunk (K/V pages read once per 32 queries), then
    // the o_proj input conversion the decode merge would have fused
    if (R.prefill_ntile > 0)
      return pa_prefill_packed_internal(&view, R.q, hid, R.o, hid, R.prefill_tiles,
                                        R.prefill_ntile, R.ctx, R.n, R.prefill_maxend, sm,
                                        R.attn_ws, R.attn_ws_bytes, st, &ro, window);
    return pa_prefill_internal(&view, R.q, hid, R.o, hid, R.prefill_row, R.prefill_p0, R.n, sm,
                               R.attn_ws, R.attn_ws_bytes, st, &ro, window);
  }
  RET_IF(pa_decode_internal(&view, rq, R.q, hid, R.o, R.beam_rows, R.ctx, sm, R.attn_ws,
                            R.attn_ws_bytes, st, &ro));
  if (R.wgm_quant)  // the packed int8 o_proj input + row scales
    LLM_HIP_RET(launch_quantize_rows(R.o, R.n, hid, static_cast<int8_t*>(R.act), R.sa, st, 1));
  return LLM_OK;
}

int llm_decoder::layer_post(int l, hipStream_t st, const Rows& R) {
  const size_t lh = (size_t)l * hid;
  const bool i8 = wdtype == LLM_I8;
  WeightGemm g;
  g.dtype = wdtype;
  g.a_packed = 1;
  g.w_keep = w_keep;
  g.A = R.act;
  g.M = R.n;
  // o_proj: input produced (packed) by the attention merge, or quantised from
  // the attention's fp32 rows by the GEMM's own prologue
  g.W_packed = wo.p + sz_o * l; g.N = hid; g.K = hid; g.C = R.x;
  if (i8) { g.sa = R.sa; g.sw = sw_o.p + lh; }
  const bool qpro = quant_prologue(R);
  if (qpro) {
    g.ln_x = R.o;
    g.ln_quant_only = 1;
    if (tap_q) { g.act_out = R.act; g.sa_out = R.sa; }  // the taps read A and the scales back
  }
  if (!R.oacc) RET_IF(weight_gemm(g, st));  // (fused: the attention wrote x)
  g.ln_x = nullptr; g.ln_quant_only = 0; g.act_out = nullptr; g.sa_out = nullptr;
  RET_IF(tap(l, 1, R, hid, st));
  // LN2 -> mlp_fc1 (+b1, ReLU)
  const bool split_fc2 = fc2_split(R);
  RET_IF(layer_norm_into(g, R, ln2_g.p + lh, ln2_b.p + lh, st, split_fc2 ? R.x : nullptr));
  g.W_packed = w1.p + sz_1 * l; g.N = inter; g.K = hid;
  g.bias = b1.p + (size_t)l * inter; g.act = LLM_ACT_RELU;
  if (i8) {
    g.C = R.h1;
    g.sw = sw1.p + (size_t)l * inter;
  } else {
    // fp16 decoder: the fc1 epilogue writes fc2's packed fp16 input directly
    // (no per-row scale to wait for, so no conversion launch)
    g.C = nullptr;
    g.C16 = R.act2;
  }
  RET_IF(weight_gemm(g, st));
  RET_IF(tap(l, 2, R, hid, st));
  g.ln_x = nullptr; g.ln_emb = nullptr; g.act_out = nullptr; g.sa_out = nullptr;
  g.C16 = nullptr;
  if (!i8) g.A = R.act2;
  // quantise h1 -> mlp_fc2 (+b2)
  if (i8)
    LLM_HIP_RET(launch_quantize_rows(R.h1, R.n, inter, static_cast<int8_t*>(R.act), R.sa, st, 1));
  RET_IF(tap(l, 3, R, inter, st));
  g.W_packed = w2.p + sz_2 * l; g.N = hid; g.K = inter; g.C = R.x;
  g.bias = b2.p + lh; g.act = LLM_ACT_NONE;
  if (i8) g.sw = sw2.p + lh;
  g.ksplit2 = split_fc2 ? 1 : 0;  // (x was zeroed by the LN2 launch)
  return weight_gemm(g, st);
}

// The decode rows: the active batch in the step buffers, with the forms of
// its launches decided (the fused o_proj, the workgroup merge + quantise) --
// what the step enqueues, what llm_decoder_attention_plan reports and what
// llm_decoder_run_attention times.
// scratch_oproj (run_attention): the fused o_proj writes the attention rows'
// fp32 buffer, not x, and accumulates into columns of its own (oacc_run:
// allocated on first use, zero, and every completed column clears itself, as
// the step's do) with a range flag of its own (oflag_run: a clamp there never
// fails a step or a sync).
int llm_decoder::decode_rows(Rows* out, bool scratch_oproj) {
  Rows& R = *out = Rows{};
  R.n = batch;
  R.x = x.p; R.q = qkv.p; R.o = o.p; R.h1 = h1.p;
  R.act = wdtype == LLM_I8 ? (void*)qa.p : (void*)a16.p;
  if (wdtype == LLM_F16) R.act2 = a16.p + b16 * qa_ld;
  R.sa = sa.p;
  R.pos = pos.p;
  R.ctx = ctx.p;
  R.row_group = row_group;
  R.attn_ws = attn_ws.p;
  R.attn_ws_bytes = attn_ws_bytes;
  if (oproj_fusable(R)) {
    if (scratch_oproj && !oacc_run.p) {
      RET_IF(oacc_run.alloc(oacc.n));
      LLM_HIP_RET(hipMemset(oacc_run.p, 0, sizeof(long long) * oacc_run.n));
      RET_IF(oflag_run.alloc(1));
      LLM_HIP_RET(hipMemset(oflag_run.p, 0, sizeof(int)));
    }
    R.oacc = scratch_oproj ? oacc_run.p : oacc.p;
    R.oproj_out = scratch_oproj ? R.o : R.x;
    R.oflag = scratch_oproj ? oflag_run.p : oflag.p;
  }
  R.wgm_quant = wgm_quant_ok(R);
  return LLM_OK;
}

// Tap stage `stage` of layer l (0: LN1 out, 1: attention out, 2: LN2 out,
// 3: fc1 out): the rows' packed int8 activations (K per row) and row scales.
// Decode rows only (prefill chunks are not tapped); captured into the graph.
// FP16 decoders: the four packed fp16 GEMM inputs (2 bytes per element, no
// scales); stage 3 (fc2's input) is act2, written by the fc1 epilogue.
int llm_decoder::tap(int l, int stage, const Rows& R, int K, hipStream_t st) {
  if (!tap_q || R.is_prefill() || R.beam_rows) return LLM_OK;
  const bool f16 = wdtype == LLM_F16;
  const size_t es = f16 ? 2 : 1;
  const size_t slot = (size_t)l * 4 + stage;
  const size_t n16 = ((size_t)R.n + 15) / 16 * 16;
  const void* src = f16 && stage == 3 ? R.act2 : R.act;
  LLM_HIP_RET(hipMemcpyAsync(tap_q + slot * b16 * qa_ld * es, src, n16 * K * es,
                             hipMemcpyDeviceToDevice, st));
  if (!f16)
    LLM_HIP_RET(hipMemcpyAsync(tap_s + slot * maxB, R.sa, sizeof(float) * R.n,
                               hipMemcpyDeviceToDevice, st));
  return LLM_OK;
}

// LM head + token choice for rows r0.. (x rows given): logits into the step's
// logits buffer; greedy ids from the LM head's fused argmax partials, or a
// device draw (sample_rows) with the rows' positions as draw counters.
// adv_pos / adv_ctx (optional): advance the rows' positions afterwards (fused
// into the argmax launch; a launch of its own after a draw, which reads them).
int llm_decoder::next_tokens(const float* xr, int n, int r0, const int32_t* ctr, hipStream_t st,
                             int32_t* adv_pos, int32_t* adv_ctx) {
  float* lg = logits.p + (size_t)r0 * V;
  if (beam_mode && adv_pos) {  // the decode step of a beam search (rows 0 .. batch - 1)
    LLM_HIP_RET(launch_lm_head(xr, emb_packed.p, lg, n, V, hid, nullptr,
                               lm_pi.p + (size_t)r0 * lm_nwg, st));
    LLM_HIP_RET(launch_beam_select(lg, beam_score.p + r0, n / row_group, row_group, V,
                                   cand_score.p + 2 * r0, cand_parent.p + 2 * r0,
                                   cand_token.p + 2 * r0, beam_ws.p, st));
    LLM_HIP_RET(launch_advance(adv_pos, adv_ctx, n, st));
    return LLM_OK;
  }
  if (serving) {  // every row by its request's settings: one launch, greedy rows included
    LLM_HIP_RET(launch_lm_head(xr, emb_packed.p, lg, n, V, hid, nullptr,
                               lm_pi.p + (size_t)r0 * lm_nwg, st));
    LLM_HIP_RET(launch_sample_each(lg, n, V, sv_temp.p + r0, sv_topk.p + r0, sv_topp.p + r0,
                                   sv_seed.p + r0, ctr, tokens.p + r0, st));
    if (adv_pos) LLM_HIP_RET(launch_advance(adv_pos, adv_ctx, n, st));
    return LLM_OK;
  }
  const bool sample = temperature > 0.f && top_k != 1;
  float* pv = lm_pv.p + (size_t)r0 * lm_nwg;
  int32_t* pi = lm_pi.p + (size_t)r0 * lm_nwg;
  LLM_HIP_RET(launch_lm_head(xr, emb_packed.p, lg, n, V, hid, sample ? nullptr : pv, pi, st));
  if (sample) {
    LLM_HIP_RET(launch_sample(lg, n, r0, V, temperature, top_k, top_p, sample_seed, ctr,
                              tokens.p + r0, st));
    if (adv_pos) LLM_HIP_RET(launch_advance(adv_pos, adv_ctx, n, st));
  } else {
    LLM_HIP_RET(launch_argmax_partials(pv, pi, n, lm_nwg, tokens.p + r0, st, adv_pos, adv_ctx));
  }
  return LLM_OK;
}

// One decode step of all active rows (captured into the step graph).  The
// embedding has no launch of its own: layer 0's first LayerNorm (launch or
// GEMM prologue) reads E[token] rows directly.
int llm_decoder::enqueue_step(hipStream_t st) {
  Rows R;
  RET_IF(decode_rows(&R));
  LnSource embed;
  embed.emb = reinterpret_cast<const _Float16*>(emb.p);
  embed.tok = tokens.p;
  embed.V = V;
  for (int l = 0; l < L; ++l) {
    RET_IF(layer_pre(l, st, R, l == 0 ? &embed : nullptr));
    RET_IF(layer_attn(l, st, R));
    RET_IF(layer_post(l, st, R));
  }
  return next_tokens(x.p, batch, 0, pos.p, st, pos.p, ctx.p);
}

int llm_decoder::run_step(const int32_t* tokens_host, float* logits_dev, int32_t* next_host,
                          hipStream_t st) {
  LLM_REQUIRE(weights_ready, "decoder: weights not loaded");
  LLM_REQUIRE(batch > 0, "decoder: no active rows (call generate / begin first)");
  KvCache* k = kv_impl(kv);
  {
    std::lock_guard<std::mutex> g(k->mu);
    for (int b = 0; b < batch; ++b) {
      LLM_REQUIRE(h_pos[b] < cfg.max_seq_len, "decoder: row reached max_seq_len");
      RET_IF(k->prepare_append(b, h_pos[b]));
      // windowed: the step attends to tokens >= h_pos[b] + 1 - window only
      if (window > 0) RET_IF(k->release_before(b, h_pos[b] + 1 - window));
    }
    RET_IF(k->sync(st));
  }
  if (tokens_host) {
    for (int b = 0; b < batch; ++b)
      LLM_REQUIRE(tokens_host[b] >= 0 && tokens_host[b] < V, "decoder: token id out of range");
    LLM_HIP_RET(hipMemcpyAsync(tokens.p, tokens_host, sizeof(int32_t) * batch,
                               hipMemcpyHostToDevice, st));
  }
  if (!use_graph) {
    RET_IF(enqueue_step(st));
  } else {
    if (graph_batch != batch) {
      if (graph) { (void)hipGraphExecDestroy(graph); graph = nullptr; }
      hipGraph_t g;
      LLM_HIP_RET(hipStreamSynchronize(st));
      LLM_HIP_RET(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
      int rc = enqueue_step(stream);
      hipError_t e = hipStreamEndCapture(stream, &g);
      if (rc) return rc;
      if (e != hipSuccess)
        return fail(LLM_ERR_HIP, std::string("graph capture: ") + hipGetErrorString(e));
      e = hipGraphInstantiate(&graph, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      if (e != hipSuccess)
        return fail(LLM_ERR_HIP, std::string("graph instantiate: ") + hipGetErrorString(e));
      graph_batch = batch;
    }
    LLM_HIP_RET(hipGraphLaunch(graph, st));
  }
  for (int b = 0; b < batch; ++b) h_pos[b] += 1;
  if (logits_dev)
    LLM_HIP_RET(hipMemcpyAsync(logits_dev, logits.p, sizeof(float) * batch * V,
                               hipMemcpyDeviceToDevice, st));
  if (beam_mode) {  // the candidates of num_seqs = batch / W sequences, 2W each
    h_cand.resize((size_t)6 * batch);
    const size_t nb = sizeof(int32_t) * 2 * batch;
    LLM_HIP_RET(hipMemcpyAsync(h_cand.data(), cand_score.p, nb, hipMemcpyDeviceToHost, st));
    LLM_HIP_RET(hipMemcpyAsync(h_cand.data() + 2 * batch, cand_parent.p, nb,
                               hipMemcpyDeviceToHost, st));
    LLM_HIP_RET(hipMemcpyAsync(h_cand.data() + 4 * batch, cand_token.p, nb,
                               hipMemcpyDeviceToHost, st));
  }
  if (next_host) {
    LLM_HIP_RET(hipMemcpyAsync(next_host, tokens.p, sizeof(int32_t) * batch,
                               hipMemcpyDeviceToHost, st));
    if (oflag.p) {
      hipLaunchKernelGGL(take_flag_kernel, dim3(1), dim3(1), 0, st, oflag.p);
      LLM_HIP_RET(hipGetLastError());
      LLM_HIP_RET(hipMemcpyAsync(h_oflag, oflag.p + 1, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    LLM_HIP_RET(hipStreamSynchronize(st));
    if (oflag.p) return report_range(*h_oflag);
  }
  return LLM_OK;
}

// The fused o_proj's range guard (common.hpp oacc_term), reported ONCE: the
// flag is read and cleared in one device atomic (take_flag_kernel), so a
// clamp by a step still running on another stream is never lost between the
// read and the clear; a taken flag returns LLM_ERR_RANGE, and the steps after
// it (and the next llm_decoder_sync) succeed unless they clamp again.
// range_clamped keeps the fact for llm_decoder_oproj_status until the next
// begin / generate.  Caller holds mu; `flag` is take_flag_kernel's result.
int llm_decoder::report_range(int flag) {
  if (!flag) return LLM_OK;
  range_clamped = 1;
  return fail(LLM_ERR_RANGE,
              "decoder: a head product of the fused o_proj left its fixed-point range "
              "(|v| > (2^23 - 1) / num_heads, or not finite) and was clamped; the affected "
              "hidden values of that step are wrong");
}

int llm_decoder::oproj_range_status() {
  if (!oflag.p) return LLM_OK;
  int f = 0;
  hipLaunchKernelGGL(take_flag_kernel, dim3(1), dim3(1), 0, stream, oflag.p);
  LLM_HIP_RET(hipGetLastError());
  LLM_HIP_RET(hipMemcpyAsync(&f, oflag.p + 1, sizeof(int), hipMemcpyDeviceToHost, stream));
  LLM_HIP_RET(hipStreamSynchronize(stream));
  return report_range(f);
}

// The prefill buffers for passes of up to C rows (kept; grown on demand).
int llm_decoder::prefill_reserve(int C) {
  if (C > pf_cap) {
    const size_t C16 = ((size_t)C + 15) / 16 * 16;
    RET_IF(px.alloc((size_t)C * hid));
    RET_IF(pq.alloc((size_t)C * hid));
    RET_IF(po.alloc((size_t)C * hid));
    RET_IF(ph1.alloc((size_t)C * inter));
    RET_IF(psa.alloc((size_t)C));
    RET_IF(pact.alloc(C16 * std::max(hid, inter) * (wdtype == LLM_I8 ? 1 : 4)));  // F16: act, act2
    RET_IF(pmeta.alloc((size_t)8 * C));
    pws_bytes = 16;
    for (int b = 1; b <= C; ++b)
      pws_bytes = std::max(pws_bytes, pa_decode_workspace_bytes(b, H, D, max_tiles, 0));
    {  // the MFMA prefill's split partials (its split count is bounded at any p0)
      pa_kv_view v0;
      RET_IF(kv_cache_view(kv, 0, &v0));
      for (int b = 1; b <= C; ++b)
        pws_bytes = std::max(pws_bytes, pa_prefill_ws_bytes(&v0, cfg.max_seq_len - b, b));
      // ... and a packed pass's, whatever its segments
      pws_bytes = std::max(pws_bytes, pa_prefill_packed_part_bound(&v0, C));
    }
    RET_IF(pws.alloc(pws_bytes));
    pf_cap = C;
  }
  return LLM_OK;
}

// A segment of a prefill pass: len prompt tokens (toks) at positions p0 .. of
// active row `row`; last: the row's prompt ends with it.
struct llm_decoder::PassSeg {
  int row, p0, len;
  const int32_t* toks;
  bool last;
};

// One layer pass over the tokens of `segs` (the reference's is_prefill pass,
// attention/attention_cuda.hpp:21): the tokens are the rows of the pass —
// M = pass-size weight GEMMs, the K/V of every token appended to its row's
// pages by the qkv epilogue, and causal attention.  Everything in the pass is
// row-wise (pmeta carries each packed row's position, context, page-table row
// and token: through the paged decode kernel, token i of a segment attends to
// its row's positions < p0 + i + 1 via beam_ids = row, context_lens = p0 + i
// + 1) except the MFMA attention: `packed` takes the pass's tile table
// (pa_prefill_packed), else the pass is one segment and takes the
// single-sequence launch (pa_prefill; no tile table is built or uploaded).
// A row whose last token is in the pass gets its next token from that packed
// row's logits (argmax / sampling), so decode steps continue from the prompt.
int llm_decoder::prefill_pass(const std::vector<PassSeg>& segs, bool packed, hipStream_t st) {
  const int CAP = pf_cap;  // pmeta's array stride
  const int nseg = (int)segs.size();
  std::vector<int32_t> meta((size_t)(packed ? 8 : 4) * CAP), pc((size_t)2 * nseg);
  int m = 0, maxend = 0, ntile = 0;
  for (const PassSeg& s : segs) {
    LLM_REQUIRE(m + s.len <= CAP && (packed || nseg == 1), "prefill: bad pass");
    for (int i = 0; i < s.len; ++i) {
      meta[m + i] = s.p0 + i;
      meta[CAP + m + i] = s.p0 + i + 1;
      meta[2 * CAP + m + i] = s.row;
      meta[3 * CAP + m + i] = s.toks[i];
    }
    m += s.len;
    maxend = std::max(maxend, s.p0 + s.len);
  }
  if (packed) {
    pa_kv_view v0;
    RET_IF(kv_cache_view(kv, 0, &v0));
    std::vector<pa_prefill_seg> tsegs;
    for (const PassSeg& s : segs) tsegs.push_back(pa_prefill_seg{s.row, s.p0, s.len});
    ntile = pa_prefill_packed_tiles(&v0, tsegs.data(), nseg, meta.data() + 4 * CAP, CAP);
    LLM_REQUIRE(ntile >= 1 && ntile <= CAP, "prefill_rows: bad segment list");
  }
  {
    KvCache* k = kv_impl(kv);
    std::lock_guard<std::mutex> gk(k->mu);
    for (const PassSeg& s : segs) {
      // windowed: the segment's first query sees tokens >= p0 - window + 1, the
      // later ones no earlier (released first: the pass may need those pages)
      if (window > 0) RET_IF(k->release_before(s.row, s.p0 - window + 1));
      for (int t = s.p0; t < s.p0 + s.len; t = (t / TS + 1) * TS) RET_IF(k->prepare_append(s.row, t));
    }
    RET_IF(k->sync(st));
  }
  LLM_HIP_RET(hipMemcpyAsync(pmeta.p, meta.data(), ((size_t)4 * CAP + 4 * ntile) * sizeof(int32_t),
                             hipMemcpyHostToDevice, st));
  Rows R;
  R.n = m;
  R.x = px.p; R.q = pq.p; R.o = po.p; R.h1 = ph1.p; R.act = pact.p; R.sa = psa.p;
  if (wdtype == LLM_F16)
    R.act2 = pact.p + (((size_t)CAP + 15) / 16 * 16) * std::max(hid, inter) * 2;
  R.pos = pmeta.p; R.ctx = pmeta.p + CAP; R.beam_rows = pmeta.p + 2 * CAP;
  if (packed) {
    R.prefill_tiles = pmeta.p + 4 * CAP;
    R.prefill_ntile = ntile;
    R.prefill_maxend = maxend;
  } else {
    R.prefill_row = segs[0].row;
    R.prefill_p0 = segs[0].p0;
  }
  R.attn_ws = pws.p; R.attn_ws_bytes = pws_bytes;
  LLM_HIP_RET(launch_embed(emb.p, pmeta.p + 3 * CAP, m, hid, V, px.p, st));
  for (int l = 0; l < L; ++l) {
    RET_IF(layer_pre(l, st, R));
    RET_IF(layer_attn(l, st, R));
    RET_IF(layer_post(l, st, R));
  }
  int q0 = 0;
  for (int j = 0; j < nseg; ++j) {
    const PassSeg& s = segs[j];
    const int last = q0 + s.len - 1;
    h_pos[s.row] = s.p0 + s.len;
    // (serving: the step that follows takes its token and positions from the
    // host -- serve_step -- so an admission pays no LM head)
    if (s.last && !serving) {  // the row's last token: logits -> its next token, decode state
      RET_IF(next_tokens(px.p + (size_t)last * hid, 1, s.row, pmeta.p + last, st));
      pc[2 * j] = s.p0 + s.len;
      pc[2 * j + 1] = s.p0 + s.len + 1;
      LLM_HIP_RET(hipMemcpyAsync(pos.p + s.row, &pc[2 * j], sizeof(int32_t),
                                 hipMemcpyHostToDevice, st));
      LLM_HIP_RET(hipMemcpyAsync(ctx.p + s.row, &pc[2 * j + 1], sizeof(int32_t),
                                 hipMemcpyHostToDevice, st));
    }
    q0 += s.len;
  }
  LLM_HIP_RET(hipStreamSynchronize(st));  // meta / pc are this pass's staging
  return LLM_OK;
}

// The prompts of `nrows` active rows (lens[i] tokens of row rows[i], `total`
// > 0 in all, concatenated in toks; checked by the caller) through layer
// passes of up to kPrefillChunk tokens, packed by prefill_passes
// (prefill_pack.hpp): segments of different rows share a pass, and a long
// prompt continues in the next pass.
int llm_decoder::prefill_run(const int32_t* rows, const int32_t* toks, const int32_t* lens,
                             int nrows, long long total, bool packed, hipStream_t st) {
  const int C = (int)std::min<long long>(total, kPrefillChunk);
  RET_IF(prefill_reserve(C));
  std::vector<int> start(nrows);
  std::vector<const int32_t*> row_toks(nrows);
  for (int i = 0; i < nrows; ++i) {
    start[i] = h_pos[rows[i]];
    row_toks[i] = toks;
    toks += lens[i];
  }
  std::vector<PassSeg> segs;
  for (const PrefillPass& pass : prefill_passes(start.data(), lens, nrows, C)) {
    segs.clear();
    for (const PrefillSeg& s : pass) {
      const int off = s.p0 - start[s.src];
      segs.push_back(PassSeg{rows[s.src], s.p0, s.len, row_toks[s.src] + off,
                             off + s.len == lens[s.src]});
    }
    RET_IF(prefill_pass(segs, packed, st));
  }
  return LLM_OK;
}

// Chunked prefill of `n` prompt tokens of active row `row` (llm_decoder_prefill):
// one segment per pass, attended by the single-sequence launch.
int llm_decoder::prefill(int row, const int32_t* toks, int n, hipStream_t st) {
  LLM_REQUIRE(weights_ready, "prefill: weights not loaded");
  LLM_REQUIRE(row >= 0 && row < batch, "prefill: row is not active");
  LLM_REQUIRE(n >= 1 && toks, "prefill: need >= 1 token");
  LLM_REQUIRE(h_pos[row] + n < cfg.max_seq_len, "prefill: prompt exceeds max_seq_len");
  for (int i = 0; i < n; ++i) LLM_REQUIRE(toks[i] >= 0 && toks[i] < V, "prefill: token id out of range");
  return prefill_run(&row, toks, &n, 1, n, false, st);
}

// Packed prefill (llm_decoder_prefill_rows): the prompts of several active rows
// through shared layer passes, attended by the tile-table launch (also where
// a pass holds one segment: the two launches plan their splits differently).
int llm_decoder::prefill_rows(const int32_t* rows, const int32_t* toks, const int32_t* lens,
                              int nrows, hipStream_t st) {
  LLM_REQUIRE(weights_ready, "prefill_rows: weights not loaded");
  LLM_REQUIRE(nrows >= 0 && (nrows == 0 || (rows && lens)), "prefill_rows: NULL argument");
  long long total = 0;
  std::vector<char> seen(batch, 0);
  for (int i = 0; i < nrows; ++i) {
    LLM_REQUIRE(rows[i] >= 0 && rows[i] < batch, "prefill_rows: row is not active");
    LLM_REQUIRE(!seen[rows[i]], "prefill_rows: a row is given twice");
    seen[rows[i]] = 1;
    LLM_REQUIRE(lens[i] >= 0, "prefill_rows: negative length");
    LLM_REQUIRE((long long)h_pos[rows[i]] + lens[i] < cfg.max_seq_len,
                "prefill_rows: prompt exceeds max_seq_len");
    total += lens[i];
  }
  LLM_REQUIRE(total == 0 || toks, "prefill_rows: tokens is NULL");
  for (long long i = 0; i < total; ++i)
    LLM_REQUIRE(toks[i] >= 0 && toks[i] < V, "prefill_rows: token id out of range");
  if (total == 0) return LLM_OK;
  return prefill_run(rows, toks, lens, nrows, total, true, st);
}

// prompt[:-1] of n sequences into rows s * row_step (generate: every row;
// beam search: beam 0 of every sequence), through shared passes
// (packed_prefill) or row by row.  The prefill's own token choice is not used.
int llm_decoder::prefill_prompts(const int32_t* prompts, const int32_t* prompt_lens,
                                 int prompt_stride, int n, int row_step) {
  std::vector<int32_t> prow(n), plen(n), ptok;
  for (int s = 0; s < n; ++s) {
    const int32_t* ps = prompts + (size_t)s * prompt_stride;
    prow[s] = s * row_step;
    plen[s] = prompt_lens[s] - 1;
    if (packed_prefill) ptok.insert(ptok.end(), ps, ps + plen[s]);
    else if (plen[s] > 0) RET_IF(prefill(prow[s], ps, plen[s], stream));
  }
  if (packed_prefill) return prefill_rows(prow.data(), ptok.data(), plen.data(), n, stream);
  return LLM_OK;
}

static int reset_rows(llm_decoder* d, int batch, int start_pos) {
  LLM_REQUIRE(batch > 0 && batch <= d->maxB, "decoder: batch must be in [1, max_batch]");
  RET_IF(kv_cache_clear(d->kv));
  d->batch = batch;
  if (d->row_group != 1) d->graph_batch = -1;  // the captured attention launch used the beam group
  d->row_group = 1;
  d->h_pos.assign(d->maxB, 0);
  for (int b = 0; b < batch; ++b) d->h_pos[b] = start_pos;
  if (d->oacc.p) LLM_HIP_RET(hipMemset(d->oacc.p, 0, sizeof(long long) * d->oacc.n));
  if (d->oflag.p) LLM_HIP_RET(hipMemset(d->oflag.p, 0, sizeof(int)));
  d->range_clamped = 0;
  std::vector<int32_t> pos(batch, start_pos), ctx(batch, start_pos + 1), tok(batch, 0);
  LLM_HIP_RET(hipMemcpy(d->pos.p, pos.data(), sizeof(int32_t) * batch, hipMemcpyHostToDevice));
  LLM_HIP_RET(hipMemcpy(d->ctx.p, ctx.data(), sizeof(int32_t) * batch, hipMemcpyHostToDevice));
  LLM_HIP_RET(hipMemcpy(d->tokens.p, tok.data(), sizeof(int32_t) * batch, hipMemcpyHostToDevice));
  LLM_HIP_RET(hipDeviceSynchronize());
  return LLM_OK;
}

// Non-contiguous page gather (shuffled page pool, seed 7).
static void shuffle_free_pages(KvCache* k, uint64_t seed) {
  std::lock_guard<std::mutex> gk(k->mu);
  std::mt19937_64 rng(seed ^ 7);
  for (auto& f : k->free_lists) std::shuffle(f.begin(), f.end(), rng);
}

// The reserved page tables pushed, then seeded random K/V over the whole
// pools (K scaled so q.k ~ O(1)); LLM_FP8 pools hold the same values encoded
// at scale 1.
static int fill_pools(llm_decoder* d, uint64_t seed) {
  KvCache* k = kv_impl(d->kv);
  RET_IF(kv_cache_sync(d->kv, d->stream));
  const size_t np = (size_t)k->num_pages, pe = k->page_elems, ps = k->page_stride() / k->es;
  const auto fill = d->kvt == LLM_FP8 ? launch_fill_random_fp8 : launch_fill_random_f16;
  LLM_HIP_RET(fill(k->k_pool, np, pe, ps, seed * 2 + 1, 0.05f, d->stream));
  LLM_HIP_RET(fill(k->v_pool, np, pe, ps, seed * 2 + 2, 1.0f, d->stream));
  LLM_HIP_RET(hipStreamSynchronize(d->stream));
  return LLM_OK;
}

extern "C" int llm_decoder_begin_synthetic(llm_decoder* d, int batch, int context_len,
                                           uint64_t seed, int shuffle) {
  LLM_REQUIRE(d, "llm_decoder_begin_synthetic: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  NOT_SERVING(d, "llm_decoder_begin_synthetic");
  LLM_REQUIRE(context_len >= 0 && context_len < d->cfg.max_seq_len,
              "llm_decoder_begin_synthetic: context_len must be in [0, max_seq_len)");
  LLM_HIP_RET(hipStreamSynchronize(d->stream));
  RET_IF(reset_rows(d, batch, context_len));
  if (shuffle) shuffle_free_pages(kv_impl(d->kv), seed);
  for (int b = 0; b < batch; ++b) RET_IF(kv_cache_reserve(d->kv, b, context_len));
  return fill_pools(d, seed);
}

extern "C" int llm_decoder_begin_beams(llm_decoder* d, int num_seqs, int beam_width,
                                       int shared_len, int beam_len, uint64_t seed, int shuffle) {
  LLM_REQUIRE(d, "llm_decoder_begin_beams: NULL");
  LLM_REQUIRE(num_seqs > 0 && beam_width >= 1 && beam_width <= 4 && shared_len >= 0 &&
                  beam_len >= 0,
              "llm_decoder_begin_beams: bad arguments (beam_width in [1, 4])");
  std::lock_guard<std::mutex> g(d->mu);
  NOT_SERVING(d, "llm_decoder_begin_beams");
  if (d->window > 0)
    return fail(LLM_ERR_UNSUPPORTED, "llm_decoder_begin_beams: the decoder has a sliding window "
                                     "(llm_decoder_set_window): beam groups take none");
  const int ctx_len = shared_len + beam_len;
  LLM_REQUIRE(ctx_len < d->cfg.max_seq_len,
              "llm_decoder_begin_beams: shared_len + beam_len must be < max_seq_len");
  LLM_HIP_RET(hipStreamSynchronize(d->stream));
  const int batch = num_seqs * beam_width;
  RET_IF(reset_rows(d, batch, ctx_len));
  if (shuffle) shuffle_free_pages(kv_impl(d->kv), seed);
  // beam 0 of each sequence owns the shared prefix; the other beams fork its
  // page table (shared pages, refcounted) and then get private pages for their
  // own beam_len tokens.
  for (int sq = 0; sq < num_seqs; ++sq) {
    const int b0 = sq * beam_width;
    RET_IF(kv_cache_reserve(d->kv, b0, shared_len));
    for (int w = 1; w < beam_width; ++w) RET_IF(kv_cache_fork(d->kv, b0, b0 + w));
    for (int w = 0; w < beam_width; ++w) RET_IF(kv_cache_reserve(d->kv, b0 + w, ctx_len));
  }
  RET_IF(fill_pools(d, seed));
  d->row_group = beam_width;
  d->graph_batch = -1;  // re-capture: the attention launch depends on row_group
  return LLM_OK;
}

extern "C" int llm_decoder_prefill(llm_decoder* d, int row, const int32_t* tokens, int n) {
  LLM_REQUIRE(d, "llm_decoder_prefill: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  NOT_SERVING(d, "llm_decoder_prefill");
  return d->prefill(row, tokens, n, d->stream);
}

extern "C" int llm_decoder_prefill_rows(llm_decoder* d, const int32_t* rows, const int32_t* tokens,
                                        const int32_t* lens, int nrows) {
  LLM_REQUIRE(d, "llm_decoder_prefill_rows: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  NOT_SERVING(d, "llm_decoder_prefill_rows");
  return d->prefill_rows(rows, tokens, lens, nrows, d->stream);
}

extern "C" int llm_decoder_set_packed_prefill(llm_decoder* d, int on) {
  LLM_REQUIRE(d, "llm_decoder_set_packed_prefill: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  NOT_SERVING(d, "llm_decoder_set_packed_prefill");
  d->packed_prefill = on != 0;
  return LLM_OK;
}

extern "C" int llm_decoder_packed_prefill(const llm_decoder* d) {
  return d ? (d->packed_prefill ? 1 : 0) : -1;
}

extern "C" int llm_decoder_set_sampling(llm_decoder* d, float temperature, int top_k, float top_p,
                                        uint64_t seed) {
  LLM_REQUIRE(d, "llm_decoder_set_sampling: NULL");
  LLM_REQUIRE(top_k >= 0 && top_p > 0.f && top_p <= 1.f && d->V <= 65536,
              "llm_decoder_set_sampling: top_k >= 0, 0 < top_p <= 1, vocab <= 65536");
  std::lock_guard<std::mutex> g(d->mu);
  NOT_SERVING(d, "llm_decoder_set_sampling");
  LLM_HIP_RET(hipStreamSynchronize(d->stream));
  d->temperature = temperature;
  d->top_k = top_k;
  d->top_p = top_p;
  d->sample_seed = seed;
  d->graph_batch = -1;  // the step graph changes
  return LLM_OK;
}

extern "C" int llm_decoder_set_taps(llm_decoder* d, int8_t* q_dev, float* s_dev) {
  LLM_REQUIRE(d, "llm_decoder_set_taps: NULL");
  LLM_REQUIRE((q_dev == nullptr) == (s_dev == nullptr),
              "llm_decoder_set_taps: give both tap buffers or neither");
  std::lock_guard<std::mutex> g(d->mu);
  NOT_SERVING(d, "llm_decoder_set_taps");
  LLM_HIP_RET(hipStreamSynchronize(d->stream));
  d->tap_q = q_dev;
  d->tap_s = s_dev;
  d->graph_batch = -1;  // the step graph gains / loses the tap copies
  return LLM_OK;
}

extern "C" int llm_decoder_attention_plan(llm_decoder* d, int* nsplit, int* form) {
  LLM_REQUIRE(d && nsplit && form, "llm_decoder_attention_plan: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  LLM_REQUIRE(d->batch > 0, "llm_decoder_attention_plan: no active rows");
  Rows R;
  RET_IF(d->decode_rows(&R));
  pa_kv_view view;
  PaRequest rq;
  PaLaunch p;
  RET_IF(d->attn_request(R, &view, &rq));
  RET_IF(pa_decode_internal(&view, rq, nullptr, d->hid, nullptr, nullptr, nullptr, 1.f, nullptr, 0,
                            nullptr, nullptr, &p));
  *nsplit = p.nsplit;
  *form = p.form();
  return LLM_OK;
}

extern "C" int llm_decoder_run_attention(llm_decoder* d, int layer, void* stream) {
  LLM_REQUIRE(d, "llm_decoder_run_attention: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  LLM_REQUIRE(d->batch > 0, "llm_decoder_run_attention: no active rows");
  LLM_REQUIRE(layer >= 0 && layer < d->L, "llm_decoder_run_attention: layer out of range");
  hipStream_t st = stream ? as_stream(stream) : d->stream;
  Rows R;
  RET_IF(d->decode_rows(&R, true));  // (a timed run: its own o_proj target)
  return d->layer_attn(layer, st, R);
}

extern "C" int llm_decoder_oproj_status(llm_decoder* d, int* clamped, long long* nonzero_columns) {
  LLM_REQUIRE(d, "llm_decoder_oproj_status: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  LLM_HIP_RET(hipDeviceSynchronize());
  int f = 0;
  long long nz = 0;
  if (d->oflag.p) LLM_HIP_RET(hipMemcpy(&f, d->oflag.p, sizeof(int), hipMemcpyDeviceToHost));
  f = f || d->range_clamped;
  for (const DevBuf<long long>* b : {&d->oacc, &d->oacc_run}) {
    if (!b->p) continue;
    std::vector<long long> h(b->n);
    LLM_HIP_RET(hipMemcpy(h.data(), b->p, sizeof(long long) * b->n, hipMemcpyDeviceToHost));
    for (long long v : h) nz += v != 0;
  }
  if (clamped) *clamped = f;
  if (nonzero_columns) *nonzero_columns = nz;
  return LLM_OK;
}

extern "C" int llm_decoder_step(llm_decoder* d, const int32_t* tokens, float* logits_dev,
                                int32_t* next_host, void* stream) {
  LLM_REQUIRE(d, "llm_decoder_step: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  NOT_SERVING(d, "llm_decoder_step");
  hipStream_t st = stream ? as_stream(stream) : d->stream;
  return d->run_step(tokens, logits_dev, next_host, st);
}

extern "C" int llm_decoder_copy_next(llm_decoder* d, int32_t* dst_dev, void* stream) {
  LLM_REQUIRE(d && dst_dev, "llm_decoder_copy_next: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  LLM_REQUIRE(d->batch > 0, "llm_decoder_copy_next: no active rows");
  hipStream_t st = stream ? as_stream(stream) : d->stream;
  LLM_HIP_RET(hipMemcpyAsync(dst_dev, d->tokens.p, sizeof(int32_t) * d->batch,
                             hipMemcpyDeviceToDevice, st));
  return LLM_OK;
}

extern "C" int llm_decoder_sync(llm_decoder* d) {
  LLM_REQUIRE(d, "llm_decoder_sync: NULL");
  LLM_HIP_RET(hipDeviceSynchronize());
  std::lock_guard<std::mutex> g(d->mu);
  return d->oproj_range_status();
}

extern "C" int llm_decoder_context_len(const llm_decoder* d, int row) {
  if (!d || row < 0 || row >= d->batch) return -1;
  return d->h_pos[row];
}

// The prompts of generate / beam_search (`who`): every one 1 .. prompt_stride
// tokens of the vocabulary.  *max_len: the longest.
static int check_prompts(const std::string& who, const llm_decoder* d, const int32_t* prompts,
                         const int32_t* prompt_lens, int prompt_stride, int n, int* max_len) {
  *max_len = 0;
  for (int s = 0; s < n; ++s) {
    LLM_REQUIRE(prompt_lens[s] >= 1 && prompt_lens[s] <= prompt_stride,
                who + ": every prompt needs >= 1 token");
    for (int i = 0; i < prompt_lens[s]; ++i) {
      const int t = prompts[(size_t)s * prompt_stride + i];
      LLM_REQUIRE(t >= 0 && t < d->V, who + ": token id out of range");
    }
    *max_len = std::max(*max_len, prompt_lens[s]);
  }
  return LLM_OK;
}

extern "C" int llm_decoder_generate(llm_decoder* d, const int32_t* prompts,
                                    const int32_t* prompt_lens, int prompt_stride, int batch,
                                    int max_gen_len, float temperature, int32_t* out) {
  LLM_REQUIRE(d && prompts && prompt_lens && out, "llm_decoder_generate: NULL");
  LLM_REQUIRE(max_gen_len >= 0, "llm_decoder_generate: max_gen_len < 0");
  // generate is greedy argmax whatever the temperature, as the reference's
  // sample_from_logits (decoder/cuda_decoder.cu:7-14): argmax is invariant to
  // temperature > 0.  A device-sampling mode set by llm_decoder_set_sampling
  // applies to llm_decoder_step only; it is suspended here and restored after.
  (void)temperature;
  std::lock_guard<std::mutex> g(d->mu);
  NOT_SERVING(d, "llm_decoder_generate");
  struct SamplingGuard {
    llm_decoder* d;
    float t;
    bool active;
    explicit SamplingGuard(llm_decoder* dd)
        : d(dd), t(dd->temperature), active(dd->temperature > 0.f && dd->top_k != 1) {
      if (active) { d->temperature = 0.f; d->graph_batch = -1; }
    }
    ~SamplingGuard() {
      if (active) { d->temperature = t; d->graph_batch = -1; }
    }
  } sampling_guard(d);
  LLM_REQUIRE(batch >= 1 && batch <= d->maxB, "llm_decoder_generate: batch out of range");
  int max_len = 0;
  RET_IF(check_prompts("llm_decoder_generate", d, prompts, prompt_lens, prompt_stride, batch,
                       &max_len));
  if (max_gen_len == 0) return LLM_OK;
  LLM_REQUIRE(max_len + max_gen_len - 1 <= d->cfg.max_seq_len,
              "llm_decoder_generate: prompt + max_gen_len exceeds max_seq_len");
  LLM_HIP_RET(hipStreamSynchronize(d->stream));
  RET_IF(reset_rows(d, batch, 0));
  // every prompt but its last token goes through chunked prefill; decode steps
  // then run all rows in lockstep, each at its own position
  RET_IF(d->prefill_prompts(prompts, prompt_lens, prompt_stride, batch, 1));
  // a step whose fused o_proj clamped (LLM_ERR_RANGE) still produced its ids:
  // generation runs to the end, fills `out`, and then returns the status
  std::vector<int32_t> tok(batch), next(batch);
  int range_rc = LLM_OK;
  for (int s = 0; s < max_gen_len; ++s) {
    for (int b = 0; b < batch; ++b)
      tok[b] = s == 0 ? prompts[(size_t)b * prompt_stride + prompt_lens[b] - 1] : next[b];
    const int rc = d->run_step(tok.data(), nullptr, next.data(), d->stream);
    if (rc == LLM_ERR_RANGE) range_rc = rc;
    else RET_IF(rc);
    for (int b = 0; b < batch; ++b) out[(size_t)b * max_gen_len + s] = next[b];
  }
  if (range_rc) return fail(LLM_ERR_RANGE, "llm_decoder_generate: the fused o_proj clamped a head "
                                           "product in at least one step; `out` is complete, the "
                                           "ids after that step may differ");
  return LLM_OK;
}

// ---------------------------------------------------------------------------
// continuous batching (llm_decoder.h: llm_decoder_serve_*)
// ---------------------------------------------------------------------------
// The live rows' device state from the host's: positions and context lengths
// (h_pos) and the requests' sampling settings.  Called when the rows changed
// (an admission or a move), before the step; the staging vectors stay
// untouched until the step's closing synchronisation.
int llm_decoder::serve_upload() {
  const int n = plan.live();
  for (int r = 0; r < n; ++r) {
    const llm_request_options& o = requests.at(plan.row(r).id).opt;
    hs_temp[r] = o.temperature;
    hs_topk[r] = o.top_k;
    hs_topp[r] = o.top_p;
    hs_seed[r] = o.seed;
    hs_pos[r] = h_pos[r];
    hs_ctx[r] = h_pos[r] + 1;
  }
  auto up = [&](void* dst, const void* src, size_t bytes) {
    return hipMemcpyAsync(dst, src, bytes * n, hipMemcpyHostToDevice, stream);
  };
  LLM_HIP_RET(up(sv_temp.p, hs_temp.data(), sizeof(float)));
  LLM_HIP_RET(up(sv_topk.p, hs_topk.data(), sizeof(int32_t)));
  LLM_HIP_RET(up(sv_topp.p, hs_topp.data(), sizeof(float)));
  LLM_HIP_RET(up(sv_seed.p, hs_seed.data(), sizeof(uint64_t)));
  LLM_HIP_RET(up(pos.p, hs_pos.data(), sizeof(int32_t)));
  LLM_HIP_RET(up(ctx.p, hs_ctx.data(), sizeof(int32_t)));
  serve_dirty = false;
  return LLM_OK;
}

// Row `row` was retired by plan (its request `id` ended or was cancelled;
// nothing is in flight): its pages go back, and if plan moved the last live
// row into it (mv), that row's page-table entries are re-parented (fork =
// shared, release of the source = owned again with refcount 1: no page is
// copied, and the next append writes in place) and its host position follows;
// the device copies are rewritten by the next step's serve_upload.
int llm_decoder::serve_release(int row, long long id, const ServeMove* mv) {
  requests.erase(id);
  RET_IF(kv_cache_release(kv, row));
  h_pos[row] = 0;
  if (mv) {
    RET_IF(kv_cache_fork(kv, mv->src, mv->dst));
    RET_IF(kv_cache_release(kv, mv->src));
    h_pos[mv->dst] = h_pos[mv->src];
    h_pos[mv->src] = 0;
    serve_dirty = true;
  }
  batch = plan.live();
  return LLM_OK;
}

static_assert(LLM_FINISH_EOS == 1 && LLM_FINISH_LENGTH == 2, "ServePlan::finish_step's reasons");

int llm_decoder::serve_step(float* logits_dev, llm_serve_event* events, int* n_events) {
  const int before = plan.live(), na = plan.admit(), live = plan.live();
  if (live == 0) return LLM_OK;
  batch = live;
  if (na) {
    serve_dirty = true;
    // prompt[:-1] of the new rows, as prefill_prompts chooses
    std::vector<int32_t> prow, plen, ptok;
    for (int r = before; r < live; ++r) {
      const std::vector<int32_t>& p = requests.at(plan.row(r).id).prompt;
      const int n = (int)p.size() - 1;
      h_pos[r] = 0;
      if (packed_prefill) {
        prow.push_back(r);
        plen.push_back(n);
        ptok.insert(ptok.end(), p.begin(), p.begin() + n);
      } else if (n > 0) {
        RET_IF(prefill(r, p.data(), n, stream));
      }
    }
    if (packed_prefill) RET_IF(prefill_rows(prow.data(), ptok.data(), plen.data(), na, stream));
  }
  if (serve_dirty) RET_IF(serve_upload());
  for (int r = 0; r < live; ++r) hs_tok[r] = requests.at(plan.row(r).id).feed;
  const bool new_graph = use_graph && graph_batch != batch;  // (run_step instantiates then)
  const int rc = run_step(hs_tok.data(), logits_dev, hs_next.data(), stream);
  if (rc != LLM_ERR_RANGE) RET_IF(rc);  // (a clamped step still produced its ids)
  graph_instantiations += new_graph;
  *n_events = live;
  RET_IF(plan.finish_step(
      [&](int r, const ServeReq& q) {
        ServeRequest& rq = requests.at(q.id);
        rq.feed = hs_next[r];
        events[r] = llm_serve_event{q.id, rq.feed, q.delivered, r, 0};
        return rq.feed == rq.opt.eos_token;
      },
      [&](int r, const ServeReq& q, int finish, const ServeMove* mv) {
        events[r].finish = finish;  // (LLM_FINISH_EOS / _LENGTH are finish_step's 1 / 2)
        return serve_release(r, q.id, mv);
      }));
  if (rc) return fail(LLM_ERR_RANGE, "llm_decoder_serve_step: the fused o_proj clamped a head "
                                     "product in this step; the events are complete, the ids "
                                     "after it may differ");
  return LLM_OK;
}

extern "C" int llm_decoder_serve_begin(llm_decoder* d) {
  LLM_REQUIRE(d, "llm_decoder_serve_begin: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  LLM_REQUIRE(!d->serving, "llm_decoder_serve_begin: already serving");
  LLM_REQUIRE(d->weights_ready, "llm_decoder_serve_begin: weights not loaded");
  // (beam_mode is set only for the length of llm_decoder_beam_search, which
  // holds the mutex; the test states the entry's contract)
  if (d->beam_mode)
    return fail(LLM_ERR_UNSUPPORTED, "llm_decoder_serve_begin: the decoder is in beam mode");
  if (d->V > 65536)
    return fail(LLM_ERR_UNSUPPORTED, "llm_decoder_serve_begin: vocab_size > 65536 (the rows' "
                                     "tokens are chosen by sample_rows_each)");
  LLM_HIP_RET(hipStreamSynchronize(d->stream));
  RET_IF(kv_cache_clear(d->kv));
  d->batch = 0;
  d->row_group = 1;
  d->h_pos.assign(d->maxB, 0);
  if (d->oacc.p) LLM_HIP_RET(hipMemset(d->oacc.p, 0, sizeof(long long) * d->oacc.n));
  if (d->oflag.p) LLM_HIP_RET(hipMemset(d->oflag.p, 0, sizeof(int)));
  LLM_HIP_RET(hipDeviceSynchronize());  // null-stream memsets vs. the decoder's stream
  d->range_clamped = 0;
  const size_t B = (size_t)d->maxB;
  if (!d->sv_temp.p) {
    RET_IF(d->sv_temp.alloc(B));
    RET_IF(d->sv_topk.alloc(B));
    RET_IF(d->sv_topp.alloc(B));
    RET_IF(d->sv_seed.alloc(B));
  }
  d->hs_temp.assign(B, 0.f); d->hs_topp.assign(B, 1.f); d->hs_topk.assign(B, 0);
  d->hs_seed.assign(B, 0); d->hs_pos.assign(B, 0); d->hs_ctx.assign(B, 1);
  d->hs_tok.assign(B, 0); d->hs_next.assign(B, 0);
  ServeGeom geom;
  geom.max_rows = d->maxB;
  geom.num_pages = kv_cache_num_pages(d->kv);
  geom.pages_per_tile = d->L * d->H;
  geom.page_size = d->TS;
  geom.window = d->window;
  geom.max_seq_len = d->cfg.max_seq_len;
  d->plan.begin(geom);
  d->requests.clear();
  d->serve_dirty = false;
  d->serving = true;
  d->graph_batch = -1;  // the step's token choice becomes sample_rows_each
  return LLM_OK;
}

extern "C" int llm_decoder_serve_end(llm_decoder* d) {
  LLM_REQUIRE(d, "llm_decoder_serve_end: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  LLM_REQUIRE(d->serving, "llm_decoder_serve_end: not serving");
  LLM_HIP_RET(hipStreamSynchronize(d->stream));
  d->plan.begin(d->plan.geom());
  d->requests.clear();
  d->serving = false;
  d->graph_batch = -1;
  d->batch = 0;
  d->h_pos.assign(d->maxB, 0);
  return kv_cache_clear(d->kv);
}

extern "C" int llm_decoder_submit(llm_decoder* d, const int32_t* prompt, int n,
                                  const llm_request_options* opt, long long* id) {
  LLM_REQUIRE(d && prompt && opt && id, "llm_decoder_submit: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  LLM_REQUIRE(d->serving, "llm_decoder_submit: not serving (llm_decoder_serve_begin first)");
  LLM_REQUIRE(n >= 1, "llm_decoder_submit: a prompt needs >= 1 token");
  LLM_REQUIRE(opt->max_new_tokens >= 1, "llm_decoder_submit: max_new_tokens must be >= 1");
  LLM_REQUIRE(opt->eos_token >= -1 && opt->eos_token < d->V,
              "llm_decoder_submit: eos_token must be -1 or a token id");
  LLM_REQUIRE(std::isfinite(opt->temperature) && opt->top_k >= 0 && opt->top_p > 0.f &&
                  opt->top_p <= 1.f,
              "llm_decoder_submit: temperature finite, top_k >= 0, 0 < top_p <= 1");
  for (int i = 0; i < n; ++i)
    LLM_REQUIRE(prompt[i] >= 0 && prompt[i] < d->V, "llm_decoder_submit: token id out of range");
  LLM_REQUIRE(serve_positions(n, opt->max_new_tokens) <= d->cfg.max_seq_len,
              "llm_decoder_submit: prompt + max_new_tokens exceeds max_seq_len");
  LLM_REQUIRE(d->plan.fits(n, opt->max_new_tokens),
              "llm_decoder_submit: the request needs " +
                  std::to_string(serve_need(d->plan.geom(), n, opt->max_new_tokens)) +
                  " pages, the pool has " + std::to_string(d->plan.geom().num_pages));
  const long long rid = d->plan.submit(n, opt->max_new_tokens);
  llm_decoder::ServeRequest& rq = d->requests[rid];
  rq.prompt.assign(prompt, prompt + n);
  rq.opt = *opt;
  rq.feed = prompt[n - 1];
  *id = rid;
  return LLM_OK;
}

extern "C" int llm_decoder_cancel(llm_decoder* d, long long id) {
  LLM_REQUIRE(d, "llm_decoder_cancel: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  LLM_REQUIRE(d->serving, "llm_decoder_cancel: not serving");
  if (d->plan.cancel_waiting(id)) {
    d->requests.erase(id);
    return LLM_OK;
  }
  const int row = d->plan.row_of(id);
  LLM_REQUIRE(row >= 0, "llm_decoder_cancel: no waiting or live request has this id");
  ServeMove mv;
  const bool moved = d->plan.retire(row, &mv);
  return d->serve_release(row, id, moved ? &mv : nullptr);
}

extern "C" int llm_decoder_serve_step(llm_decoder* d, float* logits_dev, llm_serve_event* events,
                                      int cap, int* n_events) {
  LLM_REQUIRE(d && events && n_events, "llm_decoder_serve_step: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  LLM_REQUIRE(d->serving, "llm_decoder_serve_step: not serving (llm_decoder_serve_begin first)");
  LLM_REQUIRE(cap >= d->maxB, "llm_decoder_serve_step: events needs room for max_batch entries");
  *n_events = 0;
  return d->serve_step(logits_dev, events, n_events);
}

extern "C" int llm_decoder_serve_stats(const llm_decoder* d, int* live, int* waiting,
                                       long long* committed_pages,
                                       long long* graph_instantiations) {
  LLM_REQUIRE(d, "llm_decoder_serve_stats: NULL");
  std::lock_guard<std::mutex> g(const_cast<llm_decoder*>(d)->mu);
  if (live) *live = d->plan.live();
  if (waiting) *waiting = d->plan.waiting();
  if (committed_pages) *committed_pages = d->plan.committed();
  if (graph_instantiations) *graph_instantiations = d->graph_instantiations;
  return LLM_OK;
}

// ---------------------------------------------------------------------------
// beam search (llm_decoder.h: llm_decoder_beam_search)
// ---------------------------------------------------------------------------
namespace {

struct BeamHyp {
  std::vector<int32_t> ids;
  float sum = 0.f;    // cumulative log-probability (the device's fp32 score)
  float score = 0.f;  // sum / len^alpha
};

float beam_final_score(float sum, size_t len, float alpha) {
  return (float)((double)sum / std::pow((double)len, (double)alpha));
}

}  // namespace

extern "C" int llm_decoder_beam_search(llm_decoder* d, const int32_t* prompts,
                                       const int32_t* prompt_lens, int prompt_stride,
                                       int num_seqs, const llm_beam_options* opt,
                                       int32_t* out_ids, int32_t* out_len,
                                       float* out_sum_logprob, float* out_score) {
  LLM_REQUIRE(d && prompts && prompt_lens && opt && out_ids && out_len && out_sum_logprob &&
                  out_score,
              "llm_decoder_beam_search: NULL");
  const int W = opt->beam_width, max_new = opt->max_new_tokens;
  LLM_REQUIRE(W >= 1 && W <= 4, "llm_decoder_beam_search: beam_width must be in [1, 4]");
  LLM_REQUIRE(max_new >= 1, "llm_decoder_beam_search: max_new_tokens must be >= 1");
  LLM_REQUIRE(opt->length_penalty >= 0.f && std::isfinite(opt->length_penalty),
              "llm_decoder_beam_search: length_penalty must be finite and >= 0");
  LLM_REQUIRE(opt->eos_token >= -1 && opt->eos_token < d->V,
              "llm_decoder_beam_search: eos_token must be -1 or a token id");
  LLM_REQUIRE(num_seqs >= 1 && (long long)num_seqs * W <= d->maxB,
              "llm_decoder_beam_search: num_seqs * beam_width must be in [1, max_batch]");
  LLM_REQUIRE(d->V >= 2 * W, "llm_decoder_beam_search: vocab_size < 2 * beam_width");
  LLM_REQUIRE(d->V <= 65536, "llm_decoder_beam_search: vocab_size > 65536");
  int max_len = 0;
  RET_IF(check_prompts("llm_decoder_beam_search", d, prompts, prompt_lens, prompt_stride, num_seqs,
                       &max_len));
  LLM_REQUIRE(max_len + max_new - 1 <= d->cfg.max_seq_len,
              "llm_decoder_beam_search: prompt + max_new_tokens exceeds max_seq_len");
  std::lock_guard<std::mutex> g(d->mu);
  NOT_SERVING(d, "llm_decoder_beam_search");
  if (d->window > 0)
    return fail(LLM_ERR_UNSUPPORTED, "llm_decoder_beam_search: the decoder has a sliding window "
                                     "(llm_decoder_set_window): beam groups take none");
  LLM_REQUIRE(d->weights_ready, "llm_decoder_beam_search: weights not loaded");
  // the step graph's token choice becomes the beam selection for the length
  // of the search (a sampling mode is untouched: beam mode takes precedence)
  struct ModeGuard {
    llm_decoder* d;
    ~ModeGuard() {
      if (d->beam_mode) { d->beam_mode = false; d->graph_batch = -1; }
    }
  } mode_guard{d};
  LLM_HIP_RET(hipStreamSynchronize(d->stream));
  const int rows = num_seqs * W, K = 2 * W;
  RET_IF(reset_rows(d, rows, 0));
  // prompt[:-1] into beam 0's pages (the prefill's own token choice, argmax or
  // a draw, is not used), shared with the other beams
  RET_IF(d->prefill_prompts(prompts, prompt_lens, prompt_stride, num_seqs, W));
  for (int s = 0; s < num_seqs; ++s) {
    const int b0 = s * W, n = prompt_lens[s] - 1;
    for (int w = 1; w < W; ++w) {
      if (n > 0) RET_IF(kv_cache_fork(d->kv, b0, b0 + w));
      d->h_pos[b0 + w] = n;
    }
  }
  std::vector<int32_t> pos(rows), ctx(rows), tok(rows), dummy(rows), parent(W);
  std::vector<float> score(rows);
  for (int r = 0; r < rows; ++r) {
    pos[r] = d->h_pos[r];
    ctx[r] = pos[r] + 1;
    tok[r] = prompts[(size_t)(r / W) * prompt_stride + prompt_lens[r / W] - 1];
    score[r] = r % W == 0 ? 0.f : -INFINITY;
  }
  LLM_HIP_RET(hipMemcpy(d->pos.p, pos.data(), sizeof(int32_t) * rows, hipMemcpyHostToDevice));
  LLM_HIP_RET(hipMemcpy(d->ctx.p, ctx.data(), sizeof(int32_t) * rows, hipMemcpyHostToDevice));
  d->row_group = W;
  d->beam_mode = true;
  d->graph_batch = -1;

  std::vector<std::vector<BeamHyp>> finished(num_seqs);
  std::vector<char> done(num_seqs, 0);
  std::vector<std::vector<int32_t>> hist(rows), next_hist(W);
  std::vector<float> next_score(W);
  std::vector<int32_t> next_tok(W);
  int range_rc = LLM_OK, steps = 0;
  for (int st = 0; st < max_new; ++st) {
    LLM_HIP_RET(hipMemcpyAsync(d->beam_score.p, score.data(), sizeof(float) * rows,
                               hipMemcpyHostToDevice, d->stream));
    float* lg = opt->trace_logits_dev ? opt->trace_logits_dev + (size_t)st * rows * d->V : nullptr;
    // (next_host: the step waits for the device, so h_cand is complete, and
    // reports a clamp of the fused o_proj as generate's steps do)
    const int rc = d->run_step(tok.data(), lg, dummy.data(), d->stream);
    if (rc == LLM_ERR_RANGE) range_rc = rc;
    else RET_IF(rc);
    steps = st + 1;
    const float* cs = reinterpret_cast<const float*>(d->h_cand.data());
    const int32_t* cp = d->h_cand.data() + 2 * rows;
    const int32_t* ct = d->h_cand.data() + 4 * rows;
    bool all_done = true;
    for (int s = 0; s < num_seqs; ++s) {
      const int b0 = s * W;
      int live = 0;
      for (int j = 0; j < K; ++j) {
        const float sc = cs[(size_t)s * K + j];
        const int32_t p = cp[(size_t)s * K + j], t = ct[(size_t)s * K + j];
        if (opt->trace_cand_score) opt->trace_cand_score[((size_t)st * num_seqs + s) * K + j] = sc;
        if (opt->trace_cand_parent) opt->trace_cand_parent[((size_t)st * num_seqs + s) * K + j] = p;
        if (opt->trace_cand_token) opt->trace_cand_token[((size_t)st * num_seqs + s) * K + j] = t;
        if (p < 0 || p >= W || t < 0 || t >= d->V)
          return fail(LLM_ERR_HIP, "llm_decoder_beam_search: the device returned a candidate out "
                                   "of range");
        if (t == opt->eos_token) {
          if (j < W && !done[s]) {
            BeamHyp h;
            h.ids = hist[b0 + p];
            h.ids.push_back(t);
            h.sum = sc;
            h.score = beam_final_score(sc, h.ids.size(), opt->length_penalty);
            finished[s].push_back(std::move(h));
          }
        } else if (live < W) {
          parent[live] = p;
          next_tok[live] = t;
          next_score[live] = sc;
          next_hist[live] = hist[b0 + p];
          next_hist[live].push_back(t);
          ++live;
        }
      }
      if (live != W)
        return fail(LLM_ERR_HIP, "llm_decoder_beam_search: fewer than beam_width live candidates");
      for (int w = 0; w < W; ++w) {
        hist[b0 + w].swap(next_hist[w]);
        tok[b0 + w] = next_tok[w];
        score[b0 + w] = next_score[w];
        if (opt->trace_live_parent)
          opt->trace_live_parent[((size_t)st * num_seqs + s) * W + w] = parent[w];
        if (opt->trace_live_token)
          opt->trace_live_token[((size_t)st * num_seqs + s) * W + w] = next_tok[w];
      }
      RET_IF(kv_cache_reorder(d->kv, b0, W, parent.data(), d->h_pos[b0]));
      if ((int)finished[s].size() >= W) done[s] = 1;
      all_done = all_done && done[s];
    }
    if (all_done) break;
  }
  if (opt->steps_run) *opt->steps_run = steps;
  // the live beams of the last step: their scores for a later inspection, and
  // the page table as the reorder left it
  LLM_HIP_RET(hipMemcpyAsync(d->beam_score.p, score.data(), sizeof(float) * rows,
                             hipMemcpyHostToDevice, d->stream));
  LLM_HIP_RET(hipMemcpyAsync(d->tokens.p, tok.data(), sizeof(int32_t) * rows,
                             hipMemcpyHostToDevice, d->stream));
  RET_IF(kv_cache_sync(d->kv, d->stream));
  LLM_HIP_RET(hipStreamSynchronize(d->stream));
  for (int s = 0; s < num_seqs; ++s) {
    std::vector<BeamHyp>& pool = finished[s];
    if (!done[s])
      for (int w = 0; w < W; ++w) {
        BeamHyp h;
        h.ids = hist[s * W + w];
        h.sum = score[s * W + w];
        h.score = beam_final_score(h.sum, h.ids.size(), opt->length_penalty);
        pool.push_back(std::move(h));
      }
    std::stable_sort(pool.begin(), pool.end(),
                     [](const BeamHyp& a, const BeamHyp& b) { return a.score > b.score; });
    for (int w = 0; w < W; ++w) {
      const BeamHyp& h = pool[w];
      int32_t* o = out_ids + ((size_t)s * W + w) * max_new;
      for (int i = 0; i < max_new; ++i) o[i] = i < (int)h.ids.size() ? h.ids[i] : -1;
      out_len[s * W + w] = (int32_t)h.ids.size();
      out_sum_logprob[s * W + w] = h.sum;
      out_score[s * W + w] = h.score;
    }
  }
  if (range_rc) return fail(LLM_ERR_RANGE, "llm_decoder_beam_search: the fused o_proj clamped a "
                                           "head product in at least one step; the results are "
                                           "complete, the ids after that step may differ");
  return LLM_OK;
}

// ---------------------------------------------------------------------------
// weight files (weights/README.md:26-38; raw little-endian .bin)
// ---------------------------------------------------------------------------
static int read_file(const std::string& path, std::vector<char>& buf, size_t expect) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) return fail(LLM_ERR_IO, "cannot open weight file: " + path);  // decoder_block.hpp:13-15
  const size_t size = (size_t)f.tellg();
  if (expect && size != expect)
    return fail(LLM_ERR_IO, path + ": expected " + std::to_string(expect) + " bytes, found " +
                                std::to_string(size));
  buf.resize(size);
  f.seekg(0);
  f.read(buf.data(), size);
  if (!f) return fail(LLM_ERR_IO, "failed to read from file: " + path);
  return LLM_OK;
}

static int write_file(const std::string& path, const void* p, size_t n) {
  std::ofstream f(path, std::ios::binary);
  if (!f) return fail(LLM_ERR_IO, "cannot create " + path);
  f.write(static_cast<const char*>(p), n);
  if (!f) return fail(LLM_ERR_IO, "write failed: " + path);
  return LLM_OK;
}

static uint16_t f32_to_f16_bits(float f) {
  const _Float16 h = (_Float16)f;
  uint16_t u;
  std::memcpy(&u, &h, 2);
  return u;
}

// fp32 directory (CUDADecoder::load_weights): embedding.bin [V][hid];
// layer_i/{ln1.bin, ln2.bin} gamma+beta; attn_wq/wk/wv/wo.bin [hid][hid];
// mlp_fc1.bin [hid][inter]; mlp_fc2.bin [inter][hid]; mlp_biases.bin [inter+hid].
struct Fp32Model {
  std::vector<float> emb, ln1, ln2, wqkv, wo, w1, w2, b1, b2;  // ln: [L][2][hid]
};

static int load_fp32_dir(const std::string& dir, int L, int hid, int inter, int V, Fp32Model& m) {
  std::vector<char> buf;
  auto rd = [&](const std::string& p, size_t n, float* dst) -> int {
    RET_IF(read_file(p, buf, n * 4));
    std::memcpy(dst, buf.data(), n * 4);
    return LLM_OK;
  };
  m.emb.resize((size_t)V * hid);
  RET_IF(rd(dir + "/embedding.bin", m.emb.size(), m.emb.data()));
  m.ln1.resize((size_t)L * 2 * hid); m.ln2.resize((size_t)L * 2 * hid);
  m.wqkv.resize((size_t)L * hid * 3 * hid); m.wo.resize((size_t)L * hid * hid);
  m.w1.resize((size_t)L * hid * inter); m.w2.resize((size_t)L * inter * hid);
  m.b1.resize((size_t)L * inter); m.b2.resize((size_t)L * hid);
  std::vector<float> tmp((size_t)hid * hid), bias(inter + hid);
  for (int l = 0; l < L; ++l) {
    const std::string p = dir + "/layer_" + std::to_string(l);
    RET_IF(rd(p + "/ln1.bin", 2 * hid, m.ln1.data() + (size_t)l * 2 * hid));
    RET_IF(rd(p + "/ln2.bin", 2 * hid, m.ln2.data() + (size_t)l * 2 * hid));
    const char* names[3] = {"/attn_wq.bin", "/attn_wk.bin", "/attn_wv.bin"};
    for (int j = 0; j < 3; ++j) {  // fuse q|k|v column blocks: Wqkv[k][j*hid + n]
      RET_IF(rd(p + names[j], (size_t)hid * hid, tmp.data()));
      float* dst = m.wqkv.data() + (size_t)l * hid * 3 * hid;
      for (int k = 0; k < hid; ++k)
        std::memcpy(dst + (size_t)k * 3 * hid + (size_t)j * hid, tmp.data() + (size_t)k * hid,
                    hid * 4);
    }
    RET_IF(rd(p + "/attn_wo.bin", (size_t)hid * hid, m.wo.data() + (size_t)l * hid * hid));
    RET_IF(rd(p + "/mlp_fc1.bin", (size_t)hid * inter, m.w1.data() + (size_t)l * hid * inter));
    RET_IF(rd(p + "/mlp_fc2.bin", (size_t)inter * hid, m.w2.data() + (size_t)l * inter * hid));
    RET_IF(rd(p + "/mlp_biases.bin", (size_t)inter + hid, bias.data()));
    std::memcpy(m.b1.data() + (size_t)l * inter, bias.data(), (size_t)inter * 4);
    std::memcpy(m.b2.data() + (size_t)l * hid, bias.data() + inter, (size_t)hid * 4);
  }
  return LLM_OK;
}

static void split_ln(const std::vector<float>& ln, int L, int hid, std::vector<float>& g,
                     std::vector<float>& b) {
  g.resize((size_t)L * hid);
  b.resize((size_t)L * hid);
  for (int l = 0; l < L; ++l) {
    std::memcpy(g.data() + (size_t)l * hid, ln.data() + (size_t)l * 2 * hid, hid * 4);
    std::memcpy(b.data() + (size_t)l * hid, ln.data() + (size_t)l * 2 * hid + hid, hid * 4);
  }
}

// Per-output-column int8 quantisation (int8_quant.cpp semantics, one scale per column).
static void quantize_cols(const float* w, int K, int N, int8_t* q, float* inv) {
  for (int n = 0; n < N; ++n) {
    float mn = w[n], mx = w[n];
    for (int k = 1; k < K; ++k) {
      mn = std::min(mn, w[(size_t)k * N + n]);
      mx = std::max(mx, w[(size_t)k * N + n]);
    }
    const float absmax = std::max(std::fabs(mn), std::fabs(mx));
    const float scale = 127.f / (absmax + 1e-6f);
    for (int k = 0; k < K; ++k) {
      int v = (int)std::round(w[(size_t)k * N + n] * scale);
      v = std::max(-128, std::min(127, v));
      q[(size_t)k * N + n] = (int8_t)v;
    }
    inv[n] = 1.0f / scale;
  }
}

extern "C" int llm_decoder_load_weights(llm_decoder* d, const char* dir) {
  LLM_REQUIRE(d && dir, "llm_decoder_load_weights: NULL");
  const int L = d->L, hid = d->hid, inter = d->inter, V = d->V;
  Fp32Model m;
  RET_IF(load_fp32_dir(dir, L, hid, inter, V, m));
  std::vector<float> g1, be1, g2, be2;
  split_ln(m.ln1, L, hid, g1, be1);
  split_ln(m.ln2, L, hid, g2, be2);
  std::vector<uint16_t> emb(m.emb.size());
  for (size_t i = 0; i < emb.size(); ++i) emb[i] = f32_to_f16_bits(m.emb[i]);
  if (d->wdtype == LLM_F16) {
    auto cvt = [](const std::vector<float>& s) {
      std::vector<uint16_t> o(s.size());
      for (size_t i = 0; i < s.size(); ++i) o[i] = f32_to_f16_bits(s[i]);
      return o;
    };
    auto qkv = cvt(m.wqkv), wo = cvt(m.wo), w1 = cvt(m.w1), w2 = cvt(m.w2);
    llm_f16_weights w{emb.data(), g1.data(), be1.data(), g2.data(), be2.data(), qkv.data(),
                      wo.data(), w1.data(), w2.data(), m.b1.data(), m.b2.data()};
    return llm_decoder_set_f16_weights(d, &w);
  }
  // INT8 decoder given fp32 weights: quantise on load
  std::vector<int8_t> qqkv(m.wqkv.size()), qo(m.wo.size()), q1(m.w1.size()), q2(m.w2.size());
  std::vector<float> sqkv((size_t)L * 3 * hid), so((size_t)L * hid), s1((size_t)L * inter),
      s2((size_t)L * hid);
  for (int l = 0; l < L; ++l) {
    quantize_cols(m.wqkv.data() + (size_t)l * hid * 3 * hid, hid, 3 * hid,
                  qqkv.data() + (size_t)l * hid * 3 * hid, sqkv.data() + (size_t)l * 3 * hid);
    quantize_cols(m.wo.data() + (size_t)l * hid * hid, hid, hid, qo.data() + (size_t)l * hid * hid,
                  so.data() + (size_t)l * hid);
    quantize_cols(m.w1.data() + (size_t)l * hid * inter, hid, inter,
                  q1.data() + (size_t)l * hid * inter, s1.data() + (size_t)l * inter);
    quantize_cols(m.w2.data() + (size_t)l * inter * hid, inter, hid,
                  q2.data() + (size_t)l * inter * hid, s2.data() + (size_t)l * hid);
  }
  llm_int8_weights w{emb.data(), g1.data(), be1.data(), g2.data(), be2.data(), qqkv.data(),
                     sqkv.data(), qo.data(), so.data(), q1.data(), s1.data(), m.b1.data(),
                     q2.data(), s2.data(), m.b2.data()};
  return llm_decoder_set_int8_weights(d, &w);
}

// INT8 directory written by llm_quantize_weights: embedding.f16 [V][hid] fp16;
// layer_i/{ln1.bin, ln2.bin (fp32 gamma+beta), attn_wqkv.i8 [hid][3hid],
// attn_wqkv.scale [3hid], attn_wo.i8/.scale, mlp_fc1.i8/.scale, mlp_fc2.i8/.scale,
// mlp_biases.bin [inter+hid] fp32}.
extern "C" int llm_quantize_weights(const char* fp32_dir, const char* int8_dir, int num_layers,
                                    int hidden_dim, int inter_dim, int vocab_size) {
  LLM_REQUIRE(fp32_dir && int8_dir && num_layers > 0 && hidden_dim > 0 && vocab_size > 0,
              "llm_quantize_weights: bad arguments");
  const int L = num_layers, hid = hidden_dim, inter = inter_dim > 0 ? inter_dim : 4 * hidden_dim;
  Fp32Model m;
  RET_IF(load_fp32_dir(fp32_dir, L, hid, inter, vocab_size, m));
  const std::string out = int8_dir;
  std::vector<uint16_t> emb(m.emb.size());
  for (size_t i = 0; i < emb.size(); ++i) emb[i] = f32_to_f16_bits(m.emb[i]);
  if (std::system(("mkdir -p '" + out + "'").c_str()) != 0)
    return fail(LLM_ERR_IO, "cannot create " + out);
  RET_IF(write_file(out + "/embedding.f16", emb.data(), emb.size() * 2));
  for (int l = 0; l < L; ++l) {
    const std::string p = out + "/layer_" + std::to_string(l);
    if (std::system(("mkdir -p '" + p + "'").c_str()) != 0)
      return fail(LLM_ERR_IO, "cannot create " + p);
    RET_IF(write_file(p + "/ln1.bin", m.ln1.data() + (size_t)l * 2 * hid, (size_t)2 * hid * 4));
    RET_IF(write_file(p + "/ln2.bin", m.ln2.data() + (size_t)l * 2 * hid, (size_t)2 * hid * 4));
    struct { const char* name; const float* w; int K, N; } mats[4] = {
        {"attn_wqkv", m.wqkv.data() + (size_t)l * hid * 3 * hid, hid, 3 * hid},
        {"attn_wo", m.wo.data() + (size_t)l * hid * hid, hid, hid},
        {"mlp_fc1", m.w1.data() + (size_t)l * hid * inter, hid, inter},
        {"mlp_fc2", m.w2.data() + (size_t)l * inter * hid, inter, hid}};
    for (auto& mt : mats) {
      std::vector<int8_t> q((size_t)mt.K * mt.N);
      std::vector<float> s(mt.N);
      quantize_cols(mt.w, mt.K, mt.N, q.data(), s.data());
      RET_IF(write_file(p + "/" + mt.name + ".i8", q.data(), q.size()));
      RET_IF(write_file(p + "/" + mt.name + ".scale", s.data(), s.size() * 4));
    }
    std::vector<float> bias(inter + hid);
    std::memcpy(bias.data(), m.b1.data() + (size_t)l * inter, (size_t)inter * 4);
    std::memcpy(bias.data() + inter, m.b2.data() + (size_t)l * hid, (size_t)hid * 4);
    RET_IF(write_file(p + "/mlp_biases.bin", bias.data(), bias.size() * 4));
  }
  return LLM_OK;
}

extern "C" int llm_decoder_load_quantized_weights(llm_decoder* d, const char* dir) {
  LLM_REQUIRE(d && dir, "llm_decoder_load_quantized_weights: NULL");
  LLM_REQUIRE(d->wdtype == LLM_I8, "llm_decoder_load_quantized_weights: decoder is not INT8");
  const int L = d->L, hid = d->hid, inter = d->inter, V = d->V;
  const std::string root = dir;
  std::vector<char> buf;
  std::vector<uint16_t> emb((size_t)V * hid);
  RET_IF(read_file(root + "/embedding.f16", buf, emb.size() * 2));
  std::memcpy(emb.data(), buf.data(), emb.size() * 2);
  std::vector<float> g1((size_t)L * hid), be1((size_t)L * hid), g2((size_t)L * hid), be2((size_t)L * hid);
  std::vector<int8_t> qqkv((size_t)L * hid * 3 * hid), qo((size_t)L * hid * hid),
      q1((size_t)L * hid * inter), q2((size_t)L * inter * hid);
  std::vector<float> sqkv((size_t)L * 3 * hid), so((size_t)L * hid), s1((size_t)L * inter),
      s2((size_t)L * hid), b1((size_t)L * inter), b2((size_t)L * hid);
  for (int l = 0; l < L; ++l) {
    const std::string p = root + "/layer_" + std::to_string(l);
    RET_IF(read_file(p + "/ln1.bin", buf, (size_t)2 * hid * 4));
    std::memcpy(g1.data() + (size_t)l * hid, buf.data(), hid * 4);
    std::memcpy(be1.data() + (size_t)l * hid, buf.data() + hid * 4, hid * 4);
    RET_IF(read_file(p + "/ln2.bin", buf, (size_t)2 * hid * 4));
    std::memcpy(g2.data() + (size_t)l * hid, buf.data(), hid * 4);
    std::memcpy(be2.data() + (size_t)l * hid, buf.data() + hid * 4, hid * 4);
    struct { const char* name; int8_t* q; float* s; int K, N; } mats[4] = {
        {"attn_wqkv", qqkv.data() + (size_t)l * hid * 3 * hid, sqkv.data() + (size_t)l * 3 * hid, hid, 3 * hid},
        {"attn_wo", qo.data() + (size_t)l * hid * hid, so.data() + (size_t)l * hid, hid, hid},
        {"mlp_fc1", q1.data() + (size_t)l * hid * inter, s1.data() + (size_t)l * inter, hid, inter},
        {"mlp_fc2", q2.data() + (size_t)l * inter * hid, s2.data() + (size_t)l * hid, inter, hid}};
    for (auto& mt : mats) {
      RET_IF(read_file(p + "/" + mt.name + ".i8", buf, (size_t)mt.K * mt.N));
      std::memcpy(mt.q, buf.data(), (size_t)mt.K * mt.N);
      RET_IF(read_file(p + "/" + mt.name + ".scale", buf, (size_t)mt.N * 4));
      std::memcpy(mt.s, buf.data(), (size_t)mt.N * 4);
    }
    RET_IF(read_file(p + "/mlp_biases.bin", buf, (size_t)(inter + hid) * 4));
    std::memcpy(b1.data() + (size_t)l * inter, buf.data(), (size_t)inter * 4);
    std::memcpy(b2.data() + (size_t)l * hid, buf.data() + (size_t)inter * 4, (size_t)hid * 4);
  }
  llm_int8_weights w{emb.data(), g1.data(), be1.data(), g2.data(), be2.data(), qqkv.data(),
                     sqkv.data(), qo.data(), so.data(), q1.data(), s1.data(), b1.data(),
                     q2.data(), s2.data(), b2.data()};
  return llm_decoder_set_int8_weights(d, &w);
}
