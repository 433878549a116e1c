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
//
// The runtime is one struct (decoder_impl.hpp: llm_decoder, the rows of a
// layer pass, the device buffers) worked on by one file per concern:
//   decoder.cpp          creation, the setters and getters, the synthetic
//                        begin_* entries, step / sync and generate
//   decoder_step.cpp     the layer pass, the step graph and run_step, the
//                        fused o_proj's range report
//   decoder_prefill.cpp  chunked and packed prefill
//   decoder_serve.cpp    continuous batching (serve_plan.hpp's decisions)
//   decoder_score.cpp    teacher-forced scoring through the prefill passes
//   decoder_beam.cpp     beam search (beam_plan.hpp's bookkeeping)
//   decoder_weights.cpp  weight upload, the weight-file reader, the quantiser
#include <algorithm>
#include <cmath>
#include <memory>
#include <mutex>
#include <random>
#include <string>
#include <vector>

#include "decoder_impl.hpp"

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
  d->score_form = env_int("LLM_SCORE_FORM", 0);  // (decoder_impl.hpp; 0: the fused launch pair)
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
  d->drop_step_graph();  // the step graph carries the scales as kernel arguments
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
  d->drop_step_graph();  // the step graph carries the table as a kernel argument
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
  d->drop_step_graph();  // the step graph carries the window as a kernel argument
  return LLM_OK;
}

extern "C" int llm_decoder_window(const llm_decoder* d) { return d ? d->window : -1; }

extern "C" void llm_decoder_destroy(llm_decoder* d) {
  if (!d) return;
  if (d->stream) (void)hipStreamSynchronize(d->stream);
  delete d;
}

extern "C" kv_cache* llm_decoder_kv(llm_decoder* d) { return d ? d->kv : nullptr; }

int llm::reset_rows(llm_decoder* d, int batch, int start_pos) {
  LLM_REQUIRE(batch > 0 && batch <= d->maxB, "decoder: batch must be in [1, max_batch]");
  RET_IF(kv_cache_clear(d->kv));
  d->batch = batch;
  if (d->row_group != 1) d->drop_step_graph();  // the captured attention launch used the beam group
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
  d->drop_step_graph();  // re-capture: the attention launch depends on row_group
  return LLM_OK;
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
  d->drop_step_graph();  // the step graph changes
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
  d->drop_step_graph();  // the step graph gains / loses the tap copies
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
int llm::check_prompts(const std::string& who, const llm_decoder* d, const int32_t* prompts,
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
      if (active) { d->temperature = 0.f; d->drop_step_graph(); }
    }
    ~SamplingGuard() {
      if (active) { d->temperature = t; d->drop_step_graph(); }
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
