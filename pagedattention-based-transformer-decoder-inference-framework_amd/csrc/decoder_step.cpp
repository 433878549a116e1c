// Decoder runtime: the per-step host path.  One layer pass over a set of rows
// (layer_pre / layer_attn / layer_post and the launch forms they choose), the
// decode rows, the token choice, the step as it is captured into the hipGraph
// (enqueue_step) and replayed (run_step), and the fused o_proj's range report.
// Prefill passes (decoder_prefill.cpp) run the same layer pass on their rows.
#include <mutex>
#include <string>

#include "decoder_impl.hpp"

// f[1] = f[0], f[0] = 0 in one device atomic: the fused o_proj's range flag
// read and cleared (llm_decoder::report_range)
__global__ void take_flag_kernel(int* f) { f[1] = atomicExch(f, 0); }

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
    if (step_logprobs)  // a live request asked: every live row's, by constants of the step
      LLM_HIP_RET(launch_logprob_rows(lg, n, V, tokens.p + r0, LLM_MAX_TOP_LOGPROBS,
                                      sl_chosen.p + r0,
                                      sl_top_lp.p + (size_t)r0 * LLM_MAX_TOP_LOGPROBS,
                                      sl_top_id.p + (size_t)r0 * LLM_MAX_TOP_LOGPROBS, nullptr, st));
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
  if (serving && step_logprobs) {  // (complete with the synchronisation below)
    const size_t nt = (size_t)batch * LLM_MAX_TOP_LOGPROBS;
    LLM_HIP_RET(hipMemcpyAsync(hl_chosen.data(), sl_chosen.p, sizeof(float) * batch,
                               hipMemcpyDeviceToHost, st));
    LLM_HIP_RET(hipMemcpyAsync(hl_top_lp.data(), sl_top_lp.p, sizeof(float) * nt,
                               hipMemcpyDeviceToHost, st));
    LLM_HIP_RET(hipMemcpyAsync(hl_top_id.data(), sl_top_id.p, sizeof(int32_t) * nt,
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
