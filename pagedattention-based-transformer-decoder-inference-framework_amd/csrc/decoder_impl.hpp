// Decoder runtime, private header: the state and the few helpers that the
// decoder_*.cpp translation units share.  decoder.cpp's file comment says
// which unit holds what.  Included by those units only (never by a kernel
// file or by the bindings), so it opens namespace llm for them as decoder.cpp
// always did.
#pragma once

#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "gemm.hpp"
#include "kv_cache_impl.hpp"
#include "pa_decode.hpp"
#include "row_ops.hpp"
#include "serve_plan.hpp"

using namespace llm;

namespace llm {

// A device allocation owned by the decoder.  Named (not in an anonymous
// namespace): it is the type of llm_decoder's members, and every unit must
// see the same llm_decoder.  Hidden, like the two helpers at the end of this
// header: what was local to decoder.cpp stays out of the library's exports.
template <typename T>
struct __attribute__((visibility("hidden"))) DevBuf {
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

}  // namespace llm

#define RET_IF(x) do { int _rc = (x); if (_rc) return _rc; } while (0)

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

  // the captured step and the batch size it was captured for (run_step
  // captures again when that differs from `batch`)
  hipGraphExec_t graph = nullptr;
  int graph_batch{-1};
  // Something the captured step holds -- a kernel argument, a launch form, the
  // token choice -- changed: the next run_step captures again.  Every place
  // that invalidates the step calls this and says what changed.
  void drop_step_graph() { graph_batch = -1; }

  // activation taps (llm_decoder_set_taps): the int8 GEMM inputs and row scales
  // of every layer, copied out by the step for teacher-forced parity checks
  int8_t* tap_q = nullptr;
  float* tap_s = nullptr;
  int tap(int l, int stage, const Rows& R, int K, hipStream_t st);
  int layer_norm_into(WeightGemm& g, const Rows& R, const float* gamma, const float* beta,
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

  int layer_pre(int l, hipStream_t st, const Rows& R, const LnSource* emb = nullptr);
  int layer_attn(int l, hipStream_t st, const Rows& R);
  int attn_request(const Rows& R, pa_kv_view* view, PaRequest* rq, int l = 0);
  bool quant_prologue(const Rows& R) const;
  bool oproj_fusable(const Rows& R);
  bool wgm_quant_ok(const Rows& R);
  bool fc2_split(const Rows& R) const;
  int layer_post(int l, hipStream_t st, const Rows& R);
  int decode_rows(Rows* R, bool scratch_oproj = false);
  int next_tokens(const float* xr, int n, int r0, const int32_t* ctr, hipStream_t st,
                  int32_t* adv_pos = nullptr, int32_t* adv_ctx = nullptr);
  int enqueue_step(hipStream_t st);
  int run_step(const int32_t* tokens_host, float* logits_dev, int32_t* next_host, hipStream_t st);

  // chunked prefill (llm_decoder_prefill): buffers for one chunk of tokens
  static constexpr int kPrefillChunk = 512;
  DevBuf<float> px, pq, po, ph1, psa;
  DevBuf<uint8_t> pact, pws;
  DevBuf<int32_t> pmeta;  // [4][chunk]: pos, ctx, page-table row, token; then the
                          // packed passes' tile table [<= chunk][4]; then a
                          // scoring pass's targets [chunk]
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

  // Scoring (llm_decoder_score, decoder_score.cpp).  While `scoring` is set a
  // prefill pass ends with ONE launch_lm_head_logprobs over its packed rows
  // instead of a token choice: the targets (each packed row's next token of its
  // own sequence, seq[row]) are uploaded behind the pass's meta, and the m
  // values are copied back into out[row] at the target's position.
  struct ScoreRows {
    std::vector<const int32_t*> seq;  // per active row: its whole sequence
    std::vector<float*> out;          // per active row: its out_logprob row
  };
  const ScoreRows* scoring = nullptr;
  DevBuf<float> lp_ws, lp_val;  // the launch pair's partials; [kPrefillChunk] results
  // LLM_SCORE_FORM (read at create, scripts/bench_score.py's arms): 0 the fused
  // launch pair; 1 the unfused alternative (launch_lm_head writing the pass's
  // logits into lp_logits, then launch_logprob_rows with chosen = the targets);
  // 2 no LM head at all (the floor: the values are not computed)
  int score_form = 0;
  DevBuf<float> lp_logits;  // form 1 only: [kPrefillChunk][V]
  std::vector<float> h_lp;
  int score(const int32_t* toks, const int32_t* lens, int stride, int nseq, float* out);

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
    int top_logprobs = -1;  // llm_decoder_submit_logprobs' count; -1: did not ask
  };
  // Log-probabilities while serving: step_logprobs (a live request asks) puts
  // one launch_logprob_rows over all live rows (chosen = the step's ids, top_n
  // = LLM_MAX_TOP_LOGPROBS) behind the token choice; it is part of the step
  // graph's identity (serve_step drops the graph when it changes).  run_step
  // copies sl_* to hl_* before its closing synchronisation; hl_topn holds the
  // last step's events' counts (hl_n of them).
  bool step_logprobs = false;
  DevBuf<float> sl_chosen, sl_top_lp;
  DevBuf<int32_t> sl_top_id;
  std::vector<float> hl_chosen, hl_top_lp;
  std::vector<int32_t> hl_top_id, hl_topn;
  int hl_n = 0;
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

namespace llm {
#pragma GCC visibility push(hidden)

// decoder.cpp: the rows of a begin_* / generate / beam search start over
// (cleared pages, `batch` rows at start_pos), and the prompt check generate
// and the beam search share.
int reset_rows(llm_decoder* d, int batch, int start_pos);
int check_prompts(const std::string& who, const llm_decoder* d, const int32_t* prompts,
                  const int32_t* prompt_lens, int prompt_stride, int n, int* max_len);

#pragma GCC visibility pop
}  // namespace llm
