// Decoder runtime: beam search (llm_decoder.h: llm_decoder_beam_search), the
// device and page-table half.  The step graph runs in beam mode (its token
// choice is beam_select_rows' two launches, decoder_step.cpp next_tokens);
// between replays beam_plan.hpp ranks the hypotheses -- the finished pool,
// the done flags, the final sort are all its -- and this file uploads what it
// returns and re-parents the rows' pages (kv_cache_reorder).
#include <cmath>
#include <mutex>
#include <vector>

#include "beam_plan.hpp"
#include "decoder_impl.hpp"

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
      if (d->beam_mode) { d->beam_mode = false; d->drop_step_graph(); }
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
  d->drop_step_graph();

  BeamPlan plan;
  plan.begin(num_seqs, W, max_new, opt->eos_token, opt->length_penalty, d->V);
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
    for (int s = 0; s < num_seqs; ++s) {
      const int b0 = s * W;
      const size_t c0 = (size_t)s * K, tr = (size_t)st * num_seqs + s;
      for (int j = 0; j < K; ++j) {
        if (opt->trace_cand_score) opt->trace_cand_score[tr * K + j] = cs[c0 + j];
        if (opt->trace_cand_parent) opt->trace_cand_parent[tr * K + j] = cp[c0 + j];
        if (opt->trace_cand_token) opt->trace_cand_token[tr * K + j] = ct[c0 + j];
      }
      // the sequence's W live beams of the next step: tokens and scores into
      // the rows' uploads, the parents into the page tables
      if (const char* err = plan.step(s, cs + c0, cp + c0, ct + c0, parent.data(), tok.data() + b0,
                                      score.data() + b0))
        return fail(LLM_ERR_HIP, err);
      for (int w = 0; w < W; ++w) {
        if (opt->trace_live_parent) opt->trace_live_parent[tr * W + w] = parent[w];
        if (opt->trace_live_token) opt->trace_live_token[tr * W + w] = tok[b0 + w];
      }
      RET_IF(kv_cache_reorder(d->kv, b0, W, parent.data(), d->h_pos[b0]));
    }
    if (plan.all_done()) break;
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
  plan.finish(out_ids, out_len, out_sum_logprob, out_score);
  if (range_rc) return fail(LLM_ERR_RANGE, "llm_decoder_beam_search: the fused o_proj clamped a "
                                           "head product in at least one step; the results are "
                                           "complete, the ids after that step may differ");
  return LLM_OK;
}
