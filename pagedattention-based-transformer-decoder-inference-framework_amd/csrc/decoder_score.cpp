// Decoder runtime: teacher-forced scoring (llm_decoder_score).  The sequences
// go through the prefill passes of decoder_prefill.cpp in groups that fit the
// rows and the pool; with `scoring` set each pass ends with the LM head's
// log-softmax launch pair over its packed rows (prefill_pass), so one value per
// token comes back and no logits are materialised.
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "decoder_impl.hpp"

int llm_decoder::score(const int32_t* toks, const int32_t* lens, int stride, int nseq,
                       float* out) {
  LLM_REQUIRE(weights_ready, "llm_decoder_score: weights not loaded");
  LLM_REQUIRE(nseq >= 0 && stride >= 1, "llm_decoder_score: bad nseq / stride");
  if (nseq == 0) return LLM_OK;
  LLM_REQUIRE(toks && lens && out, "llm_decoder_score: NULL");
  // the page rule of a served request (serve_plan.hpp), for len - 1 positions
  ServeGeom geom;
  geom.max_rows = maxB;
  geom.num_pages = kv_cache_num_pages(kv);
  geom.pages_per_tile = L * H;
  geom.page_size = TS;
  geom.window = window;
  geom.max_seq_len = cfg.max_seq_len;
  std::vector<long long> need(nseq);
  for (int s = 0; s < nseq; ++s) {
    LLM_REQUIRE(lens[s] >= 1 && lens[s] <= stride,
                "llm_decoder_score: every sequence needs 1 .. stride tokens");
    LLM_REQUIRE(lens[s] - 1 < cfg.max_seq_len, "llm_decoder_score: sequence exceeds max_seq_len");
    for (int i = 0; i < lens[s]; ++i) {
      const int t = toks[(size_t)s * stride + i];
      LLM_REQUIRE(t >= 0 && t < V, "llm_decoder_score: token id out of range");
    }
    need[s] = serve_row_tiles(geom, lens[s] - 1) * geom.pages_per_tile;
    LLM_REQUIRE(need[s] <= geom.num_pages,
                "llm_decoder_score: a sequence needs " + std::to_string(need[s]) +
                    " pages, the pool has " + std::to_string(geom.num_pages));
  }
  if (score_form == 1 && V > 65536)
    return fail(LLM_ERR_UNSUPPORTED, "llm_decoder_score: LLM_SCORE_FORM=1 needs vocab_size <= 65536");
  if (!lp_val.p) {
    RET_IF(lp_val.alloc(kPrefillChunk));
    LLM_HIP_RET(hipMemset(lp_val.p, 0, sizeof(float) * kPrefillChunk));
    RET_IF(lp_ws.alloc(lm_head_logprobs_ws_floats(kPrefillChunk, V)));
    if (score_form == 1) RET_IF(lp_logits.alloc((size_t)kPrefillChunk * V));
  }
  h_lp.resize(kPrefillChunk);
  LLM_HIP_RET(hipStreamSynchronize(stream));

  struct Done {  // however the call ends: no rows active, the cache clear
    llm_decoder* d;
    ~Done() {
      d->scoring = nullptr;
      d->batch = 0;
      d->h_pos.assign(d->maxB, 0);
      (void)hipStreamSynchronize(d->stream);
      (void)kv_cache_clear(d->kv);
    }
  } done{this};

  for (int s0 = 0; s0 < nseq;) {
    // the group: sequences in order while a row is free and their needs fit
    int n = 0;
    long long pages = 0;
    while (s0 + n < nseq && n < maxB && pages + need[s0 + n] <= geom.num_pages) pages += need[s0 + n++];
    ScoreRows sr;
    std::vector<int32_t> plen(n);
    long long total = 0;
    for (int r = 0; r < n; ++r) {
      const int s = s0 + r;
      sr.seq.push_back(toks + (size_t)s * stride);
      sr.out.push_back(out + (size_t)s * stride);
      out[(size_t)s * stride] = 0.f;
      plen[r] = lens[s] - 1;
      total += plen[r];
    }
    if (total > 0) {
      RET_IF(reset_rows(this, n, 0));
      scoring = &sr;
      // prompt[:-1]-style: tokens[:len-1] of every row, as prefill_prompts chooses
      if (packed_prefill) {
        std::vector<int32_t> prow(n), ptok;
        for (int r = 0; r < n; ++r) {
          prow[r] = r;
          ptok.insert(ptok.end(), sr.seq[r], sr.seq[r] + plen[r]);
        }
        RET_IF(prefill_rows(prow.data(), ptok.data(), plen.data(), n, stream));
      } else {
        for (int r = 0; r < n; ++r)
          if (plen[r] > 0) RET_IF(prefill(r, sr.seq[r], plen[r], stream));
      }
      scoring = nullptr;
    }
    s0 += n;
  }
  return LLM_OK;
}

extern "C" int llm_decoder_score(llm_decoder* d, const int32_t* tokens, const int32_t* lens,
                                 int stride, int nseq, float* out_logprob) {
  LLM_REQUIRE(d, "llm_decoder_score: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  NOT_SERVING(d, "llm_decoder_score");
  return d->score(tokens, lens, stride, nseq, out_logprob);
}
