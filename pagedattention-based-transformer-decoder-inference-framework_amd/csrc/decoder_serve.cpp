// Decoder runtime: continuous batching.  serve_plan.hpp decides who is
// admitted, which row a request holds and which row moves at a retirement;
// this file executes those decisions on the pages, the rows' device state and
// the step (decoder_step.cpp run_step).
#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "decoder_impl.hpp"

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
  // (prefix caching: the blocks the admissions evicted, before anything allocates)
  for (const ServeEvict& e : plan.evictions()) RET_IF(kv_cache_drop_pages(kv, e.pages.data()));
  plan.evictions().clear();
  if (na) {
    serve_dirty = true;
    // prompt[:-1] of the new rows, as prefill_prompts chooses -- behind the
    // cached blocks a row hit, whose pages it shares from here on
    std::vector<int32_t> prow, plen, ptok;
    for (int r = before; r < live; ++r) {
      const ServeReq& q = plan.row(r);
      const std::vector<int32_t>& p = requests.at(q.id).prompt;
      for (int k = 0; k < q.hit_blocks; ++k)
        RET_IF(kv_cache_attach_tile(kv, r, k, plan.index().block(q.blocks[k]).pages.data()));
      const int p0 = q.hit_blocks * TS, n = (int)p.size() - 1 - p0;
      h_pos[r] = p0;
      if (packed_prefill) {
        prow.push_back(r);
        plen.push_back(n);
        ptok.insert(ptok.end(), p.begin() + p0, p.begin() + p0 + n);
      } else if (n > 0) {
        RET_IF(prefill(r, p.data() + p0, n, stream));
      }
    }
    if (packed_prefill) RET_IF(prefill_rows(prow.data(), ptok.data(), plen.data(), na, stream));
    // (the tiles' pages are mapped on the host once the prefill has returned;
    // what reads them later runs behind it on the same stream)
    for (int r = before; r < live; ++r)
      RET_IF(plan.publish(r, [&](int tile, int32_t* pages) {
        return kv_cache_hold_tile(kv, r, tile, pages);
      }));
  }
  if (serve_dirty) RET_IF(serve_upload());
  bool ask = false;
  for (int r = 0; r < live; ++r) {
    const ServeRequest& rq = requests.at(plan.row(r).id);
    hs_tok[r] = rq.feed;
    hl_topn[r] = rq.top_logprobs;
    ask = ask || rq.top_logprobs >= 0;
  }
  hl_n = live;
  if (ask != step_logprobs) {
    step_logprobs = ask;
    drop_step_graph();  // the logprob_rows launch joins / leaves the step
  }
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

static int serve_begin(llm_decoder* d, bool prefix_cache) {
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
  if (prefix_cache && d->window > 0)
    return fail(LLM_ERR_UNSUPPORTED, "llm_decoder_serve_begin_opts: prefix_cache with a sliding "
                                     "window (its page release does not compose with held "
                                     "blocks)");
  LLM_HIP_RET(hipStreamSynchronize(d->stream));
  RET_IF(kv_cache_clear(d->kv));  // (every page count is reset: plan.begin forgets the blocks)
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
  if (!d->sl_chosen.p) {
    RET_IF(d->sl_chosen.alloc(B));
    RET_IF(d->sl_top_lp.alloc(B * LLM_MAX_TOP_LOGPROBS));
    RET_IF(d->sl_top_id.alloc(B * LLM_MAX_TOP_LOGPROBS));
  }
  d->hl_chosen.assign(B, 0.f); d->hl_top_lp.assign(B * LLM_MAX_TOP_LOGPROBS, 0.f);
  d->hl_top_id.assign(B * LLM_MAX_TOP_LOGPROBS, 0); d->hl_topn.assign(B, -1);
  d->hl_n = 0;
  d->step_logprobs = false;
  ServeGeom geom;
  geom.max_rows = d->maxB;
  geom.num_pages = kv_cache_num_pages(d->kv);
  geom.pages_per_tile = d->L * d->H;
  geom.page_size = d->TS;
  geom.window = d->window;
  geom.max_seq_len = d->cfg.max_seq_len;
  d->plan.begin(geom, prefix_cache);
  d->requests.clear();
  d->serve_dirty = false;
  d->serving = true;
  d->drop_step_graph();  // the step's token choice becomes sample_rows_each
  return LLM_OK;
}

extern "C" int llm_decoder_serve_begin(llm_decoder* d) {
  LLM_REQUIRE(d, "llm_decoder_serve_begin: NULL");
  return serve_begin(d, false);
}

extern "C" int llm_decoder_serve_begin_opts(llm_decoder* d, const llm_serve_options* opt) {
  LLM_REQUIRE(d && opt, "llm_decoder_serve_begin_opts: NULL");
  LLM_REQUIRE(opt->prefix_cache == 0 || opt->prefix_cache == 1,
              "llm_decoder_serve_begin_opts: prefix_cache must be 0 or 1");
  return serve_begin(d, opt->prefix_cache == 1);
}

extern "C" int llm_decoder_serve_prefix_stats(const llm_decoder* d, llm_prefix_stats* out) {
  LLM_REQUIRE(d && out, "llm_decoder_serve_prefix_stats: NULL");
  std::lock_guard<std::mutex> g(const_cast<llm_decoder*>(d)->mu);
  const ServePrefixStats& s = d->plan.prefix_stats();
  out->positions_due = s.due;
  out->positions_hit = s.hit;
  out->cached_blocks = d->plan.index().cached_blocks();
  out->idle_pages = d->plan.idle_pages();
  out->evicted_blocks = s.evicted;
  out->deferrals = s.deferrals;
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
  d->step_logprobs = false;
  d->hl_n = 0;
  d->drop_step_graph();
  d->batch = 0;
  d->h_pos.assign(d->maxB, 0);
  return kv_cache_clear(d->kv);
}

static int submit_request(llm_decoder* d, const int32_t* prompt, int n,
                          const llm_request_options* opt, int top_logprobs, long long* id) {
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
  // (the plan reads the prompt where the request keeps it: a node of
  // `requests` stays where it is until the request is erased)
  std::vector<int32_t> copy(prompt, prompt + n);
  const long long rid = d->plan.submit(n, opt->max_new_tokens, copy.data());
  llm_decoder::ServeRequest& rq = d->requests[rid];
  rq.prompt = std::move(copy);
  rq.opt = *opt;
  rq.feed = prompt[n - 1];
  rq.top_logprobs = top_logprobs;
  *id = rid;
  return LLM_OK;
}

extern "C" int llm_decoder_submit(llm_decoder* d, const int32_t* prompt, int n,
                                  const llm_request_options* opt, long long* id) {
  LLM_REQUIRE(d && prompt && opt && id, "llm_decoder_submit: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  return submit_request(d, prompt, n, opt, -1, id);
}

extern "C" int llm_decoder_submit_logprobs(llm_decoder* d, const int32_t* prompt, int n,
                                           const llm_request_options* opt, int top_logprobs,
                                           long long* id) {
  LLM_REQUIRE(d && prompt && opt && id, "llm_decoder_submit_logprobs: NULL");
  LLM_REQUIRE(top_logprobs >= 0 && top_logprobs <= LLM_MAX_TOP_LOGPROBS,
              "llm_decoder_submit_logprobs: top_logprobs must be in [0, 8]");
  std::lock_guard<std::mutex> g(d->mu);
  LLM_REQUIRE(d->V >= LLM_MAX_TOP_LOGPROBS,
              "llm_decoder_submit_logprobs: vocab_size < 8 (the step takes the rows' top 8)");
  return submit_request(d, prompt, n, opt, top_logprobs, id);
}

extern "C" int llm_decoder_serve_logprobs(llm_decoder* d, float* chosen_lp, float* top_lp,
                                          int32_t* top_id, int32_t* top_n) {
  LLM_REQUIRE(d, "llm_decoder_serve_logprobs: NULL");
  std::lock_guard<std::mutex> g(d->mu);
  LLM_REQUIRE(d->serving, "llm_decoder_serve_logprobs: not serving");
  const size_t n = (size_t)d->hl_n, nt = n * LLM_MAX_TOP_LOGPROBS;
  if (chosen_lp) std::copy(d->hl_chosen.begin(), d->hl_chosen.begin() + n, chosen_lp);
  if (top_lp) std::copy(d->hl_top_lp.begin(), d->hl_top_lp.begin() + nt, top_lp);
  if (top_id) std::copy(d->hl_top_id.begin(), d->hl_top_id.begin() + nt, top_id);
  if (top_n) std::copy(d->hl_topn.begin(), d->hl_topn.begin() + n, top_n);
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
