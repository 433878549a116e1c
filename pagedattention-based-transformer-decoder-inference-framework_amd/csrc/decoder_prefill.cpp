// Decoder runtime: prefill.  A prompt's tokens are the rows of a layer pass
// (decoder_step.cpp) of up to kPrefillChunk tokens: one row's chunk per pass
// (llm_decoder_prefill), or segments of several rows packed into shared
// passes by prefill_pack.hpp (llm_decoder_prefill_rows).
#include <algorithm>
#include <mutex>
#include <vector>

#include "decoder_impl.hpp"
#include "prefill_pack.hpp"

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
    RET_IF(pmeta.alloc((size_t)9 * C));
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
  std::vector<int32_t> targets;
  if (scoring) {  // each packed row's next token of its own sequence (maybe the next pass's)
    for (const PassSeg& s : segs)
      for (int i = 0; i < s.len; ++i) targets.push_back(scoring->seq[s.row][s.p0 + i + 1]);
    LLM_HIP_RET(hipMemcpyAsync(pmeta.p + 8 * CAP, targets.data(), (size_t)m * sizeof(int32_t),
                               hipMemcpyHostToDevice, st));
  }
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
  if (scoring) {
    const int32_t* tg = pmeta.p + 8 * CAP;
    if (score_form == 0) {
      LLM_HIP_RET(launch_lm_head_logprobs(px.p, emb_packed.p, tg, lp_val.p, nullptr, m, V, hid,
                                          lp_ws.p, st));
    } else if (score_form == 1) {
      LLM_HIP_RET(launch_lm_head(px.p, emb_packed.p, lp_logits.p, m, V, hid, nullptr, nullptr, st));
      LLM_HIP_RET(launch_logprob_rows(lp_logits.p, m, V, tg, 0, lp_val.p, nullptr, nullptr, nullptr,
                                      st));
    }
    LLM_HIP_RET(hipMemcpyAsync(h_lp.data(), lp_val.p, (size_t)m * sizeof(float),
                               hipMemcpyDeviceToHost, st));
  }
  int q0 = 0;
  for (int j = 0; j < nseg; ++j) {
    const PassSeg& s = segs[j];
    const int last = q0 + s.len - 1;
    h_pos[s.row] = s.p0 + s.len;
    if (scoring) {  // (no token choice: the rows are released when the group is scored)
      q0 += s.len;
      continue;
    }
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
  if (scoring) {
    q0 = 0;
    for (const PassSeg& s : segs) {
      for (int i = 0; i < s.len; ++i) scoring->out[s.row][s.p0 + i + 1] = h_lp[q0 + i];
      q0 += s.len;
    }
  }
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
