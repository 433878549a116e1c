// pybind11 module `llm_decoder` — the reference's Python surface
// (src/bindings.cpp:3-35, include/bindings.hpp:1-10) over the C ABI of
// libllm_decoder_hip.so (include/llm_decoder.h).
//
//   CUDADecoder(num_layers, num_heads, head_dim, hidden_dim, vocab_size, max_seq_len)
//       .load_weights(path) / .generate(...)                       bindings.cpp:5-15
//   INT8Decoder(same)
//       .load_quantized_weights(path) / .quantize_weights(src, dst) / .generate(...)
//                                                                  bindings.cpp:18-29
// generate accepts both call conventions in the tree:
//   generate(input_ids, max_len, temperature=1.0) -> list           (bindings.cpp:8-15)
//   generate(input_ids, output_ids, max_gen_len, temperature=1.0)   (api/router.py:23,
//       web/app.py:23, cli/chat_cli.py:24 — fills output_ids in place)
// and both return / fill prompt + generated ids (cuda_decoder.cu:49,59).
// Both decoders take a keyword kv_dtype ("float16" by default; "fp8" /
// "float8_e4m3fn": LLM_FP8 KV pages with per-layer scales, set_kv_scales) and
// have a read-only prefill_kernel ("mfma" / "decode": llm_decoder_prefill_kernel).
// Additions: generate_batch, beam_search / beam_search_batch
// (llm_decoder_beam_search: [(ids, score), ...] per prompt, best first; what
// api/router.py's stream_chat_beam loops greedy generate for), the module-level
// beam_select (beam_select_rows), set_weights (host numpy arrays), low-level
// begin_synthetic / step for the bench, prefill(row, tokens) and its packed
// form prefill_batch(rows, token_lists) (llm_decoder_prefill_rows) with the
// read/write packed_prefill switch that generate* / beam_search* follow
// (llm_decoder_set_packed_prefill, default False), continuous batching
// (serve_begin / submit / cancel / serve_step / serve_stats / serve_end over
// llm_decoder_serve_*, and generate_many, the serve loop over any number of
// prompts), PageTable / KVTileCache classes with
// the kv_cache/ API names (page_table.hpp:5-37, kv_tile_cache.hpp:9-41) and
// paged_attention() over raw device pointers.
//
// Errors: any non-zero C-ABI status raises RuntimeError with llm_last_error().
// The GIL is released around device work; each decoder serialises its own
// calls with an internal mutex (KVTileCache's std::mutex, kv_tile_cache.hpp:73).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "llm_decoder.h"

namespace py = pybind11;

namespace {

void check(int rc) {
  if (rc != LLM_OK) throw std::runtime_error(std::string("llm_decoder: ") + llm_last_error());
}

template <typename T>
py::array_t<T, py::array::c_style | py::array::forcecast> arr(const py::dict& w, const char* k,
                                                                size_t expect) {
  if (!w.contains(k)) throw std::invalid_argument(std::string("set_weights: missing '") + k + "'");
  auto a = py::array_t<T, py::array::c_style | py::array::forcecast>::ensure(w[k]);
  if (!a) throw std::invalid_argument(std::string("set_weights: bad array '") + k + "'");
  if ((size_t)a.size() != expect)
    throw std::invalid_argument(std::string("set_weights: '") + k + "' has " +
                                std::to_string(a.size()) + " elements, expected " +
                                std::to_string(expect));
  return a;
}

class Decoder {
 public:
  Decoder(int weight_dtype, int num_layers, int num_heads, int head_dim, int hidden_dim,
          int vocab_size, int max_seq_len, int max_batch, int page_size, int inter_dim,
          float attn_scale, long long num_pages, const std::string& kv_dtype) {
    const int kvt = kv_dtype == "float16" || kv_dtype == "half" || kv_dtype == "fp16" ? LLM_F16
                    : kv_dtype == "fp8" || kv_dtype == "float8_e4m3fn"                  ? LLM_FP8
                                                                                        : -1;
    if (kvt < 0)
      throw std::invalid_argument("kv_dtype must be 'float16' or 'fp8' / 'float8_e4m3fn'");
    llm_decoder_config c{};
    c.num_layers = num_layers; c.num_heads = num_heads; c.head_dim = head_dim;
    c.hidden_dim = hidden_dim; c.vocab_size = vocab_size; c.max_seq_len = max_seq_len;
    c.inter_dim = inter_dim; c.page_size = page_size; c.weight_dtype = weight_dtype;
    c.max_batch = max_batch; c.attn_scale = attn_scale; c.num_pages = num_pages;
    check(llm_decoder_create_kv(&c, kvt, &d_));
    cfg_ = c;
    if (cfg_.inter_dim <= 0) cfg_.inter_dim = 4 * hidden_dim;
  }
  ~Decoder() { llm_decoder_destroy(d_); }
  Decoder(const Decoder&) = delete;
  Decoder& operator=(const Decoder&) = delete;

  void load_weights(const std::string& path) {
    py::gil_scoped_release nogil;
    check(llm_decoder_load_weights(d_, path.c_str()));
  }
  void load_quantized_weights(const std::string& path) {
    py::gil_scoped_release nogil;
    check(llm_decoder_load_quantized_weights(d_, path.c_str()));
  }
  void quantize_weights(const std::string& src, const std::string& dst) {
    py::gil_scoped_release nogil;
    check(llm_quantize_weights(src.c_str(), dst.c_str(), cfg_.num_layers, cfg_.hidden_dim,
                               cfg_.inter_dim, cfg_.vocab_size));
  }

  void set_weights(const py::dict& w) {
    const size_t L = cfg_.num_layers, hid = cfg_.hidden_dim, inter = cfg_.inter_dim,
                 V = cfg_.vocab_size;
    auto emb = arr<uint16_t>(w, "emb", V * hid);
    auto ln1_g = arr<float>(w, "ln1_g", L * hid), ln1_b = arr<float>(w, "ln1_b", L * hid);
    auto ln2_g = arr<float>(w, "ln2_g", L * hid), ln2_b = arr<float>(w, "ln2_b", L * hid);
    auto b1 = arr<float>(w, "b1", L * inter), b2 = arr<float>(w, "b2", L * hid);
    if (cfg_.weight_dtype == LLM_I8) {
      auto wqkv = arr<int8_t>(w, "wqkv", L * hid * 3 * hid), wo = arr<int8_t>(w, "wo", L * hid * hid);
      auto w1 = arr<int8_t>(w, "w1", L * hid * inter), w2 = arr<int8_t>(w, "w2", L * inter * hid);
      auto sq = arr<float>(w, "sw_qkv", L * 3 * hid), so = arr<float>(w, "sw_o", L * hid);
      auto s1 = arr<float>(w, "sw1", L * inter), s2 = arr<float>(w, "sw2", L * hid);
      llm_int8_weights x{emb.data(), ln1_g.data(), ln1_b.data(), ln2_g.data(), ln2_b.data(),
                         wqkv.data(), sq.data(), wo.data(), so.data(), w1.data(), s1.data(),
                         b1.data(), w2.data(), s2.data(), b2.data()};
      py::gil_scoped_release nogil;
      check(llm_decoder_set_int8_weights(d_, &x));
    } else {
      auto wqkv = arr<uint16_t>(w, "wqkv", L * hid * 3 * hid), wo = arr<uint16_t>(w, "wo", L * hid * hid);
      auto w1 = arr<uint16_t>(w, "w1", L * hid * inter), w2 = arr<uint16_t>(w, "w2", L * inter * hid);
      llm_f16_weights x{emb.data(), ln1_g.data(), ln1_b.data(), ln2_g.data(), ln2_b.data(),
                        wqkv.data(), wo.data(), w1.data(), w2.data(), b1.data(), b2.data()};
      py::gil_scoped_release nogil;
      check(llm_decoder_set_f16_weights(d_, &x));
    }
  }

  std::vector<std::vector<int>> generate_batch(const std::vector<std::vector<int>>& prompts,
                                               int max_gen_len, float temperature) {
    const int B = (int)prompts.size();
    if (B == 0) return {};
    size_t stride = 1;
    for (auto& p : prompts) stride = std::max(stride, p.size());
    std::vector<int32_t> flat((size_t)B * stride, 0), lens(B);
    for (int b = 0; b < B; ++b) {
      lens[b] = (int32_t)prompts[b].size();
      std::copy(prompts[b].begin(), prompts[b].end(), flat.begin() + (size_t)b * stride);
    }
    std::vector<int32_t> out((size_t)B * std::max(max_gen_len, 0));
    {
      py::gil_scoped_release nogil;
      check(llm_decoder_generate(d_, flat.data(), lens.data(), (int)stride, B, max_gen_len,
                                 temperature, out.data()));
    }
    std::vector<std::vector<int>> res(B);
    for (int b = 0; b < B; ++b) {
      res[b] = prompts[b];  // output_ids = input_ids (cuda_decoder.cu:49)
      for (int g = 0; g < max_gen_len; ++g) res[b].push_back(out[(size_t)b * max_gen_len + g]);
    }
    return res;
  }

  py::object generate(py::args args, py::kwargs kwargs) {
    // form 1: (input_ids, max_len[, temperature]) -> list
    // form 2: (input_ids, output_ids: list, max_gen_len[, temperature]) -> None
    std::vector<int> input;
    py::object out_list = py::none();
    int max_len = -1;
    float temperature = 1.0f;
    size_t i = 0;
    if (args.size() > i) input = args[i++].cast<std::vector<int>>();
    else if (kwargs.contains("input_ids")) input = kwargs["input_ids"].cast<std::vector<int>>();
    else throw std::invalid_argument("generate: input_ids is required");
    if (args.size() > i && py::isinstance<py::list>(args[i])) out_list = args[i++];
    else if (kwargs.contains("output_ids")) out_list = kwargs["output_ids"];
    if (args.size() > i) max_len = args[i++].cast<int>();
    for (const char* k : {"max_gen_len", "max_len", "max_tokens"})
      if (kwargs.contains(k)) max_len = kwargs[k].cast<int>();
    if (args.size() > i) temperature = args[i++].cast<float>();
    if (kwargs.contains("temperature")) temperature = kwargs["temperature"].cast<float>();
    if (max_len < 0) throw std::invalid_argument("generate: max_gen_len is required");
    if (input.empty()) throw std::invalid_argument("generate: input_ids must not be empty");
    auto res = generate_batch({input}, max_len, temperature)[0];
    if (!out_list.is_none()) {
      py::list l = out_list.cast<py::list>();
      while (py::len(l) > 0) l.attr("pop")();
      for (int t : res) l.append(t);
      return py::none();
    }
    return py::cast(res);
  }

  // llm_decoder_beam_search over a batch of prompts: per prompt the beam_width
  // hypotheses [(ids, score), ...], best first (ids: the generated tokens, EOS
  // included).  return_trace: (results, trace) with trace a dict of numpy
  // arrays -- cand_parent / cand_token / cand_score [steps][num_seqs][2W],
  // live_parent / live_token [steps][num_seqs][W], sum_logprob / length
  // [num_seqs][W], steps -- and, when trace_logits_ptr names a device buffer of
  // [max_new_tokens][num_seqs * W][V] floats, every step's logits there.
  py::object beam_search_batch(const std::vector<std::vector<int>>& prompts, int beam_width,
                               int max_new_tokens, int eos_token_id, float length_penalty,
                               bool return_trace, uintptr_t trace_logits_ptr) {
    const int S = (int)prompts.size();
    if (S == 0) return py::list();
    if (beam_width < 1 || beam_width > 4)
      throw std::invalid_argument("beam_search: beam_width must be in [1, 4]");
    if (max_new_tokens < 1) throw std::invalid_argument("beam_search: max_new_tokens must be >= 1");
    const int W = beam_width, K = 2 * W;
    size_t stride = 1;
    for (auto& p : prompts) stride = std::max(stride, p.size());
    std::vector<int32_t> flat((size_t)S * stride, 0), lens(S);
    for (int s = 0; s < S; ++s) {
      lens[s] = (int32_t)prompts[s].size();
      std::copy(prompts[s].begin(), prompts[s].end(), flat.begin() + (size_t)s * stride);
    }
    const size_t T = (size_t)max_new_tokens;
    std::vector<int32_t> ids((size_t)S * W * T), len((size_t)S * W);
    std::vector<float> sum((size_t)S * W), score((size_t)S * W);
    std::vector<int32_t> cp, ct, lp, lt;
    std::vector<float> cs;
    int steps = 0;
    llm_beam_options o{};
    o.beam_width = W; o.max_new_tokens = max_new_tokens; o.eos_token = eos_token_id;
    o.length_penalty = length_penalty;
    o.steps_run = &steps;
    if (return_trace) {
      cp.assign(T * S * K, -1); ct.assign(T * S * K, -1); cs.assign(T * S * K, 0.f);
      lp.assign(T * S * W, -1); lt.assign(T * S * W, -1);
      o.trace_cand_parent = cp.data(); o.trace_cand_token = ct.data();
      o.trace_cand_score = cs.data();
      o.trace_live_parent = lp.data(); o.trace_live_token = lt.data();
      o.trace_logits_dev = reinterpret_cast<float*>(trace_logits_ptr);
    }
    {
      py::gil_scoped_release nogil;
      check(llm_decoder_beam_search(d_, flat.data(), lens.data(), (int)stride, S, &o, ids.data(),
                                    len.data(), sum.data(), score.data()));
    }
    py::list res;
    for (int s = 0; s < S; ++s) {
      py::list hyps;
      for (int w = 0; w < W; ++w) {
        const int32_t* p = ids.data() + ((size_t)s * W + w) * T;
        hyps.append(py::make_tuple(std::vector<int>(p, p + len[s * W + w]), score[s * W + w]));
      }
      res.append(hyps);
    }
    if (!return_trace) return res;
    auto a3 = [&](auto& v, int n) {
      using E = typename std::remove_reference_t<decltype(v)>::value_type;
      py::array_t<E> a({(py::ssize_t)steps, (py::ssize_t)S, (py::ssize_t)n});
      std::copy(v.begin(), v.begin() + (size_t)steps * S * n, a.mutable_data());
      return a;
    };
    auto a2 = [&](auto& v) {
      using E = typename std::remove_reference_t<decltype(v)>::value_type;
      py::array_t<E> a({(py::ssize_t)S, (py::ssize_t)W});
      std::copy(v.begin(), v.end(), a.mutable_data());
      return a;
    };
    py::dict tr;
    tr["cand_parent"] = a3(cp, K); tr["cand_token"] = a3(ct, K); tr["cand_score"] = a3(cs, K);
    tr["live_parent"] = a3(lp, W); tr["live_token"] = a3(lt, W);
    tr["sum_logprob"] = a2(sum); tr["length"] = a2(len); tr["score"] = a2(score);
    tr["steps"] = steps;
    return py::make_tuple(res, tr);
  }
  py::object beam_search(const std::vector<int>& input_ids, int beam_width, int max_new_tokens,
                         int eos_token_id, float length_penalty, bool return_trace,
                         uintptr_t trace_logits_ptr) {
    if (input_ids.empty()) throw std::invalid_argument("beam_search: input_ids must not be empty");
    py::object r = beam_search_batch({input_ids}, beam_width, max_new_tokens, eos_token_id,
                                     length_penalty, return_trace, trace_logits_ptr);
    if (!return_trace) return r.cast<py::list>()[0];
    py::tuple t = r.cast<py::tuple>();
    return py::make_tuple(t[0].cast<py::list>()[0], t[1]);
  }

  void begin_synthetic(int batch, int context_len, uint64_t seed, bool shuffle) {
    py::gil_scoped_release nogil;
    check(llm_decoder_begin_synthetic(d_, batch, context_len, seed, shuffle ? 1 : 0));
  }

  void prefill(int row, const std::vector<int32_t>& tokens) {
    py::gil_scoped_release nogil;
    check(llm_decoder_prefill(d_, row, tokens.data(), (int)tokens.size()));
  }

  // llm_decoder_prefill_rows: the prompts of several rows through shared passes
  void prefill_batch(const std::vector<int32_t>& rows,
                     const std::vector<std::vector<int32_t>>& tokens) {
    if (rows.size() != tokens.size())
      throw std::invalid_argument("prefill_batch: one token list per row");
    std::vector<int32_t> lens, flat;
    for (const auto& t : tokens) {
      lens.push_back((int32_t)t.size());
      flat.insert(flat.end(), t.begin(), t.end());
    }
    py::gil_scoped_release nogil;
    check(llm_decoder_prefill_rows(d_, rows.data(), flat.data(), lens.data(), (int)rows.size()));
  }
  bool packed_prefill() const { return llm_decoder_packed_prefill(d_) == 1; }
  void set_packed_prefill(bool on) { check(llm_decoder_set_packed_prefill(d_, on ? 1 : 0)); }

  void set_sampling(float temperature, int top_k, float top_p, uint64_t seed) {
    py::gil_scoped_release nogil;
    check(llm_decoder_set_sampling(d_, temperature, top_k, top_p, seed));
  }

  // Continuous batching (llm_decoder_serve_*): submit at any time, one
  // serve_step = admissions + their prefill + one decode step of all live rows
  // prefix_cache: prompt blocks are shared between the session's requests
  // (llm_decoder_serve_begin_opts)
  void serve_begin(bool prefix_cache) {
    py::gil_scoped_release nogil;
    const llm_serve_options o{prefix_cache ? 1 : 0};
    check(llm_decoder_serve_begin_opts(d_, &o));
  }
  void serve_end() {
    py::gil_scoped_release nogil;
    check(llm_decoder_serve_end(d_));
  }
  // logprobs: None (nothing asked), or 0 .. 8: the chosen token's
  // log-probability plus that many top alternatives (serve_logprobs)
  long long submit(const std::vector<int32_t>& tokens, int max_new_tokens, int eos_token_id,
                   float temperature, int top_k, float top_p, uint64_t seed, py::object logprobs) {
    llm_request_options o{max_new_tokens, eos_token_id, temperature, top_k, top_p, seed};
    long long id = -1;
    if (logprobs.is_none()) check(llm_decoder_submit(d_, tokens.data(), (int)tokens.size(), &o, &id));
    else
      check(llm_decoder_submit_logprobs(d_, tokens.data(), (int)tokens.size(), &o,
                                        logprobs.cast<int>(), &id));
    return id;
  }
  // The last serve_step's log-probabilities, one entry per event in event order:
  // (logprob of the chosen token, [(id, logprob), ...] of the request's top
  // alternatives), or None for a request that did not ask.
  py::list serve_logprobs() {
    const size_t B = (size_t)std::max(cfg_.max_batch, 1);
    std::vector<float> clp(B), tlp(B * LLM_MAX_TOP_LOGPROBS);
    std::vector<int32_t> tid(B * LLM_MAX_TOP_LOGPROBS), tn(B, -2);
    check(llm_decoder_serve_logprobs(d_, clp.data(), tlp.data(), tid.data(), tn.data()));
    py::list res;
    for (size_t r = 0; r < B && tn[r] != -2; ++r) res.append(logprob_entry(clp, tlp, tid, tn, r));
    return res;
  }
  static py::object logprob_entry(const std::vector<float>& clp, const std::vector<float>& tlp,
                                  const std::vector<int32_t>& tid, const std::vector<int32_t>& tn,
                                  size_t r) {
    if (tn[r] < 0) return py::none();
    py::list top;
    for (int j = 0; j < tn[r]; ++j)
      top.append(py::make_tuple(tid[r * LLM_MAX_TOP_LOGPROBS + j], tlp[r * LLM_MAX_TOP_LOGPROBS + j]));
    return py::make_tuple(clp[r], top);
  }
  // Teacher-forced scoring (llm_decoder_score): per sequence a float32 array of
  // len - 1 values, entry i - 1 = log p(seq[i] | seq[:i]).
  py::list score(const std::vector<std::vector<int32_t>>& sequences) {
    const int n = (int)sequences.size();
    size_t stride = 1;
    for (const auto& q : sequences) stride = std::max(stride, q.size());
    std::vector<int32_t> toks((size_t)n * stride, 0), lens(n);
    for (int s = 0; s < n; ++s) {
      lens[s] = (int)sequences[s].size();
      std::copy(sequences[s].begin(), sequences[s].end(), toks.begin() + (size_t)s * stride);
    }
    std::vector<float> out((size_t)n * stride, 0.f);
    {
      py::gil_scoped_release nogil;
      check(llm_decoder_score(d_, toks.data(), lens.data(), (int)stride, n, out.data()));
    }
    py::list res;
    for (int s = 0; s < n; ++s) {
      py::array_t<float> a((py::ssize_t)(lens[s] - 1));
      std::copy(out.begin() + (size_t)s * stride + 1, out.begin() + (size_t)s * stride + lens[s],
                a.mutable_data());
      res.append(a);
    }
    return res;
  }
  void cancel(long long id) { check(llm_decoder_cancel(d_, id)); }
  // [(id, token, index, row, finish), ...] of the step's live rows, ascending
  // row; logits_ptr: device [max_batch][V] floats for the step's logits (0: none)
  py::list serve_step(uintptr_t logits_ptr) {
    std::vector<llm_serve_event> ev((size_t)std::max(cfg_.max_batch, 1));
    int n = 0;
    {
      py::gil_scoped_release nogil;
      check(llm_decoder_serve_step(d_, reinterpret_cast<float*>(logits_ptr), ev.data(),
                                   (int)ev.size(), &n));
    }
    py::list res;
    for (int i = 0; i < n; ++i)
      res.append(py::make_tuple(ev[i].id, ev[i].token, ev[i].index, ev[i].row, ev[i].finish));
    return res;
  }
  // {live, waiting, committed_pages, graph_instantiations}
  py::dict serve_stats() const {
    int live = 0, waiting = 0;
    long long committed = 0, inst = 0;
    check(llm_decoder_serve_stats(d_, &live, &waiting, &committed, &inst));
    py::dict s;
    s["live"] = live; s["waiting"] = waiting; s["committed_pages"] = committed;
    s["graph_instantiations"] = inst;
    return s;
  }
  // {positions_due, positions_hit, cached_blocks, idle_pages, evicted_blocks,
  // deferrals} of the session's prefix cache (zeros without one)
  py::dict serve_prefix_stats() const {
    llm_prefix_stats p{};
    check(llm_decoder_serve_prefix_stats(d_, &p));
    py::dict s;
    s["positions_due"] = p.positions_due; s["positions_hit"] = p.positions_hit;
    s["cached_blocks"] = p.cached_blocks; s["idle_pages"] = p.idle_pages;
    s["evicted_blocks"] = p.evicted_blocks; s["deferrals"] = p.deferrals;
    return s;
  }
  // Any number of prompts through the serve loop: the generated ids per prompt
  // in submission order (EOS included where hit).  max_new_tokens: one int or
  // one per prompt; prompt i draws with seed + i.
  // logprobs (None, or 0 .. 8): with it the result is (ids, logprobs), logprobs
  // per prompt one serve_logprobs entry per generated token.  prefix_cache: as
  // serve_begin's.
  py::object generate_many(const std::vector<std::vector<int32_t>>& prompts,
                           py::object max_new_tokens, int eos_token_id, float temperature,
                           int top_k, float top_p, uint64_t seed, py::object logprobs,
                           bool prefix_cache) {
    const bool want_lp = !logprobs.is_none();
    const int top_lp = want_lp ? logprobs.cast<int>() : -1;
    const size_t B = (size_t)std::max(cfg_.max_batch, 1);
    struct TokenLp { float lp; std::vector<std::pair<int32_t, float>> top; };
    std::vector<std::vector<TokenLp>> lps(prompts.size());
    std::vector<float> clp(B), tlp(B * LLM_MAX_TOP_LOGPROBS);
    std::vector<int32_t> tid(B * LLM_MAX_TOP_LOGPROBS), tn(B);
    const size_t n = prompts.size();
    std::vector<int> max_new;
    if (py::isinstance<py::int_>(max_new_tokens)) max_new.assign(n, max_new_tokens.cast<int>());
    else max_new = max_new_tokens.cast<std::vector<int>>();
    if (max_new.size() != n)
      throw std::invalid_argument("generate_many: max_new_tokens must be an int or one per prompt");
    std::vector<std::vector<int>> out(n);
    auto result = [&]() -> py::object {
      if (!want_lp) return py::cast(out);
      py::list all;
      for (const auto& per : lps) {
        py::list one;
        for (const TokenLp& t : per) {
          py::list top;
          for (const auto& p : t.top) top.append(py::make_tuple(p.first, p.second));
          one.append(py::make_tuple(t.lp, top));
        }
        all.append(one);
      }
      return py::make_tuple(py::cast(out), all);
    };
    if (n == 0) return result();
    std::vector<llm_serve_event> ev((size_t)std::max(cfg_.max_batch, 1));
    {
    py::gil_scoped_release nogil;
    const llm_serve_options so{prefix_cache ? 1 : 0};
    check(llm_decoder_serve_begin_opts(d_, &so));
    int rc = LLM_OK, range_rc = LLM_OK;
    for (size_t i = 0; i < n && rc == LLM_OK; ++i) {
      llm_request_options o{max_new[i], eos_token_id, temperature, top_k, top_p, seed + i};
      long long id = -1;
      rc = want_lp ? llm_decoder_submit_logprobs(d_, prompts[i].data(), (int)prompts[i].size(), &o,
                                                 top_lp, &id)
                   : llm_decoder_submit(d_, prompts[i].data(), (int)prompts[i].size(), &o, &id);
    }
    for (size_t left = n; rc == LLM_OK && left > 0;) {
      int ne = 0;
      rc = llm_decoder_serve_step(d_, nullptr, ev.data(), (int)ev.size(), &ne);
      if (rc == LLM_ERR_RANGE) { range_rc = rc; rc = LLM_OK; }  // (ids complete, as generate)
      if (rc == LLM_OK && ne == 0) {  // requests outstanding and nothing live or admissible
        (void)llm_decoder_serve_end(d_);
        throw std::runtime_error("llm_decoder: generate_many: a serve step returned no event "
                                 "with requests outstanding");
      }
      if (rc == LLM_OK && want_lp && ne > 0)
        rc = llm_decoder_serve_logprobs(d_, clp.data(), tlp.data(), tid.data(), tn.data());
      for (int j = 0; rc == LLM_OK && j < ne; ++j) {
        out[(size_t)ev[j].id].push_back(ev[j].token);
        left -= ev[j].finish != 0;
        if (want_lp) {
          TokenLp t{clp[j], {}};
          for (int k = 0; k < tn[j]; ++k)
            t.top.emplace_back(tid[(size_t)j * LLM_MAX_TOP_LOGPROBS + k],
                               tlp[(size_t)j * LLM_MAX_TOP_LOGPROBS + k]);
          lps[(size_t)ev[j].id].push_back(std::move(t));
        }
      }
    }
    std::string err = rc != LLM_OK ? llm_last_error() : "";
    const int rc_end = llm_decoder_serve_end(d_);
    if (rc != LLM_OK) throw std::runtime_error("llm_decoder: " + err);
    check(rc_end);
    if (range_rc)
      throw std::runtime_error("llm_decoder: generate_many: the fused o_proj clamped a head "
                               "product in at least one step");
    }
    return result();
  }

  void begin_beams(int num_seqs, int beam_width, int shared_len, int beam_len, uint64_t seed,
                   bool shuffle) {
    py::gil_scoped_release nogil;
    check(llm_decoder_begin_beams(d_, num_seqs, beam_width, shared_len, beam_len, seed,
                                  shuffle ? 1 : 0));
  }

  py::object step(py::object tokens, uintptr_t logits_ptr, uintptr_t stream, bool want_next) {
    std::vector<int32_t> tok;
    const int32_t* tp = nullptr;
    if (!tokens.is_none()) {
      tok = tokens.cast<std::vector<int32_t>>();
      tp = tok.data();
    }
    int n = 0;
    for (;; ++n)
      if (llm_decoder_context_len(d_, n) < 0) break;
    if (tp && (int)tok.size() != n) throw std::invalid_argument("step: need one token per active row");
    std::vector<int32_t> next(want_next ? n : 0);
    {
      py::gil_scoped_release nogil;
      check(llm_decoder_step(d_, tp, reinterpret_cast<float*>(logits_ptr),
                             want_next ? next.data() : nullptr, reinterpret_cast<void*>(stream)));
    }
    if (!want_next) return py::none();
    return py::cast(std::vector<int>(next.begin(), next.end()));
  }

  void sync() {
    py::gil_scoped_release nogil;
    check(llm_decoder_sync(d_));
  }
  void copy_next_ids(uintptr_t dst, uintptr_t stream) {
    py::gil_scoped_release nogil;
    check(llm_decoder_copy_next(d_, reinterpret_cast<int32_t*>(dst), reinterpret_cast<void*>(stream)));
  }
  // llm_decoder_set_taps: device pointers (0, 0 switches the taps off)
  void set_taps(uintptr_t q_ptr, uintptr_t s_ptr) {
    py::gil_scoped_release nogil;
    check(llm_decoder_set_taps(d_, reinterpret_cast<int8_t*>(q_ptr), reinterpret_cast<float*>(s_ptr)));
  }
  int context_len(int row) const { return llm_decoder_context_len(d_, row); }
  void run_attention(int layer, uintptr_t stream) {
    py::gil_scoped_release nogil;
    check(llm_decoder_run_attention(d_, layer, reinterpret_cast<void*>(stream)));
  }
  // llm_decoder_oproj_status: (range guard tripped, accumulator columns not at zero)
  py::tuple oproj_status() {
    int clamped = 0;
    long long nz = 0;
    {
      py::gil_scoped_release nogil;
      check(llm_decoder_oproj_status(d_, &clamped, &nz));
    }
    return py::make_tuple(clamped != 0, nz);
  }
  // llm_decoder_attention_plan: (splits per (row, head), LLM_PA_FORM_*)
  py::tuple attention_plan() {
    int ns = 0, form = 0;
    check(llm_decoder_attention_plan(d_, &ns, &form));
    return py::make_tuple(ns, form);
  }
  uintptr_t kv_handle() const { return reinterpret_cast<uintptr_t>(llm_decoder_kv(d_)); }
  // llm_decoder_set_kv_scales: per-layer scales of an fp8 KV decoder (None: all 1.0)
  void set_kv_scales(py::object k, py::object v) {
    std::vector<float> ks, vs;
    if (!k.is_none()) ks = k.cast<std::vector<float>>();
    if (!v.is_none()) vs = v.cast<std::vector<float>>();
    if ((!k.is_none() && (int)ks.size() != cfg_.num_layers) ||
        (!v.is_none() && (int)vs.size() != cfg_.num_layers))
      throw std::invalid_argument("set_kv_scales: need one scale per layer");
    check(llm_decoder_set_kv_scales(d_, k.is_none() ? nullptr : ks.data(),
                                    v.is_none() ? nullptr : vs.data()));
  }
  // llm_decoder_set_rope: set_rope(theta=10000.0) builds the standard table
  // (llm_rope_table), set_rope(table=ndarray) takes float32 [max_seq_len,
  // head_dim] of (cos, sin) pairs, set_rope(None) turns rotation off
  void set_rope(py::object table, double theta) {
    if (table.is_none()) {
      check(llm_decoder_set_rope(d_, nullptr));
      return;
    }
    const size_t S = (size_t)cfg_.max_seq_len, D = (size_t)cfg_.head_dim;
    if (table.is(py::ellipsis())) {
      std::vector<float> t(S * D);
      check(llm_rope_table(theta, cfg_.head_dim, cfg_.max_seq_len, t.data()));
      check(llm_decoder_set_rope(d_, t.data()));
      return;
    }
    auto a = py::array_t<float, py::array::c_style | py::array::forcecast>::ensure(table);
    if (!a || a.ndim() != 2 || (size_t)a.shape(0) != S || (size_t)a.shape(1) != D)
      throw std::invalid_argument("set_rope: table must be float32 [max_seq_len, head_dim]");
    check(llm_decoder_set_rope(d_, a.data()));
  }
  bool rope() const { return llm_decoder_rope(d_) == 1; }
  // llm_decoder_set_window: sliding-window attention over the last `window`
  // positions (0: off), before any rows are active
  void set_window(int window) { check(llm_decoder_set_window(d_, window)); }
  int window() const { return llm_decoder_window(d_); }
  std::string kv_dtype() const {
    return llm_decoder_kv_dtype(d_) == LLM_FP8 ? "float8_e4m3fn" : "float16";
  }
  // llm_decoder_prefill_kernel: the attention kernel prompt chunks take
  std::string prefill_kernel() const {
    return llm_decoder_prefill_kernel(d_) == LLM_PREFILL_MFMA ? "mfma" : "decode";
  }
  const llm_decoder_config& config() const { return cfg_; }

 private:
  llm_decoder* d_ = nullptr;
  llm_decoder_config cfg_{};
};

class CUDADecoder : public Decoder {
 public:
  CUDADecoder(int L, int H, int D, int hid, int V, int S, int max_batch, int page_size, int inter,
              float attn_scale, long long num_pages, const std::string& kv_dtype)
      : Decoder(LLM_F16, L, H, D, hid, V, S, max_batch, page_size, inter, attn_scale, num_pages,
                kv_dtype) {}
};

class INT8Decoder : public Decoder {
 public:
  INT8Decoder(int L, int H, int D, int hid, int V, int S, int max_batch, int page_size, int inter,
              float attn_scale, long long num_pages, const std::string& kv_dtype)
      : Decoder(LLM_I8, L, H, D, hid, V, S, max_batch, page_size, inter, attn_scale, num_pages,
                kv_dtype) {}
};

// KVTileCache<T> (kv_cache/kv_tile_cache.hpp:9-41) with a layer dimension.
class KVTileCache {
 public:
  KVTileCache() = default;
  ~KVTileCache() { if (c_) kv_cache_destroy(c_); }
  // dtype: the T of KVTileCache<T> — "float16" (default), "bfloat16", "float32", "int8" --
  // or "fp8" / "float8_e4m3fn" (LLM_FP8 bytes; the caller keeps the scales)
  void init(int num_pages, int tile_size, int head_dim, int num_layers, int num_beams,
            int num_heads, int max_tiles, const std::string& dtype) {
    const int kvt = dtype == "float16" || dtype == "half" ? LLM_F16
                    : dtype == "bfloat16"                 ? LLM_BF16
                    : dtype == "float32" || dtype == "float" ? LLM_F32
                    : dtype == "int8"                     ? LLM_I8
                    : dtype == "fp8" || dtype == "float8_e4m3fn" ? LLM_FP8
                                                          : -1;
    if (kvt < 0)
      throw std::invalid_argument("KVTileCache: dtype must be float16, bfloat16, float32, int8 or fp8");
    if (c_) { kv_cache_destroy(c_); c_ = nullptr; }
    check(kv_cache_create_typed(num_layers, num_beams, num_heads, head_dim, tile_size, max_tiles,
                                num_pages, kvt, &c_));
    tile_size_ = tile_size; head_dim_ = head_dim; layers_ = num_layers; beams_ = num_beams;
    heads_ = num_heads; max_tiles_ = max_tiles; dtype_ = dtype;
    es_ = kvt == LLM_F32 ? 4 : kvt == LLM_I8 || kvt == LLM_FP8 ? 1 : 2;
  }
  void resize(int new_num_pages, int new_tile_size) {  // kv_tile_cache.cpp:26-37: drops contents
    init(new_num_pages, new_tile_size, head_dim_, layers_, beams_, heads_, max_tiles_, dtype_);
  }
  uintptr_t get_key_ptr(int page) const {
    need();
    if (page < 0 || page >= kv_cache_num_pages(c_)) throw std::out_of_range("page id");
    return reinterpret_cast<uintptr_t>(kv_cache_k_pool(c_)) + (uintptr_t)page * kv_cache_page_stride(c_);
  }
  uintptr_t get_value_ptr(int page) const {
    need();
    if (page < 0 || page >= kv_cache_num_pages(c_)) throw std::out_of_range("page id");
    return reinterpret_cast<uintptr_t>(kv_cache_v_pool(c_)) + (uintptr_t)page * kv_cache_page_stride(c_);
  }
  int register_tile(int beam, int head, int tile, int layer) {
    need();
    int32_t page = -1;
    check(kv_cache_register_tile(c_, layer, beam, head, tile, &page));
    return page;
  }
  int lookup(int beam, int head, int tile, int layer) const {
    need();
    return kv_cache_lookup(c_, layer, beam, head, tile);
  }
  // "lru": KVTileCache's eviction when the pool is full (kv_tile_cache.cpp:89-98);
  // "none" (default): register_tile raises instead
  void set_eviction(const std::string& policy) {
    need();
    if (policy != "lru" && policy != "none")
      throw std::invalid_argument("KVTileCache.set_eviction: policy must be 'lru' or 'none'");
    check(kv_cache_set_eviction(c_, policy == "lru" ? LLM_EVICT_LRU : LLM_EVICT_NONE));
  }
  void fork(int src, int dst) { need(); check(kv_cache_fork(c_, src, dst)); }
  // kv_cache_reorder: row first_beam + i := what row first_beam + parent[i] held
  void reorder(int first_beam, const std::vector<int32_t>& parent, int n_tokens) {
    need();
    check(kv_cache_reorder(c_, first_beam, (int)parent.size(), parent.data(), n_tokens));
  }
  void release(int beam) { need(); check(kv_cache_release(c_, beam)); }
  // kv_cache_release_before: the pages of the tiles wholly below token n_tokens
  void release_before(int beam, int n_tokens) {
    need();
    check(kv_cache_release_before(c_, beam, n_tokens));
  }
  void sync_page_table_to_gpu() { need(); check(kv_cache_sync(c_, nullptr)); check(llm_sync()); }
  // KVTileCache::save_to_file / load_from_file (kv_tile_cache.cpp:105-125):
  // format "pools" (default) is the reference's file byte for byte (raw K pool
  // then V pool; the page table stays as it is); "snapshot" is this build's
  // file that also restores the layered page table.
  void save_to_file(const std::string& p, const std::string& format) {
    need();
    check(fmt(format) ? kv_cache_save(c_, p.c_str()) : kv_cache_save_pools(c_, p.c_str()));
  }
  void load_from_file(const std::string& p, const std::string& format) {
    need();
    check(fmt(format) ? kv_cache_load(c_, p.c_str()) : kv_cache_load_pools(c_, p.c_str()));
  }
  // KVTileCacheCPU<T>::save / load (kv_tile_cache_cpu.cpp:89-123): the K ("k")
  // or V ("v") tiles of one layer as the reference's record file
  void save_tiles(const std::string& p, const std::string& kind, int layer) {
    need();
    check(kv_cache_save_tiles(c_, layer, kind_of(kind), p.c_str()));
  }
  void load_tiles(const std::string& p, const std::string& kind, int layer) {
    need();
    check(kv_cache_load_tiles(c_, layer, kind_of(kind), p.c_str()));
  }
  // k / v: C-contiguous [n][H][D] arrays whose items are the cache's element
  // bits (fp16/bf16 as uint16 or float16, float32, int8).
  void write_tokens(int layer, int beam, int pos, py::array k, py::array v) {
    need();
    const bool contig = (k.flags() & py::array::c_style) && (v.flags() & py::array::c_style);
    if (!contig || k.itemsize() != es_ || v.itemsize() != es_ || k.size() != v.size() ||
        k.size() % ((size_t)heads_ * head_dim_) != 0)
      throw std::invalid_argument("write_tokens: k/v must be C-contiguous [n][H][D] arrays of the "
                                  "cache's element size");
    const int n = (int)(k.size() / ((size_t)heads_ * head_dim_));
    check(kv_cache_write_tokens(c_, layer, beam, pos, n, k.data(), v.data()));
  }
  py::dict view(int layer) const {
    need();
    pa_kv_view v;
    check(kv_cache_view(c_, layer, &v));
    py::dict d;
    d["k_pool"] = reinterpret_cast<uintptr_t>(v.k_pool);
    d["v_pool"] = reinterpret_cast<uintptr_t>(v.v_pool);
    d["page_table"] = reinterpret_cast<uintptr_t>(v.page_table);
    d["num_pages"] = v.num_pages; d["page_size"] = v.page_size; d["head_dim"] = v.head_dim;
    d["num_beams"] = v.num_beams; d["num_heads"] = v.num_heads; d["max_tiles"] = v.max_tiles;
    d["kv_dtype"] = v.kv_dtype;
    d["page_stride"] = v.page_stride;
    return d;
  }
  long long free_pages() const { need(); return kv_cache_free_pages(c_); }
  long long num_pages() const { need(); return kv_cache_num_pages(c_); }
  uintptr_t handle() const { return reinterpret_cast<uintptr_t>(c_); }

 private:
  static int llm_sync() { return LLM_OK; }
  static bool fmt(const std::string& f) {
    if (f == "pools") return false;
    if (f == "snapshot") return true;
    throw std::invalid_argument("KVTileCache: format must be 'pools' (the reference's file) or 'snapshot'");
  }
  static int kind_of(const std::string& k) {
    if (k == "k" || k == "K") return 0;
    if (k == "v" || k == "V") return 1;
    throw std::invalid_argument("KVTileCache: kind must be 'k' or 'v'");
  }
  void need() const { if (!c_) throw std::runtime_error("KVTileCache: call init() first"); }
  kv_cache* c_ = nullptr;
  int tile_size_ = 0, head_dim_ = 0, layers_ = 1, beams_ = 1, heads_ = 1, max_tiles_ = 1;
  int es_ = 2;
  std::string dtype_ = "float16";
};

// PageTable (kv_cache/page_table.hpp:5-37): a one-layer table whose entries
// name pages of an external pool; backed by a kv_cache with 1-element pages.
class PageTable {
 public:
  PageTable() = default;
  ~PageTable() { if (c_) kv_cache_destroy(c_); }
  void init(int num_beams, int num_heads, int num_tiles) {
    if (c_) { kv_cache_destroy(c_); c_ = nullptr; }
    const long long pages = std::max<long long>(1, (long long)num_beams * num_heads * num_tiles);
    check(kv_cache_create(1, num_beams, num_heads, 1, 1, num_tiles, pages, &c_));
  }
  void clear() { need(); check(kv_cache_clear(c_)); }
  void assign(int beam, int head, int tile, int page) {
    need();
    check(kv_cache_assign(c_, 0, beam, head, tile, page));
    check(kv_cache_sync(c_, nullptr));
  }
  int lookup(int beam, int head, int tile) const { need(); return kv_cache_lookup(c_, 0, beam, head, tile); }
  void remove(int beam, int head, int tile) { need(); check(kv_cache_remove(c_, 0, beam, head, tile)); }
  void sync_to_gpu() { need(); check(kv_cache_sync(c_, nullptr)); }
  // kv_cache_release_before (a PageTable's tiles are one token each): entries
  // of tiles < n_tiles become -1 on the host; sync_to_gpu pushes them
  void release_before(int beam, int n_tiles) {
    need();
    check(kv_cache_release_before(c_, beam, n_tiles));
  }
  uintptr_t device_data() const { need(); return reinterpret_cast<uintptr_t>(kv_cache_page_table(c_, 0)); }

 private:
  void need() const { if (!c_) throw std::runtime_error("PageTable: call init() first"); }
  kv_cache* c_ = nullptr;
};

}  // namespace

PYBIND11_MODULE(llm_decoder, m) {
  m.doc() = "MI355X (gfx950) paged-attention decoder: CUDADecoder / INT8Decoder (HIP)";
  m.attr("ABI_VERSION") = llm_abi_version();

  auto dec_init = [](auto* cls) {
    return py::init([](int L, int H, int D, int hid, int V, int S, int max_batch, int page_size,
                       int inter, float attn_scale, long long num_pages,
                       const std::string& kv_dtype) {
             return new std::remove_pointer_t<decltype(cls)>(L, H, D, hid, V, S, max_batch,
                                                             page_size, inter, attn_scale,
                                                             num_pages, kv_dtype);
           });
  };
  auto common = [&](auto& c) {
    c.def("load_weights", &Decoder::load_weights, "CUDADecoder::load_weights (fp32 .bin dir)")
        .def("set_weights", &Decoder::set_weights, py::arg("weights"))
        .def("generate", &Decoder::generate)
        .def("generate_batch", &Decoder::generate_batch, py::arg("input_ids"),
             py::arg("max_gen_len"), py::arg("temperature") = 1.0f)
        .def("beam_search", &Decoder::beam_search, py::arg("input_ids"),
             py::arg("beam_width") = 4, py::arg("max_new_tokens") = 32,
             py::arg("eos_token_id") = -1, py::arg("length_penalty") = 1.0f,
             py::arg("return_trace") = false, py::arg("trace_logits_ptr") = 0)
        .def("beam_search_batch", &Decoder::beam_search_batch, py::arg("input_ids"),
             py::arg("beam_width") = 4, py::arg("max_new_tokens") = 32,
             py::arg("eos_token_id") = -1, py::arg("length_penalty") = 1.0f,
             py::arg("return_trace") = false, py::arg("trace_logits_ptr") = 0)
        .def("begin_synthetic", &Decoder::begin_synthetic, py::arg("batch"),
             py::arg("context_len"), py::arg("seed") = 0, py::arg("shuffle") = true)
        .def("prefill", &Decoder::prefill, py::arg("row"), py::arg("tokens"))
        .def("prefill_batch", &Decoder::prefill_batch, py::arg("rows"), py::arg("tokens"))
        .def_property("packed_prefill", &Decoder::packed_prefill, &Decoder::set_packed_prefill)
        .def("set_sampling", &Decoder::set_sampling, py::arg("temperature"),
             py::arg("top_k") = 0, py::arg("top_p") = 1.0f, py::arg("seed") = 0)
        .def("serve_begin", &Decoder::serve_begin, py::arg("prefix_cache") = false)
        .def("submit", &Decoder::submit, py::arg("tokens"), py::arg("max_new_tokens"),
             py::arg("eos_token_id") = -1, py::arg("temperature") = 0.0f, py::arg("top_k") = 0,
             py::arg("top_p") = 1.0f, py::arg("seed") = 0, py::arg("logprobs") = py::none())
        .def("serve_logprobs", &Decoder::serve_logprobs)
        .def("score", &Decoder::score, py::arg("sequences"))
        .def("cancel", &Decoder::cancel, py::arg("id"))
        .def("serve_step", &Decoder::serve_step, py::arg("logits_ptr") = 0)
        .def("serve_stats", &Decoder::serve_stats)
        .def("serve_prefix_stats", &Decoder::serve_prefix_stats)
        .def("serve_end", &Decoder::serve_end)
        .def("generate_many", &Decoder::generate_many, py::arg("prompts"),
             py::arg("max_new_tokens"), py::arg("eos_token_id") = -1,
             py::arg("temperature") = 0.0f, py::arg("top_k") = 0, py::arg("top_p") = 1.0f,
             py::arg("seed") = 0, py::arg("logprobs") = py::none(),
             py::arg("prefix_cache") = false)
        .def("begin_beams", &Decoder::begin_beams, py::arg("num_seqs"), py::arg("beam_width"),
             py::arg("shared_len"), py::arg("beam_len"), py::arg("seed") = 0,
             py::arg("shuffle") = true)
        .def("step", &Decoder::step, py::arg("tokens") = py::none(), py::arg("logits_ptr") = 0,
             py::arg("stream") = 0, py::arg("want_next") = true)
        .def("sync", &Decoder::sync)
        .def("set_taps", &Decoder::set_taps, py::arg("q_ptr"), py::arg("s_ptr"))
        .def("copy_next_ids", &Decoder::copy_next_ids, py::arg("dst_ptr"), py::arg("stream") = 0)
        .def("context_len", &Decoder::context_len)
        .def("attention_plan", &Decoder::attention_plan)
        .def("oproj_status", &Decoder::oproj_status)
        .def("run_attention", &Decoder::run_attention, py::arg("layer") = 0,
             py::arg("stream") = 0)
        .def("set_kv_scales", &Decoder::set_kv_scales, py::arg("k_scale") = py::none(),
             py::arg("v_scale") = py::none())
        .def("set_rope", &Decoder::set_rope, py::arg("table") = py::ellipsis(),
             py::arg("theta") = 10000.0)
        .def_property_readonly("rope", &Decoder::rope)
        .def("set_window", &Decoder::set_window, py::arg("window"))
        .def_property_readonly("window", &Decoder::window)
        .def_property_readonly("kv_dtype", &Decoder::kv_dtype)
        .def_property_readonly("prefill_kernel", &Decoder::prefill_kernel)
        .def_property_readonly("kv_handle", &Decoder::kv_handle);
  };
  py::class_<Decoder>(m, "_Decoder");
  py::class_<CUDADecoder, Decoder> cd(m, "CUDADecoder");
  cd.def(dec_init((CUDADecoder*)nullptr), py::arg("num_layers"), py::arg("num_heads"),
         py::arg("head_dim"), py::arg("hidden_dim"), py::arg("vocab_size"),
         py::arg("max_seq_len"), py::arg("max_batch") = 1, py::arg("page_size") = 16,
         py::arg("inter_dim") = 0, py::arg("attn_scale") = 1.0f, py::arg("num_pages") = 0,
         py::arg("kv_dtype") = "float16");
  common(cd);
  py::class_<INT8Decoder, Decoder> id(m, "INT8Decoder");
  id.def(dec_init((INT8Decoder*)nullptr), py::arg("num_layers"), py::arg("num_heads"),
         py::arg("head_dim"), py::arg("hidden_dim"), py::arg("vocab_size"),
         py::arg("max_seq_len"), py::arg("max_batch") = 1, py::arg("page_size") = 16,
         py::arg("inter_dim") = 0, py::arg("attn_scale") = 1.0f, py::arg("num_pages") = 0,
         py::arg("kv_dtype") = "float16");
  common(id);
  id.def("load_quantized_weights", &Decoder::load_quantized_weights)
      .def("quantize_weights", &Decoder::quantize_weights);

  py::class_<KVTileCache>(m, "KVTileCache")
      .def(py::init<>())
      .def("init", &KVTileCache::init, py::arg("num_pages"), py::arg("tile_size"),
           py::arg("head_dim"), py::arg("num_layers") = 1, py::arg("num_beams") = 1,
           py::arg("num_heads") = 1, py::arg("max_tiles") = 1, py::arg("dtype") = "float16")
      .def("resize", &KVTileCache::resize)
      .def("get_key_ptr", &KVTileCache::get_key_ptr)
      .def("get_value_ptr", &KVTileCache::get_value_ptr)
      .def("register_tile", &KVTileCache::register_tile, py::arg("beam_id"), py::arg("head_id"),
           py::arg("tile_id"), py::arg("layer") = 0)
      .def("lookup", &KVTileCache::lookup, py::arg("beam_id"), py::arg("head_id"),
           py::arg("tile_id"), py::arg("layer") = 0)
      .def("set_eviction", &KVTileCache::set_eviction, py::arg("policy"))
      .def("fork", &KVTileCache::fork)
      .def("reorder", &KVTileCache::reorder, py::arg("first_beam"), py::arg("parent"),
           py::arg("n_tokens"))
      .def("release", &KVTileCache::release)
      .def("release_before", &KVTileCache::release_before, py::arg("beam"), py::arg("n_tokens"))
      .def("sync_page_table_to_gpu", &KVTileCache::sync_page_table_to_gpu)
      .def("save_to_file", &KVTileCache::save_to_file, py::arg("path"),
           py::arg("format") = "pools")
      .def("load_from_file", &KVTileCache::load_from_file, py::arg("path"),
           py::arg("format") = "pools")
      .def("save_tiles", &KVTileCache::save_tiles, py::arg("path"), py::arg("kind") = "k",
           py::arg("layer") = 0)
      .def("load_tiles", &KVTileCache::load_tiles, py::arg("path"), py::arg("kind") = "k",
           py::arg("layer") = 0)
      .def("write_tokens", &KVTileCache::write_tokens)
      .def("view", &KVTileCache::view, py::arg("layer") = 0)
      .def("free_pages", &KVTileCache::free_pages)
      .def("num_pages", &KVTileCache::num_pages)
      .def_property_readonly("handle", &KVTileCache::handle);

  py::class_<PageTable>(m, "PageTable")
      .def(py::init<>())
      .def("init", &PageTable::init)
      .def("clear", &PageTable::clear)
      .def("assign", &PageTable::assign)
      .def("lookup", &PageTable::lookup)
      .def("remove", &PageTable::remove)
      .def("sync_to_gpu", &PageTable::sync_to_gpu)
      .def("release_before", &PageTable::release_before, py::arg("beam"), py::arg("n_tiles"))
      .def("device_data", &PageTable::device_data);

  m.def("paged_attention",
        [](uintptr_t kv_handle, int layer, uintptr_t q, uintptr_t out, uintptr_t beam_ids,
           uintptr_t context_lens, int B, int H, int D, int T, float temperature, int top_k,
           float top_p, uintptr_t workspace, size_t workspace_bytes, uintptr_t stream,
           int row_group, int eos_token, float eos_threshold, uintptr_t probs_out,
           uintptr_t scores_out) {
          // AttentionCUDA::forward (attention/attention_cuda.cu:41-95) over a KVTileCache;
          // the filters and weight / score outputs of CPUAttentionInput / Output
          // (attention_cpu/attention_cpu.hpp:8-43) go through pa_decode_ex.
          pa_kv_view v;
          check(kv_cache_view(reinterpret_cast<kv_cache*>(kv_handle), layer, &v));
          const auto* qp = reinterpret_cast<const float*>(q);
          auto* op = reinterpret_cast<float*>(out);
          const auto* bi = reinterpret_cast<const int32_t*>(beam_ids);
          const auto* cl = reinterpret_cast<const int32_t*>(context_lens);
          void* ws = reinterpret_cast<void*>(workspace);
          void* st = reinterpret_cast<void*>(stream);
          if (top_k > 0 || top_p < 1.0f || eos_token >= 0 || probs_out || scores_out) {
            pa_decode_options o{temperature, top_k, top_p, eos_token, eos_threshold,
                                reinterpret_cast<float*>(probs_out),
                                reinterpret_cast<float*>(scores_out)};
            py::gil_scoped_release nogil;
            check(pa_decode_ex(&v, qp, op, bi, cl, B, H, D, T, &o, ws, workspace_bytes, st));
            return;
          }
          const float sm = 1.0f / (temperature * temperature);
          py::gil_scoped_release nogil;
          check(pa_decode_grouped(&v, qp, op, bi, cl, B, H, D, T, sm, 0, row_group, ws,
                                  workspace_bytes, st));
        },
        py::arg("kv_handle"), py::arg("layer"), py::arg("q"), py::arg("out"),
        py::arg("beam_ids") = 0, py::arg("context_lens") = 0, py::arg("B") = 1,
        py::arg("H") = 1, py::arg("D") = 64, py::arg("T") = 1, py::arg("temperature") = 1.0f,
        py::arg("top_k") = 0, py::arg("top_p") = 1.0f, py::arg("workspace") = 0,
        py::arg("workspace_bytes") = 0, py::arg("stream") = 0, py::arg("row_group") = 1,
        py::arg("eos_token") = -1, py::arg("eos_threshold") = 0.0f, py::arg("probs_out") = 0,
        py::arg("scores_out") = 0);
  m.def("beam_select",
        [](uintptr_t logits, uintptr_t score_in, int num_seqs, int W, int V, uintptr_t cand_score,
           uintptr_t cand_parent, uintptr_t cand_token, uintptr_t stream) {
          // beam_select_rows over device pointers: logits [num_seqs * W][V] and
          // score_in [num_seqs * W] fp32 -> the best 2W (score, parent, token) per sequence
          py::gil_scoped_release nogil;
          check(beam_select_rows(reinterpret_cast<const float*>(logits),
                                 reinterpret_cast<const float*>(score_in), num_seqs, W, V,
                                 reinterpret_cast<float*>(cand_score),
                                 reinterpret_cast<int32_t*>(cand_parent),
                                 reinterpret_cast<int32_t*>(cand_token),
                                 reinterpret_cast<void*>(stream)));
        },
        py::arg("logits"), py::arg("score_in"), py::arg("num_seqs"), py::arg("W"), py::arg("V"),
        py::arg("cand_score"), py::arg("cand_parent"), py::arg("cand_token"),
        py::arg("stream") = 0);
  m.def("dnnl_matmul_int8",
        [](uintptr_t A, uintptr_t B, uintptr_t C, int BATCH, int M, int N, int K, float scaleA,
           float scaleB, float scaleC, uintptr_t bias, const std::string& activation,
           uintptr_t stream) {
          // dnnl_matmul_int8 (attention_cpu/dnnl_matmul_int8.hpp:5-13): device
          // pointers; false on any failure, as the reference's catch (...) (:73-74);
          // an unknown activation adds no post-op (:44-50)
          const int act = activation == "relu" ? LLM_ACT_RELU
                          : activation == "gelu" ? LLM_ACT_GELU : LLM_ACT_NONE;
          py::gil_scoped_release nogil;
          return i8_matmul_s8(reinterpret_cast<const int8_t*>(A), reinterpret_cast<const int8_t*>(B),
                              reinterpret_cast<int8_t*>(C), BATCH, M, N, K, scaleA, scaleB, scaleC,
                              reinterpret_cast<const float*>(bias), act,
                              reinterpret_cast<void*>(stream)) == LLM_OK;
        },
        py::arg("A"), py::arg("B"), py::arg("C"), py::arg("BATCH"), py::arg("M"), py::arg("N"),
        py::arg("K"), py::arg("scaleA"), py::arg("scaleB"), py::arg("scaleC") = 1.0f,
        py::arg("bias") = 0, py::arg("activation") = "", py::arg("stream") = 0);
  // llm_rope_table: float32 [num_pos, head_dim] of (cos, sin) pairs
  m.def("rope_table",
        [](double theta, int head_dim, int num_pos) {
          if (head_dim <= 0 || num_pos <= 0) throw std::invalid_argument("rope_table: bad shape");
          py::array_t<float> a({(py::ssize_t)num_pos, (py::ssize_t)head_dim});
          check(llm_rope_table(theta, head_dim, num_pos, a.mutable_data()));
          return a;
        },
        py::arg("theta"), py::arg("head_dim"), py::arg("num_pos"));
  m.def("workspace_bytes", &pa_decode_workspace_bytes, py::arg("B"), py::arg("H"), py::arg("D"),
        py::arg("max_tiles"), py::arg("pages_per_split") = 0);
  m.def("filter_workspace_bytes", &pa_decode_ex_workspace_bytes, py::arg("B"), py::arg("H"),
        py::arg("T"));
}
