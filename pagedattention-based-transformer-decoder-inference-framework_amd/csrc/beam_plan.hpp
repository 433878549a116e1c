// Beam search: the host bookkeeping.  Host-only and pure (no HIP headers, no
// decoder state): the candidates the device reported in, the live beams of
// the next step and the ranked results out (decoder_beam.cpp
// llm_decoder_beam_search runs the device steps and re-parents the pages
// between the calls; beam_book_tune is the test entry).
//
// Policy, fixed here (include/llm_decoder.h, llm_decoder_beam_search):
//   * a sequence's 2W candidates arrive in rank order.  An EOS joins the
//     sequence's finished pool if its rank is < W and the sequence is not
//     done (it is ignored otherwise); anything else becomes the next live
//     beam until W are live, so a done sequence still advances its beams;
//   * a sequence with >= W finished hypotheses is done; the search may stop
//     when all are;
//   * at the end a sequence that is not done adds its live beams (beam order)
//     to its pool, and the best W by final score -- sum / len^length_penalty,
//     a stable sort, so equal scores keep pool order -- are the results.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace llm {

inline float beam_final_score(float sum, size_t len, float alpha) {
  return (float)((double)sum / std::pow((double)len, (double)alpha));
}

// (hidden: the libraries that include this export none of it)
class __attribute__((visibility("hidden"))) BeamPlan {
 public:
  void begin(int num_seqs, int W, int max_new, int eos_token, float length_penalty, int V) {
    S_ = num_seqs; W_ = W; max_new_ = max_new; eos_ = eos_token; alpha_ = length_penalty; V_ = V;
    finished_.assign(S_, {});
    done_.assign(S_, 0);
    hist_.assign((size_t)S_ * W_, {});
    score_.assign((size_t)S_ * W_, 0.f);
    next_hist_.assign(W_, {});
    next_score_.assign(W_, 0.f);
    next_tok_.assign(W_, 0);
    parent_.assign(W_, 0);
  }

  // One step of sequence s: its 2W candidates (score, parent beam, token) in
  // rank order.  On success NULL, with the W live beams of the next step in
  // parent / token / score (beam order) and the sequence's finished pool and
  // done flag updated.  Otherwise the text of the failure -- an LLM_ERR_HIP
  // of the caller's: the candidates are the device's -- with the live beams
  // and the three outputs untouched; the search ends there.
  const char* step(int s, const float* cand_score, const int32_t* cand_parent,
                   const int32_t* cand_token, int32_t* parent, int32_t* token, float* score) {
    const int b0 = s * W_, K = 2 * W_;
    int live = 0;
    for (int j = 0; j < K; ++j) {
      const float sc = cand_score[j];
      const int32_t p = cand_parent[j], t = cand_token[j];
      if (p < 0 || p >= W_ || t < 0 || t >= V_)
        return "llm_decoder_beam_search: the device returned a candidate out of range";
      if (t == eos_) {
        if (j < W_ && !done_[s]) {
          Hyp h;
          h.ids = hist_[b0 + p];
          h.ids.push_back(t);
          h.sum = sc;
          h.score = beam_final_score(sc, h.ids.size(), alpha_);
          finished_[s].push_back(std::move(h));
        }
      } else if (live < W_) {
        parent_[live] = p;
        next_tok_[live] = t;
        next_score_[live] = sc;
        next_hist_[live] = hist_[b0 + p];
        next_hist_[live].push_back(t);
        ++live;
      }
    }
    if (live != W_)
      return "llm_decoder_beam_search: fewer than beam_width live candidates";
    for (int w = 0; w < W_; ++w) {
      hist_[b0 + w].swap(next_hist_[w]);
      parent[w] = parent_[w];
      token[w] = next_tok_[w];
      score[w] = score_[b0 + w] = next_score_[w];
    }
    if ((int)finished_[s].size() >= W_) done_[s] = 1;
    return nullptr;
  }

  bool all_done() const {
    return std::all_of(done_.begin(), done_.end(), [](char d) { return d != 0; });
  }

  // The results: out_ids [num_seqs][W][max_new] (-1 past a hypothesis' end),
  // out_len / out_sum_logprob / out_score [num_seqs][W], best first.
  void finish(int32_t* out_ids, int32_t* out_len, float* out_sum_logprob, float* out_score) {
    for (int s = 0; s < S_; ++s) {
      std::vector<Hyp>& pool = finished_[s];
      if (!done_[s])
        for (int w = 0; w < W_; ++w) {
          Hyp h;
          h.ids = hist_[s * W_ + w];
          h.sum = score_[s * W_ + w];
          h.score = beam_final_score(h.sum, h.ids.size(), alpha_);
          pool.push_back(std::move(h));
        }
      std::stable_sort(pool.begin(), pool.end(),
                       [](const Hyp& a, const Hyp& b) { return a.score > b.score; });
      for (int w = 0; w < W_; ++w) {
        const Hyp& h = pool[w];
        int32_t* o = out_ids + ((size_t)s * W_ + w) * max_new_;
        for (int i = 0; i < max_new_; ++i) o[i] = i < (int)h.ids.size() ? h.ids[i] : -1;
        out_len[s * W_ + w] = (int32_t)h.ids.size();
        out_sum_logprob[s * W_ + w] = h.sum;
        out_score[s * W_ + w] = h.score;
      }
    }
  }

 private:
  struct Hyp {
    std::vector<int32_t> ids;
    float sum = 0.f;    // cumulative log-probability (the device's fp32 score)
    float score = 0.f;  // sum / len^alpha
  };
  int S_ = 0, W_ = 0, max_new_ = 0, eos_ = -1, V_ = 0;
  float alpha_ = 0.f;
  std::vector<std::vector<Hyp>> finished_;       // [num_seqs] pools
  std::vector<char> done_;                       // [num_seqs]
  std::vector<std::vector<int32_t>> hist_;       // [num_seqs * W] the live beams' ids
  std::vector<float> score_;                     // [num_seqs * W] ... and carried scores
  std::vector<std::vector<int32_t>> next_hist_;  // [W] step's staging
  std::vector<float> next_score_;
  std::vector<int32_t> next_tok_, parent_;
};

}  // namespace llm
