// Continuous batching: the scheduler core.  Host-only and pure (no HIP
// headers, no decoder state): requests in, the row decisions of every serve
// step out (decoder_serve.cpp llm_decoder_serve_step executes them;
// serve_plan_sim_tune is the test entry).
//
// Policy, fixed here:
//   * a request may ever append T = prompt_len + max_new_tokens - 1 positions
//     (generate's bound) and is charged the pages that can hold them
//     (serve_row_tiles) when it is admitted, for as long as it lives;
//   * admission is strict FIFO at the start of a step: the head of the queue
//     enters while a row is free and committed + need(head) <= num_pages; a
//     head that does not fit is never skipped.  So no step of an admitted
//     request can run out of pages, and nothing is ever preempted;
//   * live rows are dense, 0 .. live - 1: a new request takes row `live`, and
//     a retired row r that is not the last live row receives the last one.
#pragma once

#include <algorithm>
#include <deque>
#include <vector>

namespace llm {

struct ServeGeom {
  int max_rows = 0;           // the decoder's max_batch
  long long num_pages = 0;    // of the pool
  int pages_per_tile = 0;     // num_layers * num_heads: the pages of one tile of a row
  int page_size = 0;
  int window = 0;             // sliding window (0: off)
  int max_seq_len = 0;
};

// The tiles one row can hold at once, per (layer, head), over a life of T
// appended positions -- THE per-row page rule.  kv_cache allocates a row's
// tile pos / page_size for every layer and head when position pos is appended
// (KvCache::prepare_append), so T positions take ceil(T / page_size) tiles.
// A windowed decoder releases the tiles wholly below position p + 1 - window
// before it appends p (KvCache::release_before in run_step / prefill_pass), and
// a prefill pass appends up to 512 positions after one release: at most
// window + 512 positions stay mapped, which span one tile more than they fill
// (llm_decoder_set_window's bound).
inline long long serve_row_tiles(const ServeGeom& g, long long T) {
  const long long tiles = (T + g.page_size - 1) / g.page_size;
  if (g.window <= 0) return tiles;
  return std::min(tiles, ((long long)g.window + 512 + g.page_size - 1) / g.page_size + 1);
}

// Positions a request ever appends.
inline long long serve_positions(int prompt_len, int max_new) {
  return (long long)prompt_len + max_new - 1;
}

// Pages charged to a request while it lives.
inline long long serve_need(const ServeGeom& g, int prompt_len, int max_new) {
  return serve_row_tiles(g, serve_positions(prompt_len, max_new)) * g.pages_per_tile;
}

struct ServeReq {
  long long id = -1;
  int prompt_len = 0, max_new = 0;
  long long need = 0;
  int delivered = 0;  // tokens handed out so far
};

// A row re-parented at a retirement: what row `src` (the last live row) held
// is row `dst` from now on.
struct ServeMove {
  int dst, src;
};

class ServePlan {
 public:
  void begin(const ServeGeom& g) {
    geom_ = g;
    waiting_.clear();
    live_.clear();
    committed_ = 0;
    next_id_ = 0;
  }

  const ServeGeom& geom() const { return geom_; }
  int live() const { return (int)live_.size(); }
  int waiting() const { return (int)waiting_.size(); }
  long long committed() const { return committed_; }
  const ServeReq& row(int r) const { return live_[r]; }
  ServeReq& row(int r) { return live_[r]; }

  // Whether a request of this shape can ever be served by the geometry.
  bool fits(int prompt_len, int max_new) const {
    return prompt_len >= 1 && max_new >= 1 &&
           serve_positions(prompt_len, max_new) <= geom_.max_seq_len &&
           serve_need(geom_, prompt_len, max_new) <= geom_.num_pages;
  }

  // Queue a request; its id, or -1 if it is refused (fits).
  long long submit(int prompt_len, int max_new) {
    if (!fits(prompt_len, max_new)) return -1;
    ServeReq q;
    q.id = next_id_++;
    q.prompt_len = prompt_len;
    q.max_new = max_new;
    q.need = serve_need(geom_, prompt_len, max_new);
    waiting_.push_back(q);
    return q.id;
  }

  // Start of a step: the head of the queue enters row `live` while it fits.
  // Returns the number admitted (rows live - n .. live - 1, in id order).
  int admit() {
    int n = 0;
    while (!waiting_.empty() && live() < geom_.max_rows &&
           committed_ + waiting_.front().need <= geom_.num_pages) {
      committed_ += waiting_.front().need;
      live_.push_back(waiting_.front());
      waiting_.pop_front();
      ++n;
    }
    return n;
  }

  // Retire row r (its request ended or was cancelled).  True with *mv set if
  // the last live row moved into r.
  bool retire(int r, ServeMove* mv) {
    const int last = live() - 1;
    committed_ -= live_[r].need;
    const bool moved = r != last;
    if (moved) {
      live_[r] = live_[last];
      *mv = ServeMove{r, last};
    }
    live_.pop_back();
    return moved;
  }

  // End of a step, once its tokens are known -- the one place the delivery,
  // finish and retirement order is written (the decoder and the simulation
  // both run it).  deliver(row, req) hands out row's token as generated index
  // req.delivered and returns whether the request ends with it before its
  // length does (its EOS token); rows in ascending order.  Then the finished
  // rows retire in descending row order: retired(row, req, finish, mv) with
  // finish 1 (ended early; wins) or 2 (max_new delivered) and mv the move that
  // filled the row, or NULL.  A callback returning non-zero stops the walk and
  // is returned (the plan is then in no defined state).
  template <typename Deliver, typename Retired>
  int finish_step(Deliver&& deliver, Retired&& retired) {
    const int n = live();
    fin_.assign(n, 0);
    for (int r = 0; r < n; ++r) {
      ServeReq& q = live_[r];
      const bool early = deliver(r, static_cast<const ServeReq&>(q));
      ++q.delivered;
      fin_[r] = early ? 1 : q.delivered >= q.max_new ? 2 : 0;
    }
    for (int r = n - 1; r >= 0; --r) {
      if (!fin_[r]) continue;
      const ServeReq q = live_[r];
      ServeMove mv;
      const bool moved = retire(r, &mv);
      if (int rc = retired(r, q, fin_[r], moved ? &mv : nullptr)) return rc;
    }
    return 0;
  }

  // Take a waiting request out of the queue.
  bool cancel_waiting(long long id) {
    for (auto it = waiting_.begin(); it != waiting_.end(); ++it)
      if (it->id == id) {
        waiting_.erase(it);
        return true;
      }
    return false;
  }

  // The row a live request holds, or -1.
  int row_of(long long id) const {
    for (int r = 0; r < live(); ++r)
      if (live_[r].id == id) return r;
    return -1;
  }

 private:
  ServeGeom geom_;
  std::deque<ServeReq> waiting_;
  std::vector<ServeReq> live_;
  std::vector<int> fin_;  // finish_step: the rows' finish reasons
  long long committed_ = 0, next_id_ = 0;
};

}  // namespace llm
