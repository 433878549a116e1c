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
//
// Prefix caching (begin(g, true); off by default, and off is the policy above
// unchanged).  Prompt blocks -- tile k of a prompt over all layers and heads,
// prefix_cache.hpp -- outlive the row that computed them, and a later request
// whose prompt begins with a cached chain of blocks starts behind it:
//   * hit: a prompt of n tokens prefills n - 1 positions and may hit at most
//     floor((n - 1) / page_size) blocks, the longest cached chain from the
//     root; its row starts at hit_blocks * page_size.  Position n - 1 and all
//     after it fall in tiles the request owns: nothing appends into a shared
//     tile;
//   * publish: after its admission prefill a new row publishes the full tiles
//     it computed, hit_blocks .. floor((n - 1) / page_size) - 1, up to the
//     first one whose identity is cached already (that tile and the later ones
//     stay private).  Generated tokens are not published;
//   * same step: admission ends before a head whose first uncached block will
//     be published by a request admitted earlier in this step.  The head is
//     not skipped; it enters at the next step with the hit (it was only
//     deferred when it fitted, and a step later it needs no more);
//   * pages: committed = the live requests' private needs + pages_per_tile
//     per used block; a request's private need is (serve_row_tiles(T) -
//     hit_blocks) * pages_per_tile, and a published tile moves its
//     pages_per_tile from the request to the block.  Idle blocks hold
//     idle_pages.  Invariant, always: committed + idle_pages <= num_pages --
//     every allocated page is a live row's private page, a used block's or an
//     idle block's, so an admitted request never meets an empty pool;
//   * admission of the head: its hit blocks become used (the idle ones move
//     their pages from idle to committed) and its private need is added; it
//     enters if committed <= num_pages then -- every other idle block can be
//     evicted, leaf first -- else it waits with nothing changed; idle blocks
//     without a cached child are then evicted, least recently used first,
//     until the invariant holds.  The evicted blocks' pages are the caller's
//     to drop (evictions());
//   * retirement / cancel: the private need returns, each used block loses a
//     user; a block without users is idle and most recently used.
#pragma once

#include <algorithm>
#include <deque>
#include <utility>
#include <vector>

#include "prefix_cache.hpp"

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
  long long need = 0;  // pages charged to it (prefix caching: its private need)
  int delivered = 0;  // tokens handed out so far
  // prefix caching only: the prompt (the caller's, valid while the request is
  // waiting or live), the blocks it hit and the chain it uses (hit, then published)
  const int32_t* tokens = nullptr;
  int hit_blocks = 0;
  std::vector<int> blocks;
  long long committed_after = 0;  // the pages committed right after its admission
};

// An evicted block: its id and tile index (for the records) and the pages the
// caller returns to the pool.
struct ServeEvict {
  int block, depth;
  std::vector<int32_t> pages;
};

// Counters of a prefix-caching session (zeros without one).
struct ServePrefixStats {
  long long due = 0;        // prompt positions due: the sum of n - 1 over admitted requests
  long long hit = 0;        // ... of which served from cached blocks
  long long evicted = 0;    // blocks evicted
  long long deferrals = 0;  // admissions ended by the same-step rule
};

// A row re-parented at a retirement: what row `src` (the last live row) held
// is row `dst` from now on.
struct ServeMove {
  int dst, src;
};

class ServePlan {
 public:
  void begin(const ServeGeom& g, bool prefix_cache = false) {
    geom_ = g;
    waiting_.clear();
    live_.clear();
    committed_ = 0;
    next_id_ = 0;
    cache_ = prefix_cache;
    index_.begin(g.page_size, g.pages_per_tile);
    evictions_.clear();
    stats_ = ServePrefixStats();
    deferred_ = -1;
  }

  const ServeGeom& geom() const { return geom_; }
  int live() const { return (int)live_.size(); }
  int waiting() const { return (int)waiting_.size(); }
  long long committed() const { return committed_; }
  const PrefixIndex& index() const { return index_; }
  long long idle_pages() const { return (long long)index_.idle_blocks() * geom_.pages_per_tile; }
  const ServePrefixStats& prefix_stats() const { return stats_; }
  // The head the last admit() deferred by the same-step rule, or -1.
  long long deferred() const { return deferred_; }
  // The blocks evicted since the caller last cleared the list.
  std::vector<ServeEvict>& evictions() { return evictions_; }
  const ServeReq& row(int r) const { return live_[r]; }
  ServeReq& row(int r) { return live_[r]; }

  // Whether a request of this shape can ever be served by the geometry.
  bool fits(int prompt_len, int max_new) const {
    return prompt_len >= 1 && max_new >= 1 &&
           serve_positions(prompt_len, max_new) <= geom_.max_seq_len &&
           serve_need(geom_, prompt_len, max_new) <= geom_.num_pages;
  }

  // Queue a request; its id, or -1 if it is refused (fits).  Prefix caching
  // needs the prompt's prompt_len ids (see ServeReq::tokens).
  long long submit(int prompt_len, int max_new, const int32_t* tokens = nullptr) {
    if (!fits(prompt_len, max_new) || (cache_ && !tokens)) return -1;
    ServeReq q;
    q.id = next_id_++;
    q.prompt_len = prompt_len;
    q.max_new = max_new;
    q.need = serve_need(geom_, prompt_len, max_new);
    q.tokens = cache_ ? tokens : nullptr;
    waiting_.push_back(q);
    return q.id;
  }

  // Start of a step: the head of the queue enters row `live` while it fits.
  // Returns the number admitted (rows live - n .. live - 1, in id order).
  int admit() {
    deferred_ = -1;
    if (cache_) return admit_cached();
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
    for (int b : live_[r].blocks)
      if (index_.release(b)) committed_ -= geom_.pages_per_tile;
    const bool moved = r != last;
    if (moved) {
      live_[r] = live_[last];
      *mv = ServeMove{r, last};
    }
    live_.pop_back();
    return moved;
  }

  // Prefix caching, after the admission prefill of live row r: publish the
  // full tiles it computed.  hold(tile, pages) takes the references that keep
  // the tile's pages_per_tile pages (written to pages, layer-major) beyond the
  // row and returns non-zero on failure, which stops the walk and is returned
  // (the plan is then in no defined state).
  template <typename Hold>
  int publish(int r, Hold&& hold) {
    if (!cache_) return 0;
    ServeReq& q = live_[r];
    const int P = geom_.page_size, max_hit = (q.prompt_len - 1) / P;
    int parent = q.blocks.empty() ? -1 : q.blocks.back();
    for (int k = (int)q.blocks.size(); k < max_hit; ++k) {
      const int32_t* tok = q.tokens + (size_t)k * P;
      if (index_.find(parent, tok) >= 0) break;  // cached already: this tile stays private
      const int b = index_.insert(parent, tok);
      q.need -= geom_.pages_per_tile;  // ... which the block holds from now: committed_ is unchanged
      q.blocks.push_back(b);
      parent = b;
      if (int rc = hold(k, index_.pages(b))) return rc;
    }
    return 0;
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
  // Whether one of the n requests admitted in this step (the last n live
  // rows) will publish block h of q's prompt: it computes that tile itself
  // and its prompt agrees with q's up to the tile's end.
  bool published_this_step(int n, const ServeReq& q, int h) const {
    const int P = geom_.page_size;
    for (int r = live() - n; r < live(); ++r) {
      const ServeReq& e = live_[r];
      if (h < e.hit_blocks || h >= (e.prompt_len - 1) / P) continue;
      if (std::equal(q.tokens, q.tokens + (size_t)(h + 1) * P, e.tokens)) return true;
    }
    return false;
  }

  int admit_cached() {
    const int P = geom_.page_size;
    const long long ppt = geom_.pages_per_tile;
    int n = 0;
    while (!waiting_.empty() && live() < geom_.max_rows) {
      ServeReq& q = waiting_.front();
      const int max_hit = (q.prompt_len - 1) / P;
      index_.longest_chain(q.tokens, max_hit, &chain_);
      const int h = (int)chain_.size();
      long long idle_hits = 0;
      for (int b : chain_) idle_hits += index_.block(b).users == 0;
      const long long priv =
          (serve_row_tiles(geom_, serve_positions(q.prompt_len, q.max_new)) - h) * ppt;
      // with its hit blocks used, is there room once every other idle block is gone?
      if (committed_ + idle_hits * ppt + priv > geom_.num_pages) break;
      if (h < max_hit && published_this_step(n, q, h)) {
        deferred_ = q.id;
        ++stats_.deferrals;
        break;
      }
      for (int b : chain_) index_.use(b);
      committed_ += idle_hits * ppt + priv;
      while (committed_ + idle_pages() > geom_.num_pages) {
        const int v = index_.victim();
        if (v < 0) break;  // (not reached: an idle block implies an idle block without a child)
        evictions_.push_back(ServeEvict{v, index_.block(v).depth, {}});
        index_.erase(v, &evictions_.back().pages);
        ++stats_.evicted;
      }
      q.need = priv;
      q.hit_blocks = h;
      q.blocks = chain_;
      q.committed_after = committed_;
      stats_.due += q.prompt_len - 1;
      stats_.hit += (long long)h * P;
      live_.push_back(std::move(q));
      waiting_.pop_front();
      ++n;
    }
    return n;
  }

  ServeGeom geom_;
  std::deque<ServeReq> waiting_;
  std::vector<ServeReq> live_;
  std::vector<int> fin_;  // finish_step: the rows' finish reasons
  long long committed_ = 0, next_id_ = 0;
  // prefix caching
  bool cache_ = false;
  PrefixIndex index_;
  std::vector<int> chain_;  // admit_cached: the head's hit chain
  std::vector<ServeEvict> evictions_;
  ServePrefixStats stats_;
  long long deferred_ = -1;
};

}  // namespace llm
