// Prefix caching while serving: the index of cached prompt blocks.  Host-only
// and pure (no HIP headers, no decoder state), like serve_plan.hpp, whose
// ServePlan owns one PrefixIndex and does the page accounting over it.
//
// A block is tile k of a prompt across all layers and heads: page_size
// positions, pages_per_tile pages.  Its identity is (its parent block, or the
// root for k = 0; its page_size token ids): token ids are compared for
// equality, the hash only narrows the candidates.  So a chain of blocks from
// the root spells a prompt prefix, and two prompts share a block exactly when
// they agree on every token up to its end.
//
// A block is `used` while a live request has its pages attached (users > 0),
// else idle.  A user of a block uses every ancestor of it, so an idle block's
// cached children are idle too, and among the idle blocks there is always one
// without a cached child: eviction takes those, least recently used first.
#pragma once

#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace llm {

struct PrefixBlock {
  int parent = -1;              // block id, -1: the root
  int depth = 0;                // its tile index k
  std::vector<int32_t> tokens;  // page_size ids
  std::vector<int32_t> pages;   // pages_per_tile ids, layer-major, head-minor
  int users = 0;                // live requests using it
  int children = 0;             // cached blocks whose parent it is
  long long stamp = 0;          // recency: when it last became idle
  bool cached = false;          // (a slot of blocks_ may be free)
};

class PrefixIndex {
 public:
  void begin(int page_size, int pages_per_tile) {
    P_ = page_size;
    ppt_ = pages_per_tile;
    blocks_.clear();
    free_slots_.clear();
    by_hash_.clear();
    cached_ = idle_ = 0;
    clock_ = 0;
  }

  int page_size() const { return P_; }
  int cached_blocks() const { return cached_; }
  int idle_blocks() const { return idle_; }
  const PrefixBlock& block(int b) const { return blocks_[b]; }

  // The cached child of `parent` (-1: the root) that holds these page_size
  // ids, or -1.
  int find(int parent, const int32_t* tok) const {
    auto range = by_hash_.equal_range(hash(parent, tok));
    for (auto it = range.first; it != range.second; ++it) {
      const PrefixBlock& b = blocks_[it->second];
      if (b.parent != parent) continue;
      bool same = true;
      for (int i = 0; i < P_ && same; ++i) same = b.tokens[i] == tok[i];
      if (same) return it->second;
    }
    return -1;
  }

  // The longest cached chain from the root along a prompt's tokens, at most
  // max_blocks long: its block ids into chain (cleared first).
  void longest_chain(const int32_t* tok, int max_blocks, std::vector<int>* chain) const {
    chain->clear();
    int parent = -1;
    for (int k = 0; k < max_blocks; ++k) {
      const int b = find(parent, tok + (size_t)k * P_);
      if (b < 0) break;
      chain->push_back(b);
      parent = b;
    }
  }

  // A new block under `parent` with one user; the caller fills pages(b).
  int insert(int parent, const int32_t* tok) {
    int b;
    if (free_slots_.empty()) {
      b = (int)blocks_.size();
      blocks_.emplace_back();
    } else {
      b = free_slots_.back();
      free_slots_.pop_back();
    }
    PrefixBlock& n = blocks_[b];
    n.parent = parent;
    n.depth = parent < 0 ? 0 : blocks_[parent].depth + 1;
    n.tokens.assign(tok, tok + P_);
    n.pages.assign((size_t)ppt_, -1);
    n.users = 1;
    n.children = 0;
    n.stamp = 0;
    n.cached = true;
    if (parent >= 0) ++blocks_[parent].children;
    by_hash_.emplace(hash(parent, tok), b);
    ++cached_;
    return b;
  }
  int32_t* pages(int b) { return blocks_[b].pages.data(); }

  // One user more; true if the block was idle.
  bool use(int b) {
    const bool was_idle = blocks_[b].users++ == 0;
    idle_ -= was_idle;
    return was_idle;
  }
  // One user less; true if the block became idle: most recently used from now.
  bool release(int b) {
    PrefixBlock& n = blocks_[b];
    if (--n.users > 0) return false;
    n.stamp = ++clock_;
    ++idle_;
    return true;
  }

  // The eviction candidate: idle, no cached child, least recently used; -1 if
  // no block is idle.
  int victim() const {
    int best = -1;
    for (int b = 0; b < (int)blocks_.size(); ++b) {
      const PrefixBlock& n = blocks_[b];
      if (!n.cached || n.users != 0 || n.children != 0) continue;
      if (best < 0 || n.stamp < blocks_[best].stamp) best = b;
    }
    return best;
  }

  // Forget idle, childless block b; its page ids move into *pages_out.
  void erase(int b, std::vector<int32_t>* pages_out) {
    PrefixBlock& n = blocks_[b];
    auto range = by_hash_.equal_range(hash(n.parent, n.tokens.data()));
    for (auto it = range.first; it != range.second; ++it)
      if (it->second == b) {
        by_hash_.erase(it);
        break;
      }
    if (n.parent >= 0) --blocks_[n.parent].children;
    pages_out->swap(n.pages);
    n.pages.clear();
    n.tokens.clear();
    n.cached = false;
    --cached_;
    --idle_;
    free_slots_.push_back(b);
  }

 private:
  size_t hash(int parent, const int32_t* tok) const {
    unsigned long long h = 1469598103934665603ULL ^ (unsigned long long)(parent + 1);
    for (int i = 0; i < P_; ++i) h = (h ^ (uint32_t)tok[i]) * 1099511628211ULL;
    return (size_t)h;
  }

  int P_ = 0, ppt_ = 0;
  std::vector<PrefixBlock> blocks_;
  std::vector<int> free_slots_;
  std::unordered_multimap<size_t, int> by_hash_;
  int cached_ = 0, idle_ = 0;
  long long clock_ = 0;
};

}  // namespace llm
