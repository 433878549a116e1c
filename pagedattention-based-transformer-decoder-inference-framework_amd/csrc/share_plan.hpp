// Shared-prefix decode attention: the planner.  Host-only and pure (no HIP
// headers, no decoder state), like serve_plan.hpp: the live rows' block chains
// in, disjoint groups of rows that attend to the same leading pages out, and
// the launch geometry of the group kernel (pa_shared.hip) for those groups.
// llm_decoder::serve_upload runs it when the rows changed; share_plan_sim_tune
// is the test entry.
//
// Grouping rule, fixed here:
//   * one level: a row joins at most one group, a group is >= 2 rows and one
//     shared length P >= min_pages, in tiles (pages per head);
//   * a candidate is a node of the prefix index -- block `b` at depth k of some
//     row's chain (ServeReq::blocks: block ids are unique per node, so two rows
//     holding b at depth k hold the same k + 1 leading tiles) -- with the rows
//     that hold it and whose position is at or past the candidate's end:
//     (k + 1) * page_size <= pos.  The shared tiles are then whole pages
//     strictly below every member's current position: nothing appends into
//     them, and every token of them is inside every member's context;
//   * greedy by saving: the candidate with the largest (G - 1) * P, the page
//     reads per head the group kernel saves over per-row scans, is taken, its
//     rows leave every other candidate, and the rule repeats while a candidate
//     of >= 2 rows is left.  Ties go to the deeper candidate, then to the one
//     whose first row is lowest, so the plan is a function of its input.
//     Greedy is not optimal over all partitions (rows that share a long header
//     pairwise and a short one together can be split either way); it is exact
//     for the serving shapes this is for: a few distinct headers, each shared
//     by many rows, where the largest saving is also the right first cut.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace llm {

struct ShareGroup {
  std::vector<int> rows;  // batch rows, ascending
  int tiles = 0;          // P: leading tiles the rows share
};

struct ShareRow {
  const int* blocks = nullptr;  // the row's chain: block id of tile k
  int nblocks = 0;
  int pos = 0;  // the position this step appends (context - 1)
};

inline long long share_saving(const ShareGroup& g) {
  return (long long)((int)g.rows.size() - 1) * g.tiles;
}

inline std::vector<ShareGroup> share_plan(const std::vector<ShareRow>& rows, int page_size,
                                          int min_pages) {
  std::vector<ShareGroup> out;
  const int n = (int)rows.size();
  if (min_pages <= 0 || page_size <= 0) return out;
  std::vector<char> taken(n, 0);
  for (;;) {
    ShareGroup best;
    for (int r = 0; r < n; ++r) {
      if (taken[r]) continue;
      const int kmax = std::min(rows[r].nblocks, rows[r].pos / page_size);
      for (int k = std::max(min_pages, 1) - 1; k < kmax; ++k) {
        // the candidate (block at depth k of row r), visited from its lowest row only
        ShareGroup c;
        c.tiles = k + 1;
        bool first = true;
        for (int s = 0; s < n && first; ++s) {
          if (taken[s] || rows[s].nblocks <= k || rows[s].blocks[k] != rows[r].blocks[k] ||
              rows[s].pos / page_size < k + 1)
            continue;
          if (s < r) first = false;
          c.rows.push_back(s);
        }
        if (!first || c.rows.size() < 2) continue;
        const long long sv = share_saving(c), bs = best.rows.empty() ? -1 : share_saving(best);
        if (sv > bs || (sv == bs && c.tiles > best.tiles)) best = c;
      }
    }
    if (best.rows.size() < 2) break;
    for (int r : best.rows) taken[r] = 1;
    out.push_back(best);
  }
  return out;
}

// ---------------------------------------------------------------------------
// The group kernel's launch: query tiles and the key split
// ---------------------------------------------------------------------------
constexpr int kShareQTile = 16;    // queries per workgroup (one MFMA column block)
constexpr int kShareWaves = 4;     // waves per workgroup, one 32-key block each per round
constexpr int kShareKeyBlock = 32;
constexpr int kShareMaxPre = 32;   // prefix partial slots per (row, head) at most
constexpr int kShareTargetWgs = 1024;  // 4 workgroups per CU (256 CUs)

struct ShareLaunch {
  int ntile = 0;  // query tiles: sum over groups of ceil(G / 16)
  int npre = 0;   // key splits = prefix partial slots per (row, head)
  int bps = 0;    // 32-key blocks per split
  bool operator==(const ShareLaunch& o) const {
    return ntile == o.ntile && npre == o.npre && bps == o.bps;
  }
};

// Groups are few and their prefix long, so the grid is filled from the key
// range: splits until ntile * H * npre reaches kShareTargetWgs workgroups, each
// split at least one round of the workgroup's waves (kShareWaves blocks), at
// most kShareMaxPre splits (the merge holds them beside the suffix splits).
// One (npre, bps) for the launch, from the longest group: a shorter group's
// later splits are empty and write the empty state (sentinel, 0, 0).
inline ShareLaunch share_launch(int ntile, int H, int max_tiles_shared, int page_size) {
  ShareLaunch s;
  s.ntile = ntile;
  if (ntile <= 0 || max_tiles_shared <= 0) return s;
  const int nblk = (max_tiles_shared * page_size + kShareKeyBlock - 1) / kShareKeyBlock;
  const int want = std::min(std::max(kShareTargetWgs / std::max(ntile * H, 1), 1), kShareMaxPre);
  int bps = (nblk + want - 1) / want;
  bps = std::max((bps + kShareWaves - 1) / kShareWaves * kShareWaves, kShareWaves);
  s.bps = bps;
  s.npre = (nblk + bps - 1) / bps;
  return s;
}

// The device tables of a plan, as one int32 image: tiles[ntile][4] = {first
// index into rows, queries (<= 16), P, 0}, then the member rows group after
// group (`rows`), then first_tile[B] (P for a grouped row, 0 for any other).
// Offsets in int32 units; tiles first, so it stays 16-byte aligned.
struct ShareTables {
  std::vector<int32_t> image;
  int rows_off = 0, first_off = 0, ntile = 0, max_tiles = 0;
};

inline ShareTables share_tables(const std::vector<ShareGroup>& groups, int B) {
  ShareTables t;
  int nrows = 0;
  for (const ShareGroup& g : groups) {
    t.ntile += ((int)g.rows.size() + kShareQTile - 1) / kShareQTile;
    nrows += (int)g.rows.size();
    t.max_tiles = std::max(t.max_tiles, g.tiles);
  }
  t.rows_off = 4 * t.ntile;
  t.first_off = t.rows_off + nrows;
  t.image.assign((size_t)t.first_off + B, 0);
  int ti = 0, ri = 0;
  for (const ShareGroup& g : groups) {
    const int G = (int)g.rows.size();
    for (int o = 0; o < G; o += kShareQTile, ++ti) {
      int32_t* e = &t.image[4 * (size_t)ti];
      e[0] = ri + o, e[1] = std::min(kShareQTile, G - o), e[2] = g.tiles, e[3] = 0;
    }
    for (int r : g.rows) {
      t.image[t.rows_off + ri++] = r;
      t.image[t.first_off + r] = g.tiles;
    }
  }
  return t;
}

// int32 capacity of any plan's image over B rows: <= B / 2 groups, <= B tiles.
inline size_t share_tables_cap(int B) { return (size_t)4 * B + B + B; }

}  // namespace llm
