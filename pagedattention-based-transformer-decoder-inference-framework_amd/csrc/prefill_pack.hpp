// Chunked prefill: the pass packer.  Host-only and pure (no HIP headers, no
// decoder state): the prompts of some rows in, the layer passes that prefill
// them out (decoder_prefill.cpp prefill_run runs them; prefill_passes_tune is
// the test entry).
#pragma once

#include <algorithm>
#include <vector>

namespace llm {

// `len` tokens of input row `src` (an index into the packer's arrays), at
// positions p0 .. p0 + len - 1 of that row.
struct PrefillSeg {
  int src, p0, len;
};
using PrefillPass = std::vector<PrefillSeg>;

// Row i holds len[i] tokens from position start[i] on.  A pass is up to `cap`
// tokens, filled greedily in row order: a row that does not fit continues in
// the next pass at its new position, so a row is in a pass at most once, and
// every pass but the last holds exactly cap tokens.  Rows of length 0 add
// nothing; a one-row prefill is one segment per pass.
inline std::vector<PrefillPass> prefill_passes(const int* start, const int* len, int nrows,
                                               int cap) {
  std::vector<PrefillPass> passes;
  int room = 0;  // of the last pass
  for (int i = 0; i < nrows && cap > 0; ++i)
    for (int done = 0; done < len[i];) {
      if (room == 0) {
        passes.emplace_back();
        room = cap;
      }
      const int n = std::min(len[i] - done, room);
      passes.back().push_back(PrefillSeg{i, start[i] + done, n});
      done += n;
      room -= n;
    }
  return passes;
}

}  // namespace llm
