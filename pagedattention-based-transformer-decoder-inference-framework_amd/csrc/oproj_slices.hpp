// The fused o_proj's second copy of W_o (pa_split.hpp, PaRowOutputs::wo_heads):
// one head's rows of W_o regrouped so that a lane reads 8 consecutive k of one
// output column with a 16-byte load.  Host-only and pure (no HIP headers).
#pragma once

#include <cstddef>
#include <cstdint>

namespace llm {

// wo: fp16 bit patterns, row-major [H*D][o_n] (row k = h D + 8 kg + j, column n).
// out: [H][D/8][o_n][8], out[((h KG + kg) o_n + n) 8 + j] = wo[(h D + 8 kg + j) o_n + n].
// D must be a multiple of 8.
inline void oproj_head_slices(const uint16_t* wo, int H, int D, int o_n, uint16_t* out) {
  const int KG = D / 8;
  for (int h = 0; h < H; ++h)
    for (int kg = 0; kg < KG; ++kg)
      for (int n = 0; n < o_n; ++n)
        for (int j = 0; j < 8; ++j)
          out[(((size_t)h * KG + kg) * o_n + n) * 8 + j] = wo[(size_t)(h * D + 8 * kg + j) * o_n + n];
}

}  // namespace llm
