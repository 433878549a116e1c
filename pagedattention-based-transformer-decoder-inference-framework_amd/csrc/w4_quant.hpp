// Host reader of the W4 device layout (csrc/w4_quant.cpp), for the decoder's
// llm_decoder_expanded_weights.
#pragma once

#include <cstdint>

namespace llm {

// P: a host copy of w4_pack_weights' output for [K][N]; W8: int8 [K][N], the
// weights the packed set equals (q * multiplier).
void w4_unpack_host(const uint8_t* P, int K, int N, int8_t* W8);

}  // namespace llm
