// W4A8 weight GEMM on gfx950 MFMA: 4-bit weights with an integer multiplier
// per (128-input group, column), int8 activations, exact int32 sums and the
// i8_gemm epilogue (w4_gemm, w4_pack_weights; the decoder's w4_weight_gemm).
//
// Format (include/llm_decoder.h): w8[k][n] = q[k][n] * mul[k / 128][n] with q
// in [-7, 7] and mul in [1, 18], so the expanded weight is an ordinary int8
// and the k loop stays on v_mfma_i32_16x16x64_i8.  The result equals i8_gemm
// on the expanded weights in every bit, while the launch streams 0.508 of the
// bytes.
//
// Packed layout (w4_pack_weights), for ntiles = N / 16 column tiles and
// G = K / 128 groups:
//   * nibbles: one contiguous 1 KiB block per (column tile, group), block
//     (nt, g) at (nt G + g) * 1024.  Lane l's 16 bytes hold its B operands of
//     BOTH k-steps of the group (column nt 16 + (l & 15), k-lane group l >> 4):
//     byte i = q[128 g + 16 (l >> 4) + i] in the low nibble and
//     q[128 g + 64 + 16 (l >> 4) + i] in the high nibble.  One coalesced
//     buffer_load_dwordx4 per lane carries 32 weights.
//   * multipliers, after the nibbles (at ntiles G 1024): 16 bytes per (column
//     tile, group), byte c = mul[g][nt 16 + c].  A lane reads its own column's
//     byte; the 64 lanes of a wave read 16 consecutive bytes.
// Unpacking: with w one dword of the lane's 16 bytes,
//   (w << 4) & 0xF0F0F0F0   four int8 lanes holding 16 q of the first k-step
//   w & 0xF0F0F0F0          four int8 lanes holding 16 q of the second
// (a 4-bit two's complement value in the top nibble of a byte IS 16 q as an
// int8: no sign extension).  Two VALU operations per eight weights, and the
// four dwords of each mask are a whole MFMA B operand, in the k order of the
// A fragments (common.hpp a_frag_off_i8).
// Per group: a fresh int32 accumulator takes the two MFMAs (|sum| <= 128 * 128
// * 7 * 16 < 2^21), then acc += (sum >> 4) * mul per accumulator register: the
// sum is a multiple of 16, so the shift is exact, and the running sum carries
// no factor of 16 (|acc| <= K * 128 * 126 < 2^31 for K < 131072).  In the
// 16x16 output layout a lane holds one column (lane & 15), so one multiplier
// per lane, group and column tile.
//
// Work split: as the int8 GEMM (gemm_impl.hpp), a 512-thread workgroup owns NT
// column tiles x 16 MT rows and its 8 waves split the groups; every wave keeps
// two batches of groups in flight, the partial sums meet in LDS in a fixed
// order, and the dequant / bias / activation epilogue writes fp32.  Decode
// rows (<= 64) are 1, 2 or 4 row tiles held in registers; more rows (prefill
// chunks) are 64-row blocks over gridDim.y, each streaming the weights.
#include "common.hpp"
#include "gemm_w4.hpp"

using namespace llm;

namespace {

constexpr int kW4Group = 128;  // inputs per multiplier
constexpr int kW4Waves = 8;

struct W4Args {
  const uint8_t* A;
  int lda;
  int a_packed;
  const uint8_t* B;    // packed nibbles
  const uint8_t* mul;  // packed multipliers
  int M, N, K, G;      // G = K / 128
  const float* sa;
  const float* sw;
  const float* bias;
  int act;
  float* C;
  int c_ld;
  int32_t* acc_out;
  int w_keep;
};

__device__ __forceinline__ float w4_act(float y, int act) {
  if (act == LLM_ACT_RELU) return fmaxf(y, 0.f);
  if (act == LLM_ACT_GELU) return 0.5f * y * (1.f + erff(y * 0.70710678118654752f));
  return y;
}

// Groups per pipeline batch (two batches in flight per wave): bounded by the
// A fragments a group holds (2 k-steps x MT tiles x 4 VGPRs).
template <int MT, int NT>
constexpr int w4_unroll() {
  return MT * NT == 1 ? 4 : MT * NT == 2 ? 2 : 1;
}

template <int MT, int NT>
__global__ __launch_bounds__(kW4Waves * 64) void w4_gemm_kernel(W4Args a) {
  constexpr int WAVES = kW4Waves;
  constexpr int U = w4_unroll<MT, NT>();
  // Cross-wave partial sums, [wave][tile][reg][lane]: lane-fastest, so the
  // per-register stores and the epilogue's reads are bank-conflict free.
  __shared__ int32_t red[WAVES][MT * NT][4][64];

  const int lane = lane_id();
  const int w = wave_id_uniform();
  const int bx = blockIdx.x;
  const int nt0 = bx * NT;
  const int m0 = blockIdx.y * 16 * MT;
  const int ntiles = a.N >> 4;
  const int ntl = min(NT, ntiles - nt0);  // column tiles this workgroup has
  const int G = a.G;
  const int KS = 2 * G;  // 64-wide k-steps of A
  // wave w streams group range (w + bx) % WAVES: the workgroups of an XCD read
  // different A fragments at any moment (gemm_impl.hpp)
  const int wr = (w + bx) % WAVES;
  const int g0 = (wr * G) / WAVES;
  const int g1 = ((wr + 1) * G) / WAVES;

  // A: rows >= M and anything past the matrix read as zero (buffer bounds)
  const int arow_lane = lane & 15;
  const int kgrp = lane >> 4;
  const bool apk = a.a_packed;
  const uint32_t a_bytes = apk ? (uint32_t)(((a.M + 15) / 16) * KS) * 1024u
                               : (uint32_t)((size_t)a.M * a.lda);
  const auto arsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.A, (short)0, a_bytes, 0x00020000);
  const uint32_t a_kstride = apk ? 1024u : 64u;
  const uint32_t a_kgrp_off = apk ? 0u : (uint32_t)(kgrp * 16);
  uint32_t a_row_off[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int row = m0 + mt * 16 + arow_lane;
    a_row_off[mt] = row >= a.M ? 0xFFFFFFF0u
                    : apk      ? (uint32_t)(((m0 >> 4) + mt) * KS) * 1024u + lane * 16
                               : (uint32_t)((size_t)row * a.lda);
  }
  // B and the multipliers: this workgroup's column tiles only
  const auto brsrc = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(a.B + (size_t)nt0 * G * 1024), (short)0, (uint32_t)(ntl * G) * 1024u, 0x00020000);
  const auto mrsrc = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(a.mul + (size_t)nt0 * G * 16), (short)0, (uint32_t)(ntl * G) * 16u, 0x00020000);

  i32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[mt][j] = i32x4{0, 0, 0, 0};

  struct Batch {
    u32x4 b[U][NT];
    int mu[U][NT];
    u32x4 af[U][2][MT];
  };
  auto issue = [&](Batch& bt, int g) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int gg = g + u;
      const bool ok = gg < g1;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const bool okj = ok && j < ntl;
        const uint32_t boff = okj ? (uint32_t)(j * G + gg) * 1024u + lane * 16 : 0xFFFFFFF0u;
        bt.b[u][j] = a.w_keep ? __builtin_amdgcn_raw_buffer_load_b128(brsrc, boff, 0, 0)
                              : __builtin_amdgcn_raw_buffer_load_b128(brsrc, boff, 0, 2);
        const uint32_t moff = okj ? (uint32_t)(j * G + gg) * 16u + (lane & 15) : 0xFFFFFFF0u;
        bt.mu[u][j] = (int)__builtin_amdgcn_raw_buffer_load_b8(mrsrc, moff, 0, 0);
      }
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const uint32_t koff = (uint32_t)(2 * gg + s) * a_kstride + a_kgrp_off;
          const uint32_t aoff =
              (ok && a_row_off[mt] != 0xFFFFFFF0u) ? a_row_off[mt] + koff : 0xFFFFFFF0u;
          bt.af[u][s][mt] = __builtin_amdgcn_raw_buffer_load_b128(arsrc, aoff, 0, 0);
        }
    }
  };
  auto compute = [&](const Batch& bt) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        u32x4 lo, hi;  // 16 q of the group's first / second k-step
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          lo[d] = (bt.b[u][j][d] << 4) & 0xF0F0F0F0u;
          hi[d] = bt.b[u][j][d] & 0xF0F0F0F0u;
        }
        const int mu = bt.mu[u][j];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          i32x4 p = __builtin_amdgcn_mfma_i32_16x16x64_i8(
              __builtin_bit_cast(i32x4, bt.af[u][0][mt]), __builtin_bit_cast(i32x4, lo),
              i32x4{0, 0, 0, 0}, 0, 0, 0);
          p = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, bt.af[u][1][mt]),
                                                    __builtin_bit_cast(i32x4, hi), p, 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[mt][j][r] += (p[r] >> 4) * mu;
        }
      }
    }
  };

  // Epilogue operands are independent of the accumulators: loaded before the
  // k loop, their round trips overlap the weight stream.  Thread t owns
  // outputs t, t + NTHR, ... (column fastest).
  constexpr int ROWS = 16 * MT, COLS = 16 * NT, NTHR = WAVES * 64;
  constexpr int EPT = (ROWS * COLS + NTHR - 1) / NTHR;
  float e_scale[EPT], e_bias[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int o = threadIdx.x + e * NTHR;
    const int m = m0 + o / COLS;
    const int n = nt0 * 16 + o % COLS;
    const bool valid = o < ROWS * COLS && m < a.M && n < a.N;
    e_scale[e] = 1.f;
    if (valid && a.sa) e_scale[e] *= a.sa[m];
    if (valid && a.sw) e_scale[e] *= a.sw[n];
    e_bias[e] = valid && a.bias ? a.bias[n] : 0.f;
  }

  {
    Batch b0, b1;
    int g = g0;
    if (g < g1) issue(b0, g);
    while (g < g1) {
      if (g + U < g1) issue(b1, g + U);
      compute(b0);
      g += U;
      if (g >= g1) break;
      if (g + U < g1) issue(b0, g + U);
      compute(b1);
      g += U;
    }
  }

#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wr][mt * NT + j][r][lane] = acc[mt][j][r];
  __syncthreads();

#pragma unroll
  for (int e = 0; e < EPT; ++e) {
#pragma clang fp contract(off)  // y = acc * scale + bias rounded twice, as i8_gemm
    const int o = threadIdx.x + e * NTHR;
    if (o >= ROWS * COLS) break;
    const int cl = o % COLS;
    const int row = o / COLS;
    const int j = cl >> 4;
    const int col = cl & 15;
    const int mt = row >> 4;
    const int rl = row & 15;
    // C/D layout of the MFMA: column = lane & 15, row = 4 (lane >> 4) + reg
    const int src_lane = (rl >> 2) * 16 + col;
    const int reg = rl & 3;
    const int m = m0 + row;
    const int n = (nt0 + j) * 16 + col;
    if (m >= a.M || n >= a.N) continue;
    int32_t s = 0;
#pragma unroll
    for (int ww = 0; ww < WAVES; ++ww) s += red[ww][mt * NT + j][reg][src_lane];
    if (a.acc_out) a.acc_out[(size_t)m * a.N + n] = s;
    if (!a.C) continue;
    float y = (float)s * e_scale[e];
    if (a.bias) y = y + e_bias[e];
    a.C[(size_t)m * a.c_ld + n] = w4_act(y, a.act);
  }
}

// Interchange layout (q uint8 [K / 2][N], even k in the low nibble; mul uint8
// [K / 128][N]) -> the packed layout above.  One thread per lane chunk.
__global__ void w4_pack_kernel(const uint8_t* __restrict__ q, const uint8_t* __restrict__ mul,
                               uint8_t* __restrict__ P, int N, int G, int ntiles) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)ntiles * G * 64;
  if (idx >= total) return;
  const int lane = idx & 63;
  const size_t blk = idx >> 6;
  const int g = blk % G;
  const int nt = blk / G;
  const int n = nt * 16 + (lane & 15);
  const int kb = g * kW4Group + (lane >> 4) * 16;
  auto nib = [&](int k) -> uint32_t {
    return (q[(size_t)(k >> 1) * N + n] >> ((k & 1) * 4)) & 0xFu;
  };
  u32x4 out;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int k = kb + 4 * d + b;
      v |= (nib(k) | (nib(k + 64) << 4)) << (8 * b);
    }
    out[d] = v;
  }
  *reinterpret_cast<u32x4*>(P + idx * 16) = out;
  if (lane < 16) P[total * 16 + blk * 16 + lane] = mul[(size_t)g * N + n];
}

// The launch form, by shape: rows per workgroup 16 / 32 / 64 (more rows: 64-row
// blocks over gridDim.y); 32-row blocks at 33..64 rows when the column grid
// alone cannot fill the CUs (the second block re-reads the weights from L2 /
// the Infinity Cache, as the int8 GEMM does); two column tiles per workgroup
// (A fragments shared) at 17..32 rows when that still leaves >= 192 workgroups
// (four row tiles x two column tiles would not fit the register file).
struct W4Form {
  int mt, nt;
};
W4Form w4_form(int M, int N) {
  const int ntiles = N / 16;
  int mrows = M <= 16 ? 16 : M <= 32 ? 32 : 64;
  const int mblocks = (M + mrows - 1) / mrows;
  const int nt = (mrows == 32 && ntiles % 2 == 0 && (ntiles / 2) * mblocks >= 192) ? 2 : 1;
  if (mrows == 64 && M <= 64 && nt == 1 && ntiles < 256) mrows = 32;
  return W4Form{mrows / 16, nt};
}

template <int MT, int NT>
hipError_t w4_launch(const W4Args& a, hipStream_t st) {
  const int ntiles = a.N / 16;
  const dim3 grid((ntiles + NT - 1) / NT, (a.M + 16 * MT - 1) / (16 * MT));
  hipLaunchKernelGGL((w4_gemm_kernel<MT, NT>), grid, dim3(kW4Waves * 64), 0, st, a);
  return hipGetLastError();
}

}  // namespace

extern "C" size_t w4_packed_bytes(int K, int N) {
  if (K <= 0 || N <= 0 || K % kW4Group != 0 || N % 16 != 0) return 0;
  return (size_t)(N / 16) * (K / kW4Group) * (1024 + 16);
}

extern "C" int w4_pack_weights(const uint8_t* q, const uint8_t* m, void* W_packed, int K, int N,
                               void* stream) {
  LLM_REQUIRE(q && m && W_packed, "w4_pack_weights: NULL operand");
  LLM_REQUIRE(K > 0 && K % kW4Group == 0 && K < 131072,
              "w4_pack_weights: K must be a multiple of 128 below 131072");
  LLM_REQUIRE(N > 0 && N % 16 == 0, "w4_pack_weights: N must be a multiple of 16");
  const int G = K / kW4Group, ntiles = N / 16;
  const size_t total = (size_t)ntiles * G * 64;
  hipLaunchKernelGGL(w4_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     as_stream(stream), q, m, static_cast<uint8_t*>(W_packed), N, G, ntiles);
  LLM_HIP_RET(hipGetLastError());
  return LLM_OK;
}

int llm::w4_weight_gemm(const W4Gemm& g, hipStream_t st) {
  LLM_REQUIRE(g.M >= 0 && g.N > 0 && g.K > 0, "w4_gemm: bad M/N/K");
  if (g.M == 0) return LLM_OK;
  LLM_REQUIRE(g.A && g.W_packed, "w4_gemm: NULL operand");
  LLM_REQUIRE(g.K % kW4Group == 0 && g.K < 131072,
              "w4_gemm: K must be a multiple of 128 below 131072");
  LLM_REQUIRE(g.N % 16 == 0, "w4_gemm: N must be a multiple of 16");
  LLM_REQUIRE(g.act >= 0 && g.act <= 2, "w4_gemm: bad activation");
  const int G = g.K / kW4Group;
  if (g.a_packed) {
    LLM_REQUIRE((size_t)((g.M + 15) / 16) * 2 * G * 1024 < (1ull << 32), "w4_gemm: A too large");
  } else {
    LLM_REQUIRE(g.lda >= g.K && g.lda % 16 == 0,
                "w4_gemm: lda must be >= K and a multiple of 16");
    LLM_REQUIRE((size_t)g.M * g.lda < (1ull << 31), "w4_gemm: A too large");
  }
  LLM_REQUIRE(g.c_ld == 0 || g.c_ld >= g.N, "w4_gemm: c_ld must be >= N");
  W4Args a{};
  a.A = reinterpret_cast<const uint8_t*>(g.A);
  a.lda = g.lda;
  a.a_packed = g.a_packed ? 1 : 0;
  a.B = static_cast<const uint8_t*>(g.W_packed);
  a.mul = a.B + (size_t)(g.N / 16) * G * 1024;
  a.M = g.M; a.N = g.N; a.K = g.K; a.G = G;
  a.sa = g.sa; a.sw = g.sw; a.bias = g.bias; a.act = g.act;
  a.C = g.C; a.c_ld = g.c_ld > 0 ? g.c_ld : g.N;
  a.acc_out = g.acc_out;
  a.w_keep = g.w_keep;
  const W4Form f = w4_form(g.M, g.N);
  hipError_t e;
  if (f.nt == 2)
    e = w4_launch<2, 2>(a, st);
  else
    e = f.mt == 1 ? w4_launch<1, 1>(a, st) : f.mt == 2 ? w4_launch<2, 1>(a, st)
                                                       : w4_launch<4, 1>(a, st);
  if (e != hipSuccess) return fail(LLM_ERR_HIP, std::string("w4_gemm: ") + hipGetErrorString(e));
  return LLM_OK;
}

extern "C" int w4_gemm(const int8_t* A, int lda, int a_packed, const void* W_packed,
                       int32_t* acc_out, float* C, int M, int N, int K, const float* sa,
                       const float* sw, const float* bias, int act, void* stream) {
  W4Gemm g;
  g.A = A; g.lda = lda; g.a_packed = a_packed; g.W_packed = W_packed;
  g.M = M; g.N = N; g.K = K;
  g.sa = sa; g.sw = sw; g.bias = bias; g.act = act;
  g.C = C; g.acc_out = acc_out;
  return w4_weight_gemm(g, as_stream(stream));
}
