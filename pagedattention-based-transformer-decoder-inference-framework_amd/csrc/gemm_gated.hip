// Gated MLP (SwiGLU / GeGLU) on gfx950 MFMA: one launch computes
//   H[m, n] = act(G[m, n]) * U[m, n],  G = x . W_gate (+ scales, bias),
//                                      U = x . W_up   (+ scales, bias)
// (i8_gemm_gated, f16_gemm_gated; the decoder's gated_gemm).
//
// Layout.  Both weight matrices are in gemm_pack_weights' layout, two buffers:
// per (16-column tile, k-step) one 1 KiB block in which lane l's 16 bytes are
// its MFMA B operand.  A is row-major or packed-A (common.hpp a_frag_off_*).
//
// Work split.  A workgroup owns 16 NT columns of `inter` and 16 MT rows, for
// BOTH matrices; its 8 waves split the k-steps (rotated by the column block,
// so the workgroups of an XCD read different A lines at any moment).  Per
// k-step a wave loads its MT A fragments once and feeds 2 NT MFMAs with each
// (gate tile and up tile): A bytes per weight byte are MT : 2 NT, half of what
// the same product costs as one [K][2 inter] GEMM with the same tile.  The k
// loop runs in batches of `unroll` k-steps, two batches in flight.  The
// waves' partial sums meet in LDS in a fixed order (deterministic, no atomics,
// no hand-off between workgroups); the thread that owns (m, n) then holds both
// sums and applies scales, biases, the activation and the product in
// registers.  The unactivated G and U never reach memory.
//
// Tile forms by row count (gated_form; nothing here is tuned by measurement,
// the rules follow the byte counts above and gemm_impl.hpp's findings):
//   M <= 16       16 rows x 1 column tile.  A is one fragment per k-step
//                 against two weight fragments already; a second column tile
//                 would halve the workgroups streaming weights (pick_nt's
//                 finding for the plain GEMM at <= 16 rows).
//   17 .. 32      32 rows x 2 column tiles while that leaves >= 256
//                 workgroups (one per CU), else 32 rows x 1.
//   33 ..         64 rows x 1 column tile, row blocks of 64 on grid.y (decode
//                 rows up to 64 are one block; a 512-row prefill chunk is 8,
//                 which re-read the weights from L2 / the Infinity Cache).
// The cross-wave sums take 8 waves x 2 matrices x MT NT KiB of static LDS,
// which bounds MT NT at 4 (64 KiB).
//
// RMSNorm prologue (gemm_gated_kernel<..., PRO = 1>; i8_gemm_gated_rms,
// f16_gemm_gated_rms, the decoder's norm 2 under LLM_NORM_RMS).  The workgroup
// normalises its 16 MT rows of fp32 x itself, one wave per row with two rows'
// loads in flight (ln_wave.hpp rms_wave_compute: the bits of the RMS launch),
// while its first two batches of gate / up weights are already in flight.  The
// result is an LDS image of A in FRAGMENT order: per (row tile, k-step) one
// 1 KiB block whose 16-byte slot s = row + 16 kgroup is lane s's MFMA operand,
// so a k-step's A fragment is one ds_read_b128 per lane and the image is
// exactly 16 MT K bytes (x2 for fp16) with no padding.  The row's wave writes
// dwords (int8) or 8 bytes (fp16) that land 4 lanes per slot, slots 256 bytes
// apart: unswizzled, all 64 lanes would hit 4 banks.  Slot rows are therefore
// XORed with (kgroup + 4 kstep) & 15 (frag_slot): the 16 (kstep, kgroup)
// pairs a wave store touches go to 16 different slots mod 16 -> 64 distinct
// banks, and a 16-lane read group (fixed kstep and kgroup) still reads 16
// distinct slots.  The I8 row scales sit behind the image and are folded into
// the dequantisation factors; the cross-wave sums reuse the image's LDS after
// the k loop.  Dynamic LDS = max(image + scales, sums) <= 160 KiB
// (gated_rms_lds_bytes); which rows take this form: gated_rms_fusable.
//
// Exactness.  I8: int32 accumulation is exact and order-free; acc_gate /
// acc_up return the sums.  The epilogue rounds every operation once, in the
// order written in gated_value (no contraction).  F16: fp32 MFMA accumulation,
// the 8 k ranges added in wave order.
#include <algorithm>
#include <string>

#include "common.hpp"
#include "gemm_gated.hpp"
#include "ln_wave.hpp"

using namespace llm;

namespace {

constexpr int kWaves = 8;

template <int DTYPE>
struct GatedTraits;
template <>
struct GatedTraits<LLM_I8> {
  static constexpr int KSTEP = 64, ESIZE = 1;
  using acc_t = i32x4;
  using elem_t = int32_t;
};
template <>
struct GatedTraits<LLM_F16> {
  static constexpr int KSTEP = 32, ESIZE = 2;
  using acc_t = f32x4;
  using elem_t = float;
};

struct GatedArgs {
  const uint8_t* A;
  int lda, a_packed;
  const uint8_t* Bg;
  const uint8_t* Bu;
  int M, N, K, KS;
  const float* sa;
  const float* swg;
  const float* swu;
  const float* bg;
  const float* bu;
  int mlp;
  float* H;
  _Float16* h16;
  int ks16;  // k-steps per row tile of the packed fp16 image: ceil(N / 32)
  int32_t* accg;
  int32_t* accu;
  int w_keep;
  // RMSNorm prologue (PRO = 1): A = RMSNorm(ln_x) built in LDS; A / sa unused
  const float* ln_x;  // [M][K] fp32
  const float* ln_g;  // [K]
  float ln_eps;
  uint8_t* act_out;   // optional: column block 0 stores the image (packed-A order)
  float* sa_out;      //   and the I8 row scales
};

// 16-byte slot of fragment lane (row rl, k group g) in the 1 KiB LDS block of
// k-step ks (file comment: the swizzle that keeps the prologue's stores and
// the k loop's reads free of bank conflicts)
__device__ __forceinline__ int frag_slot(int rl, int g, int ks) {
  return (rl ^ ((g + 4 * ks) & 15)) + 16 * g;
}

// RMSNorm (+ int8 quantisation) of the workgroup's 16 MT rows into the
// fragment-order LDS image (and the I8 row scales into sa_lds).  Rows past M
// become zeros.  K <= 2048: 8 float4 chunks per lane.
template <int DTYPE, int MT>
__device__ __forceinline__ void gated_rms_prologue(const GatedArgs& a, int m0, uint8_t* alds,
                                                   float* sa_lds) {
  constexpr int CPL = 8, ROWS = 16 * MT;
  const int lane = lane_id();
  const int w = wave_id_uniform();
  const int K = a.K, K4 = K >> 2, KS = a.KS;
  LnRow<CPL> gm;
  ln_wave_load(a.ln_g, K4, true, gm);
  for (int r0 = w; r0 < ROWS; r0 += 2 * kWaves) {
    LnRow<CPL> x[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int r = r0 + q * kWaves;
      const bool ok = r < ROWS && m0 + r < a.M;
      ln_wave_load(a.ln_x + (size_t)(ok ? m0 + r : 0) * K, K4, ok, x[q]);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int r = r0 + q * kWaves;
      if (r >= ROWS) break;
      const bool mok = m0 + r < a.M;
      const float am = rms_wave_compute(x[q], gm, K, a.ln_eps);
      uint8_t* tile = alds + (size_t)(r >> 4) * KS * 1024;
      const int rl = r & 15;
      if constexpr (DTYPE == LLM_I8) {
        const float scale = 127.f / (am + 1e-6f);
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
          const int c = 64 * j + lane;  // elements 4 c .. 4 c + 3: k-step c / 16, group c / 4 % 4
          if (c < K4)
            *reinterpret_cast<uint32_t*>(tile + (c >> 4) * 1024 +
                                         frag_slot(rl, (c >> 2) & 3, c >> 4) * 16 + (c & 3) * 4) =
                mok ? ln_quant4(x[q].v[j], scale) : 0u;
        }
        if (lane == 0) sa_lds[r] = mok ? 1.0f / scale : 0.f;
      } else {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
          const int c = 64 * j + lane;  // k-step c / 8, group c / 2 % 4
          if (c < K4)
            *reinterpret_cast<ln_f16x4*>(tile + (c >> 3) * 1024 +
                                         frag_slot(rl, (c >> 1) & 3, c >> 3) * 16 + (c & 1) * 8) =
                mok ? ln_half4(x[q].v[j]) : ln_f16x4{0, 0, 0, 0};
        }
      }
    }
  }
}

// k-steps per batch: a k-step holds MT + 2 NT fragments of 4 VGPRs, two
// batches are live
template <int MT, int NT>
constexpr int gated_unroll() {
  return MT + 2 * NT >= 6 ? 2 : 4;
}

// act(g) * u, every operation rounded once
__device__ __forceinline__ float gated_value(float g, float u, int mlp) {
#pragma clang fp contract(off)
  float a;
  if (mlp == LLM_MLP_GATED_GELU)
    a = 0.5f * g * (1.f + erff(g * 0.70710678118654752f));  // apply_act's GELU
  else
    a = g / (1.f + expf(-g));
  return a * u;
}

// PRO = 1: the RMSNorm prologue, a kernel of its own, so that every launch
// without it runs the code it ran before there was one.
template <int DTYPE, int MT, int NT, int PRO = 0>
__global__ __launch_bounds__(kWaves * 64) void gemm_gated_kernel(GatedArgs a) {
  using Tr = GatedTraits<DTYPE>;
  using acc_t = typename Tr::acc_t;
  using elem_t = typename Tr::elem_t;
  constexpr int KSTEP = Tr::KSTEP, ES = Tr::ESIZE;
  constexpr int U = gated_unroll<MT, NT>();
  // [wave][gate tiles | up tiles][reg][lane]: lane-fastest, conflict-free both ways
  using RedT = elem_t[2 * MT * NT][4][64];
  extern __shared__ __attribute__((aligned(16))) uint8_t gated_smem[];
  RedT* red;
  if constexpr (PRO == 0) {
    __shared__ elem_t red_static[kWaves][2 * MT * NT][4][64];
    red = red_static;
  } else {
    red = reinterpret_cast<RedT*>(gated_smem);  // over the A image once the k loop is done
  }
  uint8_t* alds = gated_smem;
  float* sa_lds = reinterpret_cast<float*>(gated_smem + (size_t)MT * a.KS * 1024);

  const int lane = lane_id();
  const int w = wave_id_uniform();
  const int bx = blockIdx.x;
  const int nt0 = bx * NT;
  const int m0 = blockIdx.y * 16 * MT;
  const int wr = (w + bx) % kWaves;  // this wave's k range
  const int ks0 = (wr * a.KS) / kWaves;
  const int ks1 = ((wr + 1) * a.KS) / kWaves;
  const int ntiles = (a.N + 15) >> 4;

  // A: rows >= M read as zero (offset past the descriptor's range)
  const int arow_lane = lane & 15;
  const int kgrp = lane >> 4;
  const bool apk = a.a_packed;
  const uint32_t a_bytes = apk ? (uint32_t)(((a.M + 15) / 16) * a.KS * 1024u)
                               : (uint32_t)((size_t)a.M * a.lda * ES);
  const auto arsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.A, (short)0, a_bytes, 0x00020000);
  const uint32_t a_kstride = apk ? 1024u : (uint32_t)(KSTEP * ES);
  const uint32_t a_kgrp_off = apk ? 0u : (uint32_t)(kgrp * (KSTEP / 4) * ES);
  uint32_t a_row_off[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int row = m0 + mt * 16 + arow_lane;
    a_row_off[mt] = row >= a.M ? 0xFFFFFFF0u
                    : apk ? (uint32_t)((((m0 >> 4) + mt) * a.KS) * 1024u + lane * 16)
                          : (uint32_t)((size_t)row * a.lda * ES);
  }
  // B: this workgroup's column tiles of each matrix; tiles past the last read as zero
  const size_t b_base = (size_t)nt0 * a.KS * 1024;
  const uint32_t b_bytes = (uint32_t)(min(NT, ntiles - nt0) * a.KS * 1024u);
  const auto grsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)(a.Bg + b_base), (short)0, b_bytes, 0x00020000);
  const auto ursrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)(a.Bu + b_base), (short)0, b_bytes, 0x00020000);

  acc_t accg[MT][NT], accu[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < NT; ++j) accg[mt][j] = accu[mt][j] = acc_t{0, 0, 0, 0};

  struct Batch {
    u32x4 g[U][NT], u[U][NT], af[U][MT];
  };
  // do_a / do_b: the prologue kernel issues a batch's weight loads before the
  // prologue and its (LDS) A fragments after it
  auto issue = [&](Batch& bt, int ks, bool do_a = true, bool do_b = true) {
#pragma unroll
    for (int s = 0; s < U; ++s) {
      const int kk = ks + s;
      const bool ok = kk < ks1;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        if (!do_b) break;
        const uint32_t off =
            ok ? ((uint32_t)j * a.KS + (uint32_t)kk) * 1024u + lane * 16 : 0xFFFFFFF0u;
        if (a.w_keep) {
          bt.g[s][j] = __builtin_amdgcn_raw_buffer_load_b128(grsrc, off, 0, 0);
          bt.u[s][j] = __builtin_amdgcn_raw_buffer_load_b128(ursrc, off, 0, 0);
        } else {  // nt: each weight byte is read once per step
          bt.g[s][j] = __builtin_amdgcn_raw_buffer_load_b128(grsrc, off, 0, 2);
          bt.u[s][j] = __builtin_amdgcn_raw_buffer_load_b128(ursrc, off, 0, 2);
        }
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        if (!do_a) break;
        if constexpr (PRO != 0) {
          bt.af[s][mt] = ok ? *reinterpret_cast<const u32x4*>(
                                  alds + (size_t)(mt * a.KS + kk) * 1024 +
                                  frag_slot(arow_lane, kgrp, kk) * 16)
                            : u32x4{0u, 0u, 0u, 0u};
          continue;
        }
        const uint32_t off = (ok && a_row_off[mt] != 0xFFFFFFF0u)
                                 ? a_row_off[mt] + (uint32_t)kk * a_kstride + a_kgrp_off
                                 : 0xFFFFFFF0u;
        bt.af[s][mt] = __builtin_amdgcn_raw_buffer_load_b128(arsrc, off, 0, 0);
      }
    }
  };
  // each A fragment feeds the gate tile's and the up tile's MFMA
  auto compute = [&](const Batch& bt) {
#pragma unroll
    for (int s = 0; s < U; ++s)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          if constexpr (DTYPE == LLM_I8) {
            const i32x4 af = __builtin_bit_cast(i32x4, bt.af[s][mt]);
            accg[mt][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(
                af, __builtin_bit_cast(i32x4, bt.g[s][j]), accg[mt][j], 0, 0, 0);
            accu[mt][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(
                af, __builtin_bit_cast(i32x4, bt.u[s][j]), accu[mt][j], 0, 0, 0);
          } else {
            const f16x8 af = __builtin_bit_cast(f16x8, bt.af[s][mt]);
            accg[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                af, __builtin_bit_cast(f16x8, bt.g[s][j]), accg[mt][j], 0, 0, 0);
            accu[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                af, __builtin_bit_cast(f16x8, bt.u[s][j]), accu[mt][j], 0, 0, 0);
          }
        }
  };

  // Epilogue operands do not depend on the sums: loaded before the k loop so
  // their round trips overlap the weight stream.  Thread t owns outputs
  // t, t + NTHR, ... (column fastest).
  constexpr int ROWS = 16 * MT, COLS = 16 * NT, NTHR = kWaves * 64;
  constexpr int EPT = (ROWS * COLS + NTHR - 1) / NTHR;
  float e_sg[EPT], e_su[EPT], e_bg[EPT], e_bu[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int o = threadIdx.x + e * NTHR;
    const int m = m0 + o / COLS;
    const int n = nt0 * 16 + o % COLS;
    const bool valid = o < ROWS * COLS && m < a.M && n < a.N;
    e_sg[e] = e_su[e] = 1.f;
    if constexpr (DTYPE == LLM_I8) {
      const float sa = valid && a.sa ? a.sa[m] : 1.f;
      e_sg[e] = valid && a.swg ? sa * a.swg[n] : sa;
      e_su[e] = valid && a.swu ? sa * a.swu[n] : sa;
    }
    e_bg[e] = valid && a.bg ? a.bg[n] : 0.f;
    e_bu[e] = valid && a.bu ? a.bu[n] : 0.f;
  }

  {
    Batch b0, b1;
    int ks = ks0;
    bool b1_pre = false;  // b1's weight loads already issued
    if constexpr (PRO != 0) {
      // the first two batches' weights are in flight while the prologue runs
      if (ks < ks1) issue(b0, ks, false, true);
      if (ks + U < ks1) {
        issue(b1, ks + U, false, true);
        b1_pre = true;
      }
      gated_rms_prologue<DTYPE, MT>(a, m0, alds, sa_lds);
      __syncthreads();
      if constexpr (DTYPE == LLM_I8) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) {  // the prologue's row scales into the dequant factors
          const int o = threadIdx.x + e * NTHR;
          if (o < ROWS * COLS) {
            e_sg[e] *= sa_lds[o / COLS];
            e_su[e] *= sa_lds[o / COLS];
          }
        }
      }
      if (a.act_out && bx == 0) {  // the image in packed-A order (unswizzled) + the scales
        for (int i = threadIdx.x; i < MT * a.KS * 64; i += NTHR) {
          const int blk = i >> 6, sl = i & 63;
          const int mt = blk / a.KS, kk = blk % a.KS;
          if (m0 + mt * 16 + (sl & 15) >= a.M) continue;
          *reinterpret_cast<u32x4*>(a.act_out +
                                    ((size_t)(((m0 >> 4) + mt) * a.KS + kk) * 64 + sl) * 16) =
              *reinterpret_cast<const u32x4*>(alds + (size_t)blk * 1024 +
                                              frag_slot(sl & 15, sl >> 4, kk) * 16);
        }
        if (DTYPE == LLM_I8 && a.sa_out && threadIdx.x < ROWS && m0 + (int)threadIdx.x < a.M)
          a.sa_out[m0 + threadIdx.x] = sa_lds[threadIdx.x];
      }
      if (ks < ks1) issue(b0, ks, true, false);
    } else {
      if (ks < ks1) issue(b0, ks);
    }
    while (ks < ks1) {
      if (ks + U < ks1) {
        issue(b1, ks + U, true, !b1_pre);
        b1_pre = false;
      }
      compute(b0);
      ks += U;
      if (ks >= ks1) break;
      if (ks + U < ks1) issue(b0, ks + U);
      compute(b1);
      ks += U;
    }
  }

  if constexpr (PRO != 0) __syncthreads();  // every wave is done with the A image
  // (a wave with no k-steps stores its zeros)
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        red[wr][mt * NT + j][r][lane] = accg[mt][j][r];
        red[wr][MT * NT + mt * NT + j][r][lane] = accu[mt][j][r];
      }
  __syncthreads();

#pragma unroll
  for (int e = 0; e < EPT; ++e) {
#pragma clang fp contract(off)  // acc * scale + bias rounded twice, as i8_gemm
    const int o = threadIdx.x + e * NTHR;
    if (o >= ROWS * COLS) break;
    const int cl = o % COLS;
    const int row = o / COLS;
    const int t = (row >> 4) * NT + (cl >> 4);  // (row tile, column tile)
    // C/D layout of the MFMA: col = lane & 15, row = 4 (lane >> 4) + reg
    const int src_lane = ((row & 15) >> 2) * 16 + (cl & 15);
    const int reg = row & 3;
    const int m = m0 + row;
    const int n = nt0 * 16 + cl;
    if (m >= a.M || n >= a.N) continue;
    elem_t sg = 0, su = 0;
#pragma unroll
    for (int ww = 0; ww < kWaves; ++ww) {
      sg += red[ww][t][reg][src_lane];
      su += red[ww][MT * NT + t][reg][src_lane];
    }
    float g, u;
    if constexpr (DTYPE == LLM_I8) {
      if (a.accg) a.accg[(size_t)m * a.N + n] = sg;
      if (a.accu) a.accu[(size_t)m * a.N + n] = su;
      g = (float)sg * e_sg[e];
      u = (float)su * e_su[e];
    } else {
      g = sg;
      u = su;
    }
    if (a.bg) g = g + e_bg[e];
    if (a.bu) u = u + e_bu[e];
    const float h = gated_value(g, u, a.mlp);
    if (a.H) a.H[(size_t)m * a.N + n] = h;
    if (a.h16) a.h16[a_frag_off_f16(m, n, a.ks16)] = (_Float16)h;
  }
}

// The tile form of a launch: 16 mt rows x 16 nt columns per workgroup (file
// comment: the reasoning by row count).
struct GatedForm {
  int mt, nt;
};
GatedForm gated_form(int M, int N) {
  if (M <= 16) return {1, 1};
  if (M > 32) return {4, 1};
  const int ntiles = (N + 15) / 16;
  return {2, (ntiles + 1) / 2 >= 256 ? 2 : 1};
}

// Dynamic LDS of the prologue kernel: the rows' fragment-order A image + row
// scales, or the cross-wave sums that reuse it, whichever is larger.
size_t gated_rms_lds_bytes(int dtype, int mt, int nt, int K) {
  const size_t img = (size_t)16 * mt * K * (dtype == LLM_I8 ? 1 : 2) + 16 * mt * 4;
  const size_t red = (size_t)kWaves * 2 * mt * nt * 4 * 64 * 4;
  return std::max(img, red);
}
constexpr size_t kGatedLdsMax = 160 * 1024;
// Every workgroup reads all of its rows' fp32 x, and a CU takes in L2-resident
// rows slowly (ln_fusable's finding for the weight GEMM).  Measured with this
// cap at 256 KiB (scripts/bench_rmsnorm.py, profiles/rmsnorm.json; K 2048,
// inter 5632, graph-replayed): 8 rows (128 KiB per workgroup) 17.2 us fused
// against 9.9 us for the RMS launch + the gated launch, 16 rows 20.2 / 10.9,
// 32 rows (256 KiB) 29.3 / 14.8, and the decode step 12-15 % slower at 8 / 16
// rows.  So the cap is ln_fusable's 64 KiB, below every measured loss; past it
// the RMS launch + the plain gated launch serve the rows.
constexpr size_t kGatedRmsRowBytes = 64 * 1024;

template <int DTYPE, int MT, int NT>
hipError_t launch_form(const GatedArgs& a, hipStream_t st) {
  const int ntiles = (a.N + 15) / 16;
  const dim3 grid((ntiles + NT - 1) / NT, (a.M + 16 * MT - 1) / (16 * MT));
  if (a.ln_x) {
    const size_t lds = gated_rms_lds_bytes(DTYPE, MT, NT, a.K);
    static bool attr = false;  // (per instantiation) more than the default 64 KiB
    if (!attr) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_gated_kernel<DTYPE, MT, NT, 1>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGatedLdsMax);
      attr = true;
    }
    hipLaunchKernelGGL((gemm_gated_kernel<DTYPE, MT, NT, 1>), grid, dim3(kWaves * 64), lds, st, a);
    return hipGetLastError();
  }
  hipLaunchKernelGGL((gemm_gated_kernel<DTYPE, MT, NT>), grid, dim3(kWaves * 64), 0, st, a);
  return hipGetLastError();
}

template <int DTYPE>
hipError_t launch_gated(const GatedArgs& a, hipStream_t st) {
  const GatedForm f = gated_form(a.M, a.N);
  if (f.mt == 1) return launch_form<DTYPE, 1, 1>(a, st);
  if (f.mt == 4) return launch_form<DTYPE, 4, 1>(a, st);
  return f.nt == 2 ? launch_form<DTYPE, 2, 2>(a, st) : launch_form<DTYPE, 2, 1>(a, st);
}

}  // namespace

// Rows whose norm 2 the gated kernel runs as its prologue: decode row counts
// (one row block; prompt chunks take the launch), K within the prologue's 8
// chunks per lane, the image within LDS for the form gated_form picks, and the
// fp32 rows a workgroup reads within kGatedRmsRowBytes.
bool llm::gated_rms_fusable(int dtype, int M, int N, int K) {
  if (dtype != LLM_I8 && dtype != LLM_F16) return false;
  const int kstep = dtype == LLM_I8 ? 64 : 32;
  if (M <= 0 || M > 64 || N <= 0 || K <= 0 || K % kstep != 0 || K > 2048) return false;
  const GatedForm f = gated_form(M, N);
  if ((size_t)16 * f.mt * K * sizeof(float) > kGatedRmsRowBytes) return false;
  return gated_rms_lds_bytes(dtype, f.mt, f.nt, K) <= kGatedLdsMax;
}

int llm::gated_gemm(const GatedGemm& g, hipStream_t st, const char* who_c) {
  const std::string who = who_c;
  LLM_REQUIRE(g.dtype == LLM_I8 || g.dtype == LLM_F16, who + ": dtype must be I8 or F16");
  LLM_REQUIRE(g.M >= 0 && g.N > 0 && g.K > 0, who + ": bad M/N/K");
  LLM_REQUIRE(g.mlp == LLM_MLP_GATED_SILU || g.mlp == LLM_MLP_GATED_GELU,
              who + ": activation must be LLM_MLP_GATED_SILU or LLM_MLP_GATED_GELU");
  if (g.M == 0) return LLM_OK;
  LLM_REQUIRE((g.A || (g.ln_x && g.ln_g)) && g.Wg_packed && g.Wu_packed, who + ": NULL operand");
  const bool i8 = g.dtype == LLM_I8;
  LLM_REQUIRE(i8 || (!g.acc_gate && !g.acc_up), who + ": the int32 sums exist for I8 only");
  const int kstep = i8 ? 64 : 32, es = i8 ? 1 : 2;
  if (g.K % kstep != 0 || g.N % 16 != 0)
    return fail(LLM_ERR_UNSUPPORTED, who + ": the packed weight layout needs K % " +
                                         std::to_string(kstep) + " == 0 and N % 16 == 0");
  const int KS = g.K / kstep;
  if (g.ln_x) {
    if (!gated_rms_fusable(g.dtype, g.M, g.N, g.K))
      return fail(LLM_ERR_UNSUPPORTED, who + ": these rows do not take the RMSNorm prologue "
                                             "(gated_rms_fusable: rmsnorm_quant, then the gated "
                                             "launch)");
  } else if (g.a_packed) {
    LLM_REQUIRE((size_t)((g.M + 15) / 16) * KS * 1024 < (1ull << 32), who + ": A too large");
  } else {
    LLM_REQUIRE(g.lda >= g.K && g.lda % (16 / es) == 0,
                who + ": lda must be >= K and a multiple of 16 bytes");
    LLM_REQUIRE((size_t)g.M * g.lda * es < (1ull << 31), who + ": A too large");
  }
  GatedArgs a{};
  a.A = static_cast<const uint8_t*>(g.A);
  a.lda = g.lda;
  a.a_packed = g.a_packed;
  a.Bg = static_cast<const uint8_t*>(g.Wg_packed);
  a.Bu = static_cast<const uint8_t*>(g.Wu_packed);
  a.M = g.M; a.N = g.N; a.K = g.K; a.KS = KS;
  a.sa = g.sa; a.swg = g.sw_gate; a.swu = g.sw_up; a.bg = g.b_gate; a.bu = g.b_up;
  a.mlp = g.mlp;
  a.H = g.H;
  a.h16 = static_cast<_Float16*>(g.H16);
  a.ks16 = (g.N + 31) / 32;
  a.accg = g.acc_gate; a.accu = g.acc_up;
  a.w_keep = g.w_keep;
  if (g.ln_x) {
    a.A = nullptr; a.sa = nullptr;
    a.ln_x = g.ln_x; a.ln_g = g.ln_g; a.ln_eps = g.ln_eps;
    a.act_out = static_cast<uint8_t*>(g.act_out);
    a.sa_out = g.sa_out;
  }
  const hipError_t e = i8 ? launch_gated<LLM_I8>(a, st) : launch_gated<LLM_F16>(a, st);
  if (e != hipSuccess) return fail(LLM_ERR_HIP, who + ": " + hipGetErrorString(e));
  return LLM_OK;
}

extern "C" int i8_gemm_gated(const int8_t* A, int lda, int a_packed, const void* Wg_packed,
                             const void* Wu_packed, int32_t* acc_gate, int32_t* acc_up, float* H,
                             void* H16, int M, int N, int K, const float* sa,
                             const float* sw_gate, const float* sw_up, const float* b_gate,
                             const float* b_up, int mlp, void* stream) {
  GatedGemm g;
  g.dtype = LLM_I8;
  g.A = A; g.lda = lda; g.a_packed = a_packed;
  g.Wg_packed = Wg_packed; g.Wu_packed = Wu_packed;
  g.M = M; g.N = N; g.K = K;
  g.sa = sa; g.sw_gate = sw_gate; g.sw_up = sw_up; g.b_gate = b_gate; g.b_up = b_up;
  g.mlp = mlp;
  g.H = H; g.H16 = H16; g.acc_gate = acc_gate; g.acc_up = acc_up;
  return gated_gemm(g, as_stream(stream), "i8_gemm_gated");
}

extern "C" int f16_gemm_gated(const void* A, int lda, int a_packed, const void* Wg_packed,
                              const void* Wu_packed, float* H, void* H16, int M, int N, int K,
                              const float* b_gate, const float* b_up, int mlp, void* stream) {
  GatedGemm g;
  g.dtype = LLM_F16;
  g.A = A; g.lda = lda; g.a_packed = a_packed;
  g.Wg_packed = Wg_packed; g.Wu_packed = Wu_packed;
  g.M = M; g.N = N; g.K = K;
  g.b_gate = b_gate; g.b_up = b_up;
  g.mlp = mlp;
  g.H = H; g.H16 = H16;
  return gated_gemm(g, as_stream(stream), "f16_gemm_gated");
}

extern "C" int i8_gemm_gated_rms(const float* x, const float* gamma, float eps,
                                 const void* Wg_packed, const void* Wu_packed, int32_t* acc_gate,
                                 int32_t* acc_up, float* H, void* H16, int M, int N, int K,
                                 const float* sw_gate, const float* sw_up, const float* b_gate,
                                 const float* b_up, int mlp, int8_t* a_out, float* sa_out,
                                 void* stream) {
  LLM_REQUIRE(eps > 0.f, "i8_gemm_gated_rms: eps must be > 0");
  LLM_REQUIRE(M <= 0 || (x && gamma), "i8_gemm_gated_rms: NULL operand");
  GatedGemm g;
  g.dtype = LLM_I8;
  g.ln_x = x; g.ln_g = gamma; g.ln_eps = eps; g.act_out = a_out; g.sa_out = sa_out;
  g.Wg_packed = Wg_packed; g.Wu_packed = Wu_packed;
  g.M = M; g.N = N; g.K = K;
  g.sw_gate = sw_gate; g.sw_up = sw_up; g.b_gate = b_gate; g.b_up = b_up;
  g.mlp = mlp;
  g.H = H; g.H16 = H16; g.acc_gate = acc_gate; g.acc_up = acc_up;
  return gated_gemm(g, as_stream(stream), "i8_gemm_gated_rms");
}

extern "C" int f16_gemm_gated_rms(const float* x, const float* gamma, float eps,
                                  const void* Wg_packed, const void* Wu_packed, float* H, void* H16,
                                  int M, int N, int K, const float* b_gate, const float* b_up,
                                  int mlp, void* a_out, void* stream) {
  LLM_REQUIRE(eps > 0.f, "f16_gemm_gated_rms: eps must be > 0");
  LLM_REQUIRE(M <= 0 || (x && gamma), "f16_gemm_gated_rms: NULL operand");
  GatedGemm g;
  g.dtype = LLM_F16;
  g.ln_x = x; g.ln_g = gamma; g.ln_eps = eps; g.act_out = a_out;
  g.Wg_packed = Wg_packed; g.Wu_packed = Wu_packed;
  g.M = M; g.N = N; g.K = K;
  g.b_gate = b_gate; g.b_up = b_up;
  g.mlp = mlp;
  g.H = H; g.H16 = H16;
  return gated_gemm(g, as_stream(stream), "f16_gemm_gated_rms");
}
