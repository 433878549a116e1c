// Causal paged attention of a prompt chunk on MFMA (the reference's is_prefill
// pass: AttentionCUDA's `is_prefill` flag, attention/attention_cuda.hpp:21,
// with the maths of cpu_paged_attention_forward,
// attention_cpu/cpu_attention_kernel.cpp:37-129, per query token; SURVEY §8f
// row 4).
//
// m query tokens of ONE sequence sit at positions p0 .. p0+m-1 and their K/V
// are already in the sequence's pages (page-table row `row`).  Query i attends
// to positions 0 .. p0+i.  The decode kernel computes the same thing with one
// wave per (token, head), so each page is re-read once per query token; here a
// workgroup of NW waves owns 16·NW consecutive queries of one head, stages
// every 32-key block of K and V into LDS ONCE, and each wave runs
//   S^T[32 keys][16 queries] = K · Q^T        (v_mfma_f32_16x16x32_f16)
//   O^T[D][16 queries]     += V^T · P^T
// with the flash online softmax (log2 units, as pa_split_kernel) in between.
//
// Orientation: keys are the MFMA row index of S^T, so the C layout of S^T
// (lane l: rows 4(l>>4)+r, column l&15) already holds, per lane, 8 keys of ONE
// query: that is the B operand of the P·V product once the 32 keys are taken
// in the k order slot(key) = 8·((key&15)>>2) + 4·(key>>4) + (key&3).  V is
// staged row-major and its V^T A operand, in that same key order, is two
// hardware-transposed LDS reads (ds_read_b64_tr_b16) per 16 dims.  The query is the lane's column in both
// products, so the running max / sum / rescale are per lane (the 4 lanes of a
// query agree after a 2-step max exchange).
//
// Accuracy: q (fp32, pre-scaled by sm_scale·log2e) and p (fp32) are split into
// fp16 hi + lo halves and each product is two MFMAs; K and V are fp16 already.
// Both are first scaled by a power of two (q per query to |q|max ≈ 2^14, p by
// 2^14) because the MFMA drops fp16 subnormal inputs: unscaled, the lo half
// of every p < 0.25 was lost (1e-5 .. 5e-5 output error, measured).  Scaled,
// products of fp16 pairs are exact in the fp32 accumulator and the output
// error is at the decode kernel's level (scripts/diag_prefill.py).
//
// LLM_FP8 pools (KVT = LLM_FP8): a lane's chunk of a key row arrives as 8 e4m3
// bytes (half the global traffic and staging registers of fp16) and is decoded
// to fp16 on its way into LDS (fp8x4_to_f16 below).  Every e4m3 value is an
// fp16 normal (2^-9 .. 448), so the decode is exact, the LDS layout and all of
// the math are the fp16 instantiation's, and the output is bit-equal to the
// fp16 kernel's on pools holding the decoded values.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "pa_decode.hpp"
#include "row_ops.hpp"

namespace llm {
namespace {

struct PaPrefillArgs {
  const float* q;
  int q_stride;  // floats between query rows
  float* out;
  int out_stride;
  const uint8_t* k_pool;
  const uint8_t* v_pool;
  size_t page_stride;     // bytes
  const int32_t* pt_row;  // page_table + row * H * max_tiles
  int H, max_tiles, num_pages;
  int p0, m;
  // packed form (PACKED kernels): blockIdx.x indexes tiles[ntile][4] =
  // {q0, nq, row, p0} (device), pt_row is unused and m is the packed row count
  const int32_t* tiles;
  const int32_t* page_table;
  float qscale;  // sm_scale * log2(e)
  // key-range split (blockIdx.z = split s: tiles [s*pps, (s+1)*pps)); with
  // part_acc the unnormalised state goes to the decode layout
  // [(i*H + h)*nsplit + s][D] / [..][2] (m, l) for pa_merge_rows_internal
  int nsplit, pps;
  float* part_acc;
  float* part_ml;
  // multiplies the normalised head of the one-pass form (LLM_FP8: the V scale;
  // the split form hands it to the merge)
  float out_scale;
  // sliding window (0: off): the query at position p attends to positions
  // max(0, p - window + 1) .. p
  int window;
};

constexpr int kKeyBlock = 32;
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
constexpr float kPScale = 16384.f;  // P enters the PV MFMA as p * 2^14 (hi + lo)

__device__ __forceinline__ void split_f16(float x, _Float16& hi, _Float16& lo) {
  hi = (_Float16)x;
  lo = (_Float16)(x - (float)hi);
}

// Four e4m3 bytes of `w` as four fp16 values (two dwords, element order kept).
// v_cvt_scalef32_pk_f16_fp8 with scale 1 (2^0) converts two bytes per VALU op
// straight to packed fp16; NaN codes (0x7F / 0xFF) come out as fp16 NaN.
__device__ __forceinline__ u32x2 fp8x4_to_f16(uint32_t w) {
  return u32x2{
      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false)),
      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true))};
}

// PACKED: the workgroup's query tile comes from the tile table (rows q0 ..
// q0+nq-1 of q / out are positions p0 .. of page-table row `row`) instead of
// blockIdx.x * 16 NW of the one sequence; everything after these five values
// is the same code.
template <int KVT, int D, int TS, int NW, bool PACKED>
__global__ __launch_bounds__(64 * NW) void pa_prefill_kernel(PaPrefillArgs a) {
  static_assert(KVT == LLM_F16 || KVT == LLM_FP8, "KV element type");
  constexpr bool FP8 = KVT == LLM_FP8;
  constexpr int ES = FP8 ? 1 : 2;  // bytes per pool element
  constexpr int KB = kKeyBlock;
  constexpr int KSTR = D + 8;   // K row stride (halves): conflict-free 16-B row reads
  constexpr int VSTR = D + 16;  // V row stride (halves): 8·odd dwords, so the
                                // 64 lanes of a transposed read hit 64 banks
  constexpr int CPR = D / 8;    // 8-element chunks per key row (16 bytes fp16, 8 bytes e4m3)
  constexpr int NCH = KB * CPR; // chunks per block, each of K and V
  constexpr int NTH = 64 * NW;
  constexpr int CPT = NCH / NTH;
  constexpr int NKK = D / 32;   // k-steps of q.k
  constexpr int ND = D / 16;    // 16-dim tiles of the output
  static_assert(NCH % NTH == 0 && D % 32 == 0 && KB % TS == 0, "shape");
  __shared__ __attribute__((aligned(16))) _Float16 Ks[KB * KSTR];
  __shared__ __attribute__((aligned(16))) _Float16 Vs[KB * VSTR];
  __shared__ int kval[KB];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = wave_id_uniform();
  const int g = lane >> 4;
  const int c = lane & 15;
  const int h = blockIdx.y;
  int q0, nq, p0;  // the tile: first row of q / out, rows, position of the first
  const int32_t* pt_row;
  if constexpr (PACKED) {
    const int4 t = *reinterpret_cast<const int4*>(a.tiles + 4 * (size_t)blockIdx.x);
    q0 = t.x, nq = t.y, p0 = t.w;
    pt_row = a.page_table + (size_t)t.z * a.H * a.max_tiles;
  } else {
    q0 = blockIdx.x * 16 * NW;
    nq = min(16 * NW, a.m - q0);
    p0 = a.p0 + q0;
    pt_row = a.pt_row;
  }
  const int qt = w * 16 + c;   // this lane's query of the tile (column of S^T / O^T)
  const int qi = q0 + qt;      // its row of q / out
  const bool qok = qt < nq;
  const int qpos = p0 + qt;
  const int lastpos = p0 + nq - 1;  // last key any query here sees
  const int split = blockIdx.z;
  const int kb0 = split * a.pps * TS / KB;
  const int nblk = min((split + 1) * a.pps * TS / KB, lastpos / KB + 1);
  // no query of this workgroup reaches this split: the merge never reads it
  if (kb0 >= nblk) return;
  // Window: wlo = the first key any query of the tile sees (its first query's
  // first visible position), qlo = this lane's query's.  The key-block loop
  // starts at wlo's block.  The splits stay absolute (the merge counts a
  // row's splits from tile 0), so a split wholly below the tile's window
  // still owes the merge a partial: an empty one, (m, l, acc) = (sentinel, 0,
  // 0), written without reading any K/V.
  const int wlo = a.window > 0 ? max(0, p0 - a.window + 1) : 0;
  const int qlo = a.window > 0 ? qpos - a.window + 1 : 0;
  const int kbs = max(kb0, wlo / KB);
  if (kbs >= nblk) {  // (split form only: one pass ends at lastpos >= wlo)
    if (qok && a.part_acc) {
      const size_t pidx = ((size_t)qi * a.H + h) * a.nsplit + split;
      float* o = a.part_acc + pidx * D + 4 * g;
#pragma unroll
      for (int nd = 0; nd < ND; ++nd)
        *reinterpret_cast<f32x4*>(o + 16 * nd) = f32x4{0.f, 0.f, 0.f, 0.f};
      if (g == 0) *reinterpret_cast<float2*>(a.part_ml + pidx * 2) = float2{kNegSentinel, 0.f};
    }
    return;
  }
  const int32_t* pt = pt_row + (size_t)h * a.max_tiles;

  // Q^T B-operand fragments: lane holds q[qi][32kk + 8g .. +7] (pre-scaled by
  // qscale), hi + lo.  The query's values are also scaled by a power of two
  // 2^(14-e) (|q|max < 2^e) so the lo halves stay clear of fp16 subnormals,
  // which the MFMA does not keep; S is scaled back exactly after the MFMA.
  float qx[NKK][8];
  float amax = 0.f;
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk) {
    f32x4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = x0;
    if (qok) {
      const float* qp = a.q + (size_t)qi * a.q_stride + h * D + 32 * kk + 8 * g;
      x0 = *reinterpret_cast<const f32x4*>(qp);
      x1 = *reinterpret_cast<const f32x4*>(qp + 4);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      qx[kk][e] = x0[e] * a.qscale;
      qx[kk][4 + e] = x1[e] * a.qscale;
      amax = fmaxf(amax, fmaxf(fabsf(qx[kk][e]), fabsf(qx[kk][4 + e])));
    }
  }
  amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
  amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
  int qe = 0;
  (void)frexpf(amax, &qe);  // amax < 2^qe (0 for amax == 0)
  qe = min(max(qe, -100), 100);
  const float qsc = ldexpf(1.f, 14 - qe), qinv = ldexpf(1.f, qe - 14);
  f16x8 qh[NKK], ql[NKK];
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      _Float16 hi, lo;
      split_f16(qx[kk][e] * qsc, hi, lo);
      qh[kk][e] = hi;
      ql[kk][e] = lo;
    }

  // Staging: chunk i of a thread = (key ch / CPR, dims 8 (ch % CPR)) of K and
  // of V — rows coalesced, both stored row-major ([key][d]); the PV product
  // reads V transposed with ds_read_b64_tr_b16.
  using Chunk = typename std::conditional<FP8, u32x2, u32x4>::type;  // 8 pool elements
  Chunk kr[CPT], vr[CPT];
  int vok[CPT];
  // page of key position kg, -1 if none / past lastpos / below the tile's window.
  // Keys in [wlo, qlo) of a later query of the tile are staged with their real
  // V and dropped by p = 0 alone: safe because those pages are still live (the
  // tile's first query sees them, and pages are released only below the first
  // query's window), so they hold written, finite values.  A release point
  // above p0 - window + 1 would break that.
  auto page_of = [&](int kg) -> int {
    const int tile = kg / TS;
    int pg = (kg <= lastpos && kg >= wlo && tile < a.max_tiles) ? pt[tile] : -1;
    return (pg >= 0 && pg < a.num_pages) ? pg : -1;
  };
  auto load = [&](int kb) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int ch = tid + i * NTH;
      const int key = ch / CPR, d0 = (ch % CPR) * 8;
      const int kg = kb * KB + key;
      const int pg = page_of(kg);
      const size_t off = (size_t)pg * a.page_stride + ((kg % TS) * D + d0) * ES;
      vok[i] = pg >= 0;
      // masked keys stage V = 0: a never-written row may hold NaN (0 * NaN)
      kr[i] = pg >= 0 ? *reinterpret_cast<const Chunk*>(a.k_pool + off) : Chunk{};
      vr[i] = pg >= 0 ? *reinterpret_cast<const Chunk*>(a.v_pool + off) : Chunk{};
    }
  };
  auto as_f16 = [](const Chunk& x) -> u32x4 {  // the chunk's 8 values as fp16
    if constexpr (FP8) {
      const u32x2 a0 = fp8x4_to_f16(x[0]), a1 = fp8x4_to_f16(x[1]);
      return u32x4{a0[0], a0[1], a1[0], a1[1]};
    } else {
      return x;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int ch = tid + i * NTH;
      const int key = ch / CPR, d0 = (ch % CPR) * 8;
      *reinterpret_cast<u32x4*>(&Ks[key * KSTR + d0]) = as_f16(kr[i]);
      *reinterpret_cast<u32x4*>(&Vs[key * VSTR + d0]) = as_f16(vr[i]);
      if (d0 == 0) kval[key] = vok[i];
    }
  };

  f32x4 O[ND];
#pragma unroll
  for (int nd = 0; nd < ND; ++nd) O[nd] = f32x4{0.f, 0.f, 0.f, 0.f};
  float mrun = kNegSentinel, lrun = 0.f;

  load(kbs);
  for (int kb = kbs; kb < nblk; ++kb) {
    if (kb > kbs) __syncthreads();  // every wave is done reading block kb-1
    stage();
    __syncthreads();
    if (kb + 1 < nblk) load(kb + 1);  // next block's loads fly during this block's math

    // S^T: two 16-key tiles
    f32x4 s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
        const f16x8 kf = *reinterpret_cast<const f16x8*>(&Ks[(16 * t + c) * KSTR + 32 * kk + 8 * g]);
        s[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qh[kk], s[t], 0, 0, 0);
        s[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, ql[kk], s[t], 0, 0, 0);
      }
      s[t] *= qinv;
    }
    // causal + window + missing-page mask, online softmax (per query = per lane)
    bool ok[2][4];
    float mloc = kNegSentinel;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * t + 4 * g + r;
        ok[t][r] = kval[key] != 0 && kb * KB + key <= qpos && kb * KB + key >= qlo;
        if (ok[t][r]) mloc = fmaxf(mloc, s[t][r]);
      }
    mloc = fmaxf(mloc, __shfl_xor(mloc, 16, 64));
    mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
    const float mnew = fmaxf(mrun, mloc);
    const float corr = __builtin_amdgcn_exp2f(mrun - mnew);
    lrun *= corr;
#pragma unroll
    for (int nd = 0; nd < ND; ++nd) O[nd] *= corr;
    f16x8 ph, pl;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = ok[t][r] ? __builtin_amdgcn_exp2f(s[t][r] - mnew) : 0.f;
        lrun += p;
        _Float16 hi, lo;
        split_f16(p * kPScale, hi, lo);  // p <= 1: scaled clear of fp16 subnormals
        ph[4 * t + r] = hi;
        pl[4 * t + r] = lo;
      }
    mrun = mnew;
    // O^T += V^T · P^T.  A operand lane l: V^T[d = 16nd + (l&15)][k 8g+j] =
    // V[key(8g+j)][d], keys 4g..4g+3 then 16+4g..16+4g+3: two transposed
    // reads of 4 V rows x 16 columns, lane 4q+p addressing row q, columns 4p..
#pragma unroll
    for (int nd = 0; nd < ND; ++nd) {
      const int q4 = c >> 2, p4 = c & 3;
      const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4*)&Vs[(4 * g + q4) * VSTR + 16 * nd + 4 * p4]);
      const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4*)&Vs[(16 + 4 * g + q4) * VSTR + 16 * nd + 4 * p4]);
      const f16x8 vf = __builtin_bit_cast(
          f16x8, s16x8{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]});
      O[nd] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, ph, O[nd], 0, 0, 0);
      O[nd] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pl, O[nd], 0, 0, 0);
    }
  }

  // the 4 lanes of a query hold partial sums over their keys
  lrun += __shfl_xor(lrun, 16, 64);
  lrun += __shfl_xor(lrun, 32, 64);
  if (qok) {
    if (a.part_acc) {  // split partial state (unnormalised, log2 units)
      const size_t pidx = ((size_t)qi * a.H + h) * a.nsplit + split;
      float* o = a.part_acc + pidx * D + 4 * g;
#pragma unroll
      for (int nd = 0; nd < ND; ++nd) *reinterpret_cast<f32x4*>(o + 16 * nd) = O[nd] * (1.0f / kPScale);
      if (g == 0) *reinterpret_cast<float2*>(a.part_ml + pidx * 2) = float2{mrun, lrun};
    } else {
      const float inv = 1.0f / (lrun + 1e-6f) * (1.0f / kPScale);
      float* o = a.out + (size_t)qi * a.out_stride + h * D + 4 * g;
      // out_scale after the normalisation, as the merge applies it (x * 1 = x:
      // fp16 pools keep their bits)
#pragma unroll
      for (int nd = 0; nd < ND; ++nd)
        *reinterpret_cast<f32x4*>(o + 16 * nd) = O[nd] * inv * a.out_scale;
    }
  }
}

// ntile > 0: the packed form, one workgroup column per entry of a.tiles
// (tiles of 16 * kPackedNW queries).
template <int KVT, int D, int TS>
hipError_t launch_prefill(const PaPrefillArgs& a, int nw, int ntile, hipStream_t st) {
  if (ntile > 0) {
    const dim3 grid(ntile, a.H, a.nsplit);
    hipLaunchKernelGGL((pa_prefill_kernel<KVT, D, TS, 4, true>), grid, dim3(256), 0, st, a);
  } else if (nw == 4) {
    const dim3 grid((a.m + 63) / 64, a.H, a.nsplit);
    hipLaunchKernelGGL((pa_prefill_kernel<KVT, D, TS, 4, false>), grid, dim3(256), 0, st, a);
  } else {
    const dim3 grid((a.m + 31) / 32, a.H, a.nsplit);
    hipLaunchKernelGGL((pa_prefill_kernel<KVT, D, TS, 2, false>), grid, dim3(128), 0, st, a);
  }
  return hipGetLastError();
}

template <int KVT>
hipError_t launch_prefill_shape(const PaPrefillArgs& a, int D, int TS, int nw, int ntile,
                                hipStream_t st) {
  if (D == 64)
    return TS == 16 ? launch_prefill<KVT, 64, 16>(a, nw, ntile, st)
                    : launch_prefill<KVT, 64, 32>(a, nw, ntile, st);
  return TS == 16 ? launch_prefill<KVT, 128, 16>(a, nw, ntile, st)
                  : launch_prefill<KVT, 128, 32>(a, nw, ntile, st);
}

// Launch geometry: NW waves (16 queries each) per workgroup; the key range is
// split until the grid holds about kTargetWgs workgroups (4 per CU), in
// splits of whole 32-key blocks and at least 2 blocks each.  The plan reads
// the view's page_size and num_heads only: it is the same for fp16 and FP8 pools.
constexpr int kTargetWgs = 1024;
struct PrefillPlan {
  int nw, nsplit, pps;
};
// The key split of nq query tiles whose longest key range ends at position
// `end` (exclusive); p.nw is set by the caller.
PrefillPlan split_plan(const pa_kv_view* kv, int end, int nq, int nw) {
  PrefillPlan p;
  p.nw = nw;
  const int TS = kv->page_size;
  const int step = kKeyBlock / TS;  // tiles per key block
  const int ntiles = (end + TS - 1) / TS;
  const int want = std::min(std::max(kTargetWgs / std::max(nq * kv->num_heads, 1), 1), 128);
  int pps = (ntiles + want - 1) / want;
  pps = std::max((pps + step - 1) / step * step, 2 * step);
  p.pps = pps;
  p.nsplit = std::max(1, std::min((ntiles + pps - 1) / pps, 128));
  if (p.nsplit * pps < ntiles) {  // > 128 splits: lengthen them
    p.pps = ((ntiles + 127) / 128 + step - 1) / step * step;
    p.nsplit = (ntiles + p.pps - 1) / p.pps;
  }
  return p;
}

PrefillPlan prefill_plan(const pa_kv_view* kv, int p0, int m) {
#if LLM_TUNING
  const int nw = env_int("LLM_PREFILL_NW", 4) == 2 ? 2 : 4;
#else
  const int nw = 4;
#endif
  return split_plan(kv, p0 + m, (m + 16 * nw - 1) / (16 * nw), nw);
}

}  // namespace

bool pa_prefill_supported(const pa_kv_view* kv) {
  return kv && (kv->kv_dtype == LLM_F16 || kv->kv_dtype == LLM_FP8) &&
         (kv->head_dim == 64 || kv->head_dim == 128) &&
         (kv->page_size == 16 || kv->page_size == 32);
}

size_t pa_prefill_ws_bytes(const pa_kv_view* kv, int p0, int m) {
  if (!pa_prefill_supported(kv) || m <= 0 || p0 < 0) return 0;
  const PrefillPlan p = prefill_plan(kv, p0, m);
  if (p.nsplit <= 1) return 0;
  return (size_t)m * kv->num_heads * p.nsplit * (size_t)(kv->head_dim + 2) * sizeof(float);
}

int pa_prefill_internal(const pa_kv_view* kv, const float* q, int q_stride, float* out,
                        int out_stride, int row, int p0, int m, float sm_scale, void* workspace,
                        size_t workspace_bytes, hipStream_t st, const PaRowOutputs* rows,
                        int window) {
  LLM_REQUIRE(kv && q, "pa_prefill: NULL argument");
  LLM_REQUIRE(window >= 0, "pa_prefill: window must be >= 0 (0: off)");
  if (!pa_prefill_supported(kv))
    return fail(LLM_ERR_UNSUPPORTED,
                "pa_prefill: fp16 or FP8 (e4m3) pools with head_dim 64 or 128 and page_size 16 "
                "or 32 only");
  const int H = kv->num_heads, D = kv->head_dim, hid = H * D;
  LLM_REQUIRE(m >= 1 && p0 >= 0, "pa_prefill: need m >= 1 and p0 >= 0");
  LLM_REQUIRE(row >= 0 && row < kv->num_beams, "pa_prefill: row outside the page table");
  LLM_REQUIRE((long long)(p0 + m + kv->page_size - 1) / kv->page_size <= kv->max_tiles,
              "pa_prefill: positions past the page table's max_tiles");
  if (q_stride <= 0) q_stride = hid;
  if (out_stride <= 0) out_stride = hid;
  LLM_REQUIRE(q_stride >= hid && out_stride >= hid && q_stride % 4 == 0 && out_stride % 4 == 0,
              "pa_prefill: row strides must be >= H*D and multiples of 4");
  LLM_REQUIRE(reinterpret_cast<uintptr_t>(q) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0,
              "pa_prefill: q and out must be 16-byte aligned");
  const bool row_out = rows && (rows->q || rows->out16);
  PrefillPlan pl = prefill_plan(kv, p0, m);
  const size_t need = pa_prefill_ws_bytes(kv, p0, m);
  const bool split = pl.nsplit > 1 && workspace && workspace_bytes >= need &&
                     (out == nullptr || out_stride == hid) &&
                     (!row_out || rows->pack);  // the merge writes packed o_proj inputs
  LLM_REQUIRE(out || (split && row_out), "pa_prefill: out is NULL");
  // (the split merge holds a whole row in LDS, as pa_decode's row outputs)
  LLM_REQUIRE(!split || (size_t)hid * 4 <= 65536,
              "pa_prefill: the split form needs H*D <= 16384 (pass no workspace: one pass)");
  PaPrefillArgs a{};
  a.q = q;
  a.q_stride = q_stride;
  a.out = out;
  a.out_stride = out_stride;
  a.k_pool = static_cast<const uint8_t*>(kv->k_pool);
  a.v_pool = static_cast<const uint8_t*>(kv->v_pool);
  a.page_stride = kv_view_page_stride(*kv);
  a.pt_row = kv->page_table + (size_t)row * H * kv->max_tiles;
  a.H = H;
  a.max_tiles = kv->max_tiles;
  a.num_pages = kv->num_pages;
  a.p0 = p0;
  a.m = m;
  a.window = window;
  a.qscale = sm_scale * kLog2e;
  if (split) {
    a.nsplit = pl.nsplit;
    a.pps = pl.pps;
    a.part_acc = static_cast<float*>(workspace);
    a.part_ml = a.part_acc + (size_t)m * H * pl.nsplit * D;
  } else {
    a.nsplit = 1;
    a.pps = kv->max_tiles;
  }
  // LLM_FP8 pools: the V scale (1 for fp16 pools, whatever the caller left there)
  const float out_scale = (rows && kv->kv_dtype == LLM_FP8) ? rows->out_scale : 1.f;
  a.out_scale = out_scale;
  const int TS = kv->page_size;
  const hipError_t e = kv->kv_dtype == LLM_FP8
                           ? launch_prefill_shape<LLM_FP8>(a, D, TS, pl.nw, 0, st)
                           : launch_prefill_shape<LLM_F16>(a, D, TS, pl.nw, 0, st);
  if (e != hipSuccess) return fail(LLM_ERR_HIP, std::string("pa_prefill launch: ") + hipGetErrorString(e));
  // The merge gets no window: prefill splits are absolute, [s*pps, (s+1)*pps)
  // from tile 0, and the splits below a query's window hold empty partials
  // (the kernel writes them), so the merge's count from tile 0 stays right.
  if (split)
    return pa_merge_rows_internal(a.part_acc, a.part_ml, (rows && !rows->keep_out) ? nullptr : out,
                                  rows, nullptr, p0, m, H, D, p0 + m, TS, pl.pps, pl.nsplit,
                                  kv->max_tiles, st, out_scale, 0);
  if (row_out) {  // one pass: convert the fp32 rows into the o_proj input
    if (rows->q)
      LLM_HIP_RET(launch_quantize_rows(out, m, hid, rows->q, rows->inv_scale, st, rows->pack));
    if (rows->out16)
      LLM_HIP_RET(launch_to_f16(out, (size_t)m * hid, rows->out16, st, rows->pack ? hid : 0));
  }
  return LLM_OK;
}

// ---------------------------------------------------------------------------
// packed form: the chunks of several sequences in one launch
// ---------------------------------------------------------------------------
namespace {

constexpr int kPackedTile = 16 * 4;  // queries per tile-table entry (the NW = 4 kernel)

// The tile table and the rows' context lengths of up to kMetaSegs segments,
// written on the device from segment descriptors that travel as kernel
// arguments: the launch copies them, so the host array may die at once.
constexpr int kMetaSegs = 48;
struct PackedMetaArgs {
  int32_t seg[kMetaSegs][5];  // row, p0, len, first packed row, first tile
  int32_t* tiles;
  int32_t* ctx;
};

__global__ __launch_bounds__(64) void packed_meta_kernel(PackedMetaArgs a) {
  const int32_t* s = a.seg[blockIdx.x];
  const int row = s[0], p0 = s[1], len = s[2], q0 = s[3], t0 = s[4];
  for (int i = threadIdx.x; i < len; i += 64) a.ctx[q0 + i] = p0 + i + 1;
  const int nt = (len + kPackedTile - 1) / kPackedTile;
  for (int t = threadIdx.x; t < nt; t += 64)
    *reinterpret_cast<int4*>(a.tiles + 4 * (size_t)(t0 + t)) =
        int4{q0 + t * kPackedTile, min(kPackedTile, len - t * kPackedTile), row,
             p0 + t * kPackedTile};
}

struct PackedShape {
  int m = 0, ntile = 0, maxend = 0;
};

// Host validation of a segment list against the view's page table.
int packed_shape(const pa_kv_view* kv, const pa_prefill_seg* segs, int nseg, PackedShape* ps) {
  LLM_REQUIRE(kv && segs, "pa_prefill_packed: NULL argument");
  LLM_REQUIRE(nseg >= 1, "pa_prefill_packed: need nseg >= 1");
  LLM_REQUIRE(kv->page_size > 0 && kv->max_tiles > 0, "pa_prefill_packed: empty page table");
  long long m = 0, ntile = 0;
  int maxend = 0;
  std::vector<int32_t> seen(nseg);
  for (int j = 0; j < nseg; ++j) {
    const pa_prefill_seg& s = segs[j];
    LLM_REQUIRE(s.len >= 1 && s.p0 >= 0, "pa_prefill_packed: every segment needs len >= 1 and p0 >= 0");
    LLM_REQUIRE(s.row >= 0 && s.row < kv->num_beams, "pa_prefill_packed: row outside the page table");
    LLM_REQUIRE(((long long)s.p0 + s.len + kv->page_size - 1) / kv->page_size <= kv->max_tiles,
                "pa_prefill_packed: positions past the page table's max_tiles");
    seen[j] = s.row;
    m += s.len;
    ntile += (s.len + kPackedTile - 1) / kPackedTile;
    maxend = std::max(maxend, s.p0 + s.len);
  }
  std::sort(seen.begin(), seen.end());
  LLM_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(),
              "pa_prefill_packed: a page-table row appears in more than one segment");
  LLM_REQUIRE(m < (1ll << 30), "pa_prefill_packed: more than 2^30 packed rows");
  ps->m = (int)m, ps->ntile = (int)ntile, ps->maxend = maxend;
  return LLM_OK;
}

size_t align16(size_t n) { return (n + 15) / 16 * 16; }

}  // namespace

size_t pa_prefill_packed_meta_bytes(int m, int ntile) {
  return align16(((size_t)4 * ntile + m) * sizeof(int32_t));
}

size_t pa_prefill_packed_part_bytes(const pa_kv_view* kv, int maxend, int ntile, int m) {
  if (!pa_prefill_supported(kv) || m <= 0 || ntile <= 0) return 0;
  const PrefillPlan p = split_plan(kv, maxend, ntile, 4);
  if (p.nsplit <= 1) return 0;
  return (size_t)m * kv->num_heads * p.nsplit * (size_t)(kv->head_dim + 2) * sizeof(float);
}

// split_plan gives at most `want` splits whatever the key range, and nq tiles
// hold at most 64 nq rows.
size_t pa_prefill_packed_part_bound(const pa_kv_view* kv, int max_rows) {
  if (!pa_prefill_supported(kv) || max_rows <= 0) return 0;
  size_t b = 0;
  for (int nq = 1; nq <= max_rows; ++nq) {
    const int want = std::min(std::max(kTargetWgs / std::max(nq * kv->num_heads, 1), 1), 128);
    const size_t rows = std::min<size_t>(max_rows, (size_t)kPackedTile * nq);
    b = std::max(b, rows * kv->num_heads * want * (size_t)(kv->head_dim + 2) * sizeof(float));
  }
  return b;
}

int pa_prefill_packed_internal(const pa_kv_view* kv, const float* q, int q_stride, float* out,
                               int out_stride, const int32_t* tiles_dev, int ntile,
                               const int32_t* ctx_dev, int m, int maxend, float sm_scale,
                               void* part_ws, size_t part_bytes, hipStream_t st,
                               const PaRowOutputs* rows, int window) {
  LLM_REQUIRE(kv && q && tiles_dev && ctx_dev, "pa_prefill_packed: NULL argument");
  LLM_REQUIRE(window >= 0, "pa_prefill_packed: window must be >= 0 (0: off)");
  if (!pa_prefill_supported(kv))
    return fail(LLM_ERR_UNSUPPORTED,
                "pa_prefill_packed: fp16 or FP8 (e4m3) pools with head_dim 64 or 128 and "
                "page_size 16 or 32 only");
  const int H = kv->num_heads, D = kv->head_dim, hid = H * D, TS = kv->page_size;
  LLM_REQUIRE(m >= 1 && ntile >= 1 && ntile <= m && maxend >= 1,
              "pa_prefill_packed: need m >= 1 rows in 1 .. m tiles");
  LLM_REQUIRE((long long)(maxend + TS - 1) / TS <= kv->max_tiles,
              "pa_prefill_packed: positions past the page table's max_tiles");
  if (q_stride <= 0) q_stride = hid;
  if (out_stride <= 0) out_stride = hid;
  LLM_REQUIRE(q_stride >= hid && out_stride >= hid && q_stride % 4 == 0 && out_stride % 4 == 0,
              "pa_prefill_packed: row strides must be >= H*D and multiples of 4");
  LLM_REQUIRE(reinterpret_cast<uintptr_t>(q) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(tiles_dev) % 16 == 0,
              "pa_prefill_packed: q, out and the tile table must be 16-byte aligned");
  const bool row_out = rows && (rows->q || rows->out16);
  // one (nsplit, pps) for the launch: the longest segment end, every tile
  const PrefillPlan pl = split_plan(kv, maxend, ntile, 4);
  const size_t need = pa_prefill_packed_part_bytes(kv, maxend, ntile, m);
  const bool split = pl.nsplit > 1 && part_ws && part_bytes >= need &&
                     (out == nullptr || out_stride == hid) &&
                     (!row_out || rows->pack);  // the merge writes packed o_proj inputs
  LLM_REQUIRE(out || (split && row_out), "pa_prefill_packed: out is NULL");
  LLM_REQUIRE(!split || (size_t)hid * 4 <= 65536,
              "pa_prefill_packed: the split form needs H*D <= 16384 (pass no split workspace: "
              "one pass)");
  PaPrefillArgs a{};
  a.q = q;
  a.q_stride = q_stride;
  a.out = out;
  a.out_stride = out_stride;
  a.k_pool = static_cast<const uint8_t*>(kv->k_pool);
  a.v_pool = static_cast<const uint8_t*>(kv->v_pool);
  a.page_stride = kv_view_page_stride(*kv);
  a.tiles = tiles_dev;
  a.page_table = kv->page_table;
  a.H = H;
  a.max_tiles = kv->max_tiles;
  a.num_pages = kv->num_pages;
  a.m = m;
  a.window = window;
  a.qscale = sm_scale * kLog2e;
  if (split) {
    a.nsplit = pl.nsplit;
    a.pps = pl.pps;
    a.part_acc = static_cast<float*>(part_ws);
    a.part_ml = a.part_acc + (size_t)m * H * pl.nsplit * D;
  } else {
    a.nsplit = 1;
    a.pps = kv->max_tiles;
  }
  const float out_scale = (rows && kv->kv_dtype == LLM_FP8) ? rows->out_scale : 1.f;
  a.out_scale = out_scale;
  const hipError_t e = kv->kv_dtype == LLM_FP8
                           ? launch_prefill_shape<LLM_FP8>(a, D, TS, 4, ntile, st)
                           : launch_prefill_shape<LLM_F16>(a, D, TS, 4, ntile, st);
  if (e != hipSuccess)
    return fail(LLM_ERR_HIP, std::string("pa_prefill_packed launch: ") + hipGetErrorString(e));
  // a row's context selects the splits its own tile wrote (no window for the
  // merge: absolute splits, empty partials below the window, as pa_prefill's)
  if (split)
    return pa_merge_rows_internal(a.part_acc, a.part_ml, (rows && !rows->keep_out) ? nullptr : out,
                                  rows, ctx_dev, -1, m, H, D, maxend, TS, pl.pps, pl.nsplit,
                                  kv->max_tiles, st, out_scale, 0);
  if (row_out) {  // one pass: convert the fp32 rows into the o_proj input
    if (rows->q)
      LLM_HIP_RET(launch_quantize_rows(out, m, hid, rows->q, rows->inv_scale, st, rows->pack));
    if (rows->out16)
      LLM_HIP_RET(launch_to_f16(out, (size_t)m * hid, rows->out16, st, rows->pack ? hid : 0));
  }
  return LLM_OK;
}

}  // namespace llm

extern "C" int pa_prefill_packed_tiles(const pa_kv_view* kv, const pa_prefill_seg* segs, int nseg,
                                       int32_t* tiles, int cap) {
  llm::PackedShape ps;
  if (llm::packed_shape(kv, segs, nseg, &ps) != LLM_OK) return -1;
  if (!tiles || cap < ps.ntile) return ps.ntile;
  int q0 = 0, t = 0;
  for (int j = 0; j < nseg; ++j) {
    for (int o = 0; o < segs[j].len; o += llm::kPackedTile, ++t) {
      tiles[4 * t + 0] = q0 + o;
      tiles[4 * t + 1] = std::min(llm::kPackedTile, segs[j].len - o);
      tiles[4 * t + 2] = segs[j].row;
      tiles[4 * t + 3] = segs[j].p0 + o;
    }
    q0 += segs[j].len;
  }
  return ps.ntile;
}

extern "C" size_t pa_prefill_packed_workspace_bytes(const pa_kv_view* kv,
                                                    const pa_prefill_seg* segs, int nseg,
                                                    int split) {
  llm::PackedShape ps;
  if (llm::packed_shape(kv, segs, nseg, &ps) != LLM_OK) return 0;
  return llm::pa_prefill_packed_meta_bytes(ps.m, ps.ntile) +
         (split ? llm::pa_prefill_packed_part_bytes(kv, ps.maxend, ps.ntile, ps.m) : 0);
}

extern "C" int pa_prefill_packed(const pa_kv_view* kv, const float* q, int q_stride, float* out,
                                 int out_stride, const pa_prefill_seg* segs, int nseg,
                                 float sm_scale, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  return pa_prefill_packed_window(kv, q, q_stride, out, out_stride, segs, nseg, sm_scale, 0,
                                  workspace, workspace_bytes, stream);
}

int llm::pa_prefill_packed_segs_internal(const pa_kv_view* kv, const float* q, int q_stride,
                                         float* out, int out_stride, const pa_prefill_seg* segs,
                                         int nseg, float sm_scale, int window, void* workspace,
                                         size_t workspace_bytes, hipStream_t st,
                                         const PaRowOutputs* rows) {
  LLM_REQUIRE(kv && q, "pa_prefill_packed: NULL argument");
  LLM_REQUIRE(window >= 0, "pa_prefill_packed: window must be >= 0 (0: off)");
  PackedShape ps;
  const int rc = packed_shape(kv, segs, nseg, &ps);
  if (rc) return rc;
  if (!pa_prefill_supported(kv))
    return fail(LLM_ERR_UNSUPPORTED,
                "pa_prefill_packed: fp16 or FP8 (e4m3) pools with head_dim 64 or 128 and "
                "page_size 16 or 32 only");
  const int hid = kv->num_heads * kv->head_dim;
  const int qs = q_stride <= 0 ? hid : q_stride, os = out_stride <= 0 ? hid : out_stride;
  LLM_REQUIRE(qs >= hid && os >= hid && qs % 4 == 0 && os % 4 == 0,
              "pa_prefill_packed: row strides must be >= H*D and multiples of 4");
  LLM_REQUIRE(reinterpret_cast<uintptr_t>(q) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0,
              "pa_prefill_packed: q and out must be 16-byte aligned");
  const size_t meta = pa_prefill_packed_meta_bytes(ps.m, ps.ntile);
  LLM_REQUIRE(workspace && workspace_bytes >= meta &&
                  reinterpret_cast<uintptr_t>(workspace) % 16 == 0,
              "pa_prefill_packed: workspace smaller than pa_prefill_packed_workspace_bytes(.., 0) "
              "or not 16-byte aligned");
  int32_t* tiles = static_cast<int32_t*>(workspace);
  int32_t* ctx = tiles + (size_t)4 * ps.ntile;
  PackedMetaArgs ma{};
  ma.tiles = tiles;
  ma.ctx = ctx;
  int q0 = 0, t0 = 0;
  for (int j0 = 0; j0 < nseg; j0 += kMetaSegs) {
    const int n = std::min(kMetaSegs, nseg - j0);
    for (int j = 0; j < n; ++j) {
      const pa_prefill_seg& s = segs[j0 + j];
      const int32_t v[5] = {s.row, s.p0, s.len, q0, t0};
      std::copy(v, v + 5, ma.seg[j]);
      q0 += s.len;
      t0 += (s.len + kPackedTile - 1) / kPackedTile;
    }
    hipLaunchKernelGGL(packed_meta_kernel, dim3(n), dim3(64), 0, st, ma);
    LLM_HIP_RET(hipGetLastError());
  }
  return pa_prefill_packed_internal(kv, q, qs, out, os, tiles, ps.ntile, ctx, ps.m, ps.maxend,
                                    sm_scale, static_cast<uint8_t*>(workspace) + meta,
                                    workspace_bytes - meta, st, rows, window);
}

extern "C" int pa_prefill_packed_window(const pa_kv_view* kv, const float* q, int q_stride,
                                        float* out, int out_stride, const pa_prefill_seg* segs,
                                        int nseg, float sm_scale, int window, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  LLM_REQUIRE(kv && q && out, "pa_prefill_packed: NULL argument");
  return llm::pa_prefill_packed_segs_internal(kv, q, q_stride, out, out_stride, segs, nseg,
                                              sm_scale, window, workspace, workspace_bytes,
                                              llm::as_stream(stream));
}

extern "C" size_t pa_prefill_workspace_bytes(const pa_kv_view* kv, int p0, int m) {
  return llm::pa_prefill_ws_bytes(kv, p0, m);
}

extern "C" int pa_prefill(const pa_kv_view* kv, const float* q, int q_stride, float* out,
                          int out_stride, int row, int p0, int m, float sm_scale, void* workspace,
                          size_t workspace_bytes, void* stream) {
  return pa_prefill_window(kv, q, q_stride, out, out_stride, row, p0, m, sm_scale, 0, workspace,
                           workspace_bytes, stream);
}

extern "C" int pa_prefill_window(const pa_kv_view* kv, const float* q, int q_stride, float* out,
                                 int out_stride, int row, int p0, int m, float sm_scale,
                                 int window, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  LLM_REQUIRE(out, "pa_prefill: out is NULL");
  return llm::pa_prefill_internal(kv, q, q_stride, out, out_stride, row, p0, m, sm_scale,
                                  workspace, workspace_bytes, llm::as_stream(stream), nullptr,
                                  window);
}
