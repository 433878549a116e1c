// Shared-prefix decode attention on MFMA: the group kernel.
//
// Served rows whose prompts begin alike map the same KV pages on their leading
// tiles (prefix caching, serve_plan.hpp).  The split kernel (pa_split.hpp)
// walks every row's whole page list, so a header shared by G live rows is
// streamed from HBM G times per layer per step.  Here a GROUP -- G >= 2 batch
// rows, any rows in any order, whose page-table entries agree on their first P
// tiles -- reads those P tiles once: for every (row of the group, head) the
// kernel computes the unnormalised online-softmax state (m, l, acc[D]) of the
// row's query over the P * page_size shared tokens.  No causal mask: every
// shared token lies below every member's context.  The rest of each row runs
// through the split kernel from tile P on (PaSplitArgs::first_tile) and the
// split merge joins the two (pa_decode.hip merge_slots).
//
// Work split.  With G queries against one K/V stream the scores are a real
// matrix product, but groups are small (2 .. max_batch rows) and the prefix is
// long, so the parallelism comes from the key range, not from query tiles
// (pa_prefill.hip's split: 64 consecutive queries per workgroup, every wave its
// own 16 queries over the same staged keys).  Here
//   * a workgroup owns (a 16-query tile of a group, a head, a key split);
//   * its kShareWaves waves hold the SAME 16 gathered queries and take
//     different 32-key blocks of the split, block kb0 + round * 4 + wave: each
//     wave stages its own block into its own LDS region (no block is staged
//     twice, none is shared between waves), with the next round's block in
//     flight in registers during the current round's math;
//   * at the end the waves' (m, l, acc) meet in LDS (over the staging space)
//     and the workgroup writes ONE partial per (query, head, split), in the
//     split merge's layout, slot `split` of the row's npre prefix slots;
//   * the key-split count comes from share_launch (share_plan.hpp): splits
//     until the grid holds ~4 workgroups per CU, one (npre, blocks per split)
//     for the launch.  A split past a shorter group's end stages nothing and
//     writes the empty state (sentinel, 0, 0), which the merge weighs with 0.
// So a shared page is read from HBM once per (group query tile, head, split).
//
// Arithmetic: pa_prefill.hip's conventions, so that the accuracy is that
// kernel's (tests at its bars): S^T = K . Q^T and O^T += V^T . P^T with
// v_mfma_f32_16x16x32_f16, keys as the MFMA row index so that S^T's C layout
// is the P.V product's B operand, V^T read with ds_read_b64_tr_b16; q and p as
// fp16 hi + lo halves pre-scaled by powers of two (the MFMA drops fp16
// subnormal inputs); log2-unit softmax; e4m3 pages decoded exactly to fp16 on
// the way into LDS.  Missing pages (-1, >= num_pages) stage K = V = 0 and are
// masked.  The shared tiles are whole written pages, so no token of them needs
// a context check.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "pa_decode.hpp"
#include "share_plan.hpp"

namespace llm {
namespace {

struct PaSharedArgs {
  const float* q;
  int q_stride;  // floats between batch rows of q
  const uint8_t* k_pool;
  const uint8_t* v_pool;
  size_t page_stride;  // bytes
  const int32_t* page_table;
  int H, max_tiles, num_pages;
  const int32_t* tiles;  // [gridDim.x][4] {first index into rows, queries, P, 0}
  const int32_t* rows;
  int bps;       // 32-key blocks per split (blockIdx.z)
  float qscale;  // sm_scale * log2(e)
  float* part_acc;  // [(b * H + h) * nslots + split][D]
  float* part_ml;   // [..][2] (m, l)
  int nslots;       // partial slots per (row, head): npre + the suffix splits
};

constexpr int KB = kShareKeyBlock;
constexpr int NW = kShareWaves;
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
constexpr float kPScale = 16384.f;  // P enters the PV MFMA as p * 2^14 (hi + lo)

__device__ __forceinline__ void split_f16(float x, _Float16& hi, _Float16& lo) {
  hi = (_Float16)x;
  lo = (_Float16)(x - (float)hi);
}

// Four e4m3 bytes as four fp16 values, exactly (pa_prefill.hip fp8x4_to_f16).
__device__ __forceinline__ u32x2 fp8x4_to_f16(uint32_t w) {
  return u32x2{
      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false)),
      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true))};
}

template <int KVT, int D, int TS>
__global__ __launch_bounds__(64 * NW) void pa_shared_kernel(PaSharedArgs a) {
  static_assert(KVT == LLM_F16 || KVT == LLM_FP8, "KV element type");
  constexpr bool FP8 = KVT == LLM_FP8;
  constexpr int ES = FP8 ? 1 : 2;   // bytes per pool element
  constexpr int KSTR = D + 8;       // K row stride (halves): conflict-free 16-B row reads
  constexpr int VSTR = D + 16;      // V row stride (halves): conflict-free transposed reads
  constexpr int CPR = D / 8;        // 8-element chunks per key row
  constexpr int CPT = KB * CPR / 64;  // chunks per lane per block, each of K and V
  constexpr int NKK = D / 32;       // k-steps of q.k
  constexpr int ND = D / 16;        // 16-dim tiles of the output
  constexpr int WSTR = KB * (KSTR + VSTR);  // halves of LDS per wave
  static_assert(D % 32 == 0 && KB % TS == 0 && (KB * CPR) % 64 == 0, "shape");
  // the waves' final states [NW][16][D] fp32 lie over the staging space
  static_assert((size_t)NW * 16 * D * 4 <= (size_t)NW * WSTR * 2, "merge space");
  __shared__ __attribute__((aligned(16))) _Float16 stage_lds[NW * WSTR];
  __shared__ int kval[NW][KB];
  __shared__ float wm[NW][16], wl[NW][16];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = wave_id_uniform();
  const int g = lane >> 4;
  const int c = lane & 15;  // this lane's query of the tile (column of S^T / O^T)
  const int h = blockIdx.y;
  const int split = blockIdx.z;
  const int4 t = *reinterpret_cast<const int4*>(a.tiles + 4 * (size_t)blockIdx.x);
  const int32_t* rows = a.rows + t.x;
  const int nq = t.y, P = t.z;
  const bool qok = c < nq;
  const int b = rows[qok ? c : 0];  // the query's batch row
  // any member's table row names the shared pages; the tile's first is read
  const int32_t* pt = a.page_table + ((size_t)rows[0] * a.H + h) * a.max_tiles;
  const int nblk = (P * TS + KB - 1) / KB;
  const int kb0 = split * a.bps;
  const int kb1 = min(kb0 + a.bps, nblk);
  // rounds of the workgroup: uniform over its waves (a wave whose block of the
  // last round is past kb1 stages nothing and masks every key)
  const int nround = kb1 > kb0 ? (kb1 - kb0 + NW - 1) / NW : 0;
  _Float16* Ks = stage_lds + w * WSTR;
  _Float16* Vs = Ks + KB * KSTR;

  // Q^T B-operand fragments: lane holds q[b][32kk + 8g .. +7] (pre-scaled by
  // qscale), hi + lo, scaled by 2^(14-e) (|q|max < 2^e) clear of fp16
  // subnormals; S is scaled back exactly after the MFMA.
  float qx[NKK][8];
  float amax = 0.f;
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk) {
    f32x4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = x0;
    if (qok && nround > 0) {
      const float* qp = a.q + (size_t)b * a.q_stride + h * D + 32 * kk + 8 * g;
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

  // Staging of the wave's own block: chunk i of a lane = (key ch / CPR, dims
  // 8 (ch % CPR)) of K and of V, rows coalesced, both row-major in LDS.
  using Chunk = typename std::conditional<FP8, u32x2, u32x4>::type;  // 8 pool elements
  Chunk kr[CPT], vr[CPT];
  int vok[CPT];
  auto load = [&](int kb) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int ch = lane + i * 64;
      const int key = ch / CPR, d0 = (ch % CPR) * 8;
      const int kg = kb * KB + key;
      const int tile = kg / TS;
      int pg = (kb < kb1 && tile < P && tile < a.max_tiles) ? pt[tile] : -1;
      pg = (pg >= 0 && pg < a.num_pages) ? pg : -1;
      const size_t off = (size_t)pg * a.page_stride + ((kg % TS) * D + d0) * ES;
      vok[i] = pg >= 0;
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
      const int ch = lane + i * 64;
      const int key = ch / CPR, d0 = (ch % CPR) * 8;
      *reinterpret_cast<u32x4*>(&Ks[key * KSTR + d0]) = as_f16(kr[i]);
      *reinterpret_cast<u32x4*>(&Vs[key * VSTR + d0]) = as_f16(vr[i]);
      if (d0 == 0) kval[w][key] = vok[i];
    }
  };

  f32x4 O[ND];
#pragma unroll
  for (int nd = 0; nd < ND; ++nd) O[nd] = f32x4{0.f, 0.f, 0.f, 0.f};
  float mrun = kNegSentinel, lrun = 0.f;

  if (nround > 0) load(kb0 + w);
  for (int it = 0; it < nround; ++it) {
    if (it > 0) __syncthreads();  // the wave's reads of its last block are done
    stage();
    __syncthreads();
    if (it + 1 < nround) load(kb0 + (it + 1) * NW + w);  // in flight during this block's math

    // S^T: two 16-key tiles
    f32x4 s[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      s[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
        const f16x8 kf = *reinterpret_cast<const f16x8*>(&Ks[(16 * tt + c) * KSTR + 32 * kk + 8 * g]);
        s[tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qh[kk], s[tt], 0, 0, 0);
        s[tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, ql[kk], s[tt], 0, 0, 0);
      }
      s[tt] *= qinv;
    }
    // missing-page mask, online softmax (per query = per lane)
    bool ok[2][4];
    float mloc = kNegSentinel;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ok[tt][r] = kval[w][16 * tt + 4 * g + r] != 0;
        if (ok[tt][r]) mloc = fmaxf(mloc, s[tt][r]);
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
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = ok[tt][r] ? __builtin_amdgcn_exp2f(s[tt][r] - mnew) : 0.f;
        lrun += p;
        _Float16 hi, lo;
        split_f16(p * kPScale, hi, lo);  // p <= 1: scaled clear of fp16 subnormals
        ph[4 * tt + r] = hi;
        pl[4 * tt + r] = lo;
      }
    mrun = mnew;
    // O^T += V^T . P^T: two transposed reads of 4 V rows x 16 columns per 16
    // dims, keys 4g..4g+3 then 16+4g..16+4g+3 (the k order of ph / pl)
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

  // The waves' states meet in LDS: wacc[w][query][D] over the staging space
  // (every wave is past its last block), then the workgroup merges them, 4
  // dims of one query per thread and pass, and writes the split's partial.  A
  // split with no block (nround 0) merges NW empty states into the empty one.
  float* wacc = reinterpret_cast<float*>(stage_lds);
  __syncthreads();
#pragma unroll
  for (int nd = 0; nd < ND; ++nd)
    *reinterpret_cast<f32x4*>(&wacc[(w * 16 + c) * D + 16 * nd + 4 * g]) = O[nd] * (1.0f / kPScale);
  if (g == 0) {
    wm[w][c] = mrun;
    wl[w][c] = lrun;
  }
  __syncthreads();
  for (int i = tid; i < 16 * (D / 4); i += 64 * NW) {
    const int qi = i / (D / 4), d = (i % (D / 4)) * 4;
    if (qi >= nq) continue;
    float M = kNegSentinel;
#pragma unroll
    for (int k = 0; k < NW; ++k) M = fmaxf(M, wm[k][qi]);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float L = 0.f;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const float wk = __builtin_amdgcn_exp2f(wm[k][qi] - M);
      L += wl[k][qi] * wk;
      acc += *reinterpret_cast<const f32x4*>(&wacc[(k * 16 + qi) * D + d]) * wk;
    }
    const size_t pidx = ((size_t)rows[qi] * a.H + h) * a.nslots + split;
    *reinterpret_cast<f32x4*>(a.part_acc + pidx * D + d) = acc;
    if (d == 0) *reinterpret_cast<float2*>(a.part_ml + pidx * 2) = float2{M, L};
  }
}

template <int KVT, int D, int TS>
hipError_t launch_shared(const PaSharedArgs& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((pa_shared_kernel<KVT, D, TS>), grid, dim3(64 * NW), 0, st, a);
  return hipGetLastError();
}

template <int KVT>
hipError_t launch_shared_shape(const PaSharedArgs& a, int D, int TS, dim3 grid, hipStream_t st) {
  if (D == 64)
    return TS == 16 ? launch_shared<KVT, 64, 16>(a, grid, st)
                    : launch_shared<KVT, 64, 32>(a, grid, st);
  return TS == 16 ? launch_shared<KVT, 128, 16>(a, grid, st)
                  : launch_shared<KVT, 128, 32>(a, grid, st);
}

size_t align16(size_t n) { return (n + 15) / 16 * 16; }

}  // namespace

// The shapes of pa_prefill_supported: the two kernels share their arithmetic.
bool pa_shared_supported(const pa_kv_view* kv) { return pa_prefill_supported(kv); }

int pa_shared_prefix_launch(const pa_kv_view* kv, const float* q, int q_stride, float qscale,
                            const PaShared& sh, float* part_acc, float* part_ml, int nslots,
                            hipStream_t st) {
  LLM_REQUIRE(kv && q && part_acc && part_ml && sh.tiles && sh.rows && sh.first_tile,
              "pa_decode_shared: NULL argument");
  if (!pa_shared_supported(kv))
    return fail(LLM_ERR_UNSUPPORTED,
                "pa_decode_shared: fp16 or FP8 (e4m3) pools with head_dim 64 or 128 and "
                "page_size 16 or 32 only");
  LLM_REQUIRE(sh.ntile >= 1 && sh.npre >= 1 && sh.npre <= kShareMaxPre && sh.bps >= 1 &&
                  nslots >= sh.npre,
              "pa_decode_shared: bad launch geometry (share_launch)");
  LLM_REQUIRE(q_stride % 4 == 0 && reinterpret_cast<uintptr_t>(q) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(sh.tiles) % 16 == 0,
              "pa_decode_shared: q rows and the tile table must be 16-byte aligned");
  PaSharedArgs a{};
  a.q = q;
  a.q_stride = q_stride;
  a.k_pool = static_cast<const uint8_t*>(kv->k_pool);
  a.v_pool = static_cast<const uint8_t*>(kv->v_pool);
  a.page_stride = kv_view_page_stride(*kv);
  a.page_table = kv->page_table;
  a.H = kv->num_heads;
  a.max_tiles = kv->max_tiles;
  a.num_pages = kv->num_pages;
  a.tiles = sh.tiles;
  a.rows = sh.rows;
  a.bps = sh.bps;
  a.qscale = qscale;
  a.part_acc = part_acc;
  a.part_ml = part_ml;
  a.nslots = nslots;
  const dim3 grid(sh.ntile, kv->num_heads, sh.npre);
  const hipError_t e =
      kv->kv_dtype == LLM_FP8
          ? launch_shared_shape<LLM_FP8>(a, kv->head_dim, kv->page_size, grid, st)
          : launch_shared_shape<LLM_F16>(a, kv->head_dim, kv->page_size, grid, st);
  if (e != hipSuccess)
    return fail(LLM_ERR_HIP, std::string("pa_shared launch: ") + hipGetErrorString(e));
  return LLM_OK;
}

namespace {

// The groups of a pa_decode_shared call: the shape checks that need no device
// value, and the plan's tables.
int shared_groups(const pa_kv_view* kv, int B, const int32_t* group_rows, const int32_t* group_off,
                  const int32_t* group_tiles, int ngroups, std::vector<ShareGroup>* out) {
  LLM_REQUIRE(kv && group_rows && group_off && group_tiles, "pa_decode_shared: NULL argument");
  LLM_REQUIRE(ngroups >= 1 && B >= 2, "pa_decode_shared: need ngroups >= 1 and B >= 2");
  LLM_REQUIRE(group_off[0] == 0, "pa_decode_shared: group_off[0] must be 0");
  std::vector<char> seen(B, 0);
  for (int j = 0; j < ngroups; ++j) {
    ShareGroup g;
    LLM_REQUIRE(group_off[j + 1] - group_off[j] >= 2, "pa_decode_shared: a group needs >= 2 rows");
    LLM_REQUIRE(group_tiles[j] >= 1 && group_tiles[j] <= kv->max_tiles,
                "pa_decode_shared: a group's shared tiles must be in [1, max_tiles]");
    g.tiles = group_tiles[j];
    for (int i = group_off[j]; i < group_off[j + 1]; ++i) {
      const int r = group_rows[i];
      LLM_REQUIRE(r >= 0 && r < B, "pa_decode_shared: group row outside the batch");
      LLM_REQUIRE(!seen[r], "pa_decode_shared: overlapping groups (a row appears twice)");
      seen[r] = 1;
      g.rows.push_back(r);
    }
    out->push_back(g);
  }
  return LLM_OK;
}

}  // namespace
}  // namespace llm

using namespace llm;

extern "C" size_t pa_decode_shared_workspace_bytes(const pa_kv_view* kv, int B, int T) {
  if (!kv || B <= 0 || T < 0 || kv->page_size <= 0) return 0;
  const int ntiles = std::max(1, std::min((T + kv->page_size - 1) / kv->page_size, kv->max_tiles));
  const size_t slots = (size_t)std::min<long long>(kMaxSplits, max_nsplit(B, kv->num_heads, ntiles) +
                                                                   kShareMaxPre);
  return align16(share_tables_cap(B) * sizeof(int32_t)) +
         (size_t)B * kv->num_heads * slots * (size_t)(kv->head_dim + 2) * sizeof(float);
}

extern "C" int pa_decode_shared(const pa_kv_view* kv, const float* q, float* out,
                                const int32_t* context_lens, int B, int H, int D, int T,
                                float sm_scale, const int32_t* group_rows,
                                const int32_t* group_off, const int32_t* group_tiles, int ngroups,
                                void* workspace, size_t workspace_bytes, void* stream) {
  LLM_REQUIRE(kv && q && out, "pa_decode_shared: NULL argument");
  LLM_REQUIRE(kv->num_heads == H && kv->head_dim == D, "pa_decode_shared: H / D are not the view's");
  if (!pa_shared_supported(kv))
    return fail(LLM_ERR_UNSUPPORTED,
                "pa_decode_shared: fp16 or FP8 (e4m3) pools with head_dim 64 or 128 and "
                "page_size 16 or 32 only");
  std::vector<ShareGroup> groups;
  const int rc = shared_groups(kv, B, group_rows, group_off, group_tiles, ngroups, &groups);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  const int TS = kv->page_size;
  // The view has no host mirror of its table: the members' claimed entries and
  // the contexts are read back (behind the stream's earlier work) and checked.
  LLM_HIP_RET(hipStreamSynchronize(st));
  std::vector<int32_t> ctx(B, T);
  if (context_lens)
    LLM_HIP_RET(hipMemcpy(ctx.data(), context_lens, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
  std::vector<int32_t> first, cur;
  for (const ShareGroup& g : groups) {
    const size_t n = (size_t)H * g.tiles;
    first.resize(n), cur.resize(n);
    for (size_t i = 0; i < g.rows.size(); ++i) {
      const int r = g.rows[i];
      LLM_REQUIRE(r < kv->num_beams, "pa_decode_shared: group row outside the page table");
      LLM_REQUIRE((long long)g.tiles * TS <= std::min(std::max(ctx[r], 0), T),
                  "pa_decode_shared: a claimed shared tile lies at or past a member's context");
      std::vector<int32_t>& dst = i == 0 ? first : cur;
      LLM_HIP_RET(hipMemcpy2D(dst.data(), sizeof(int32_t) * g.tiles,
                              kv->page_table + (size_t)r * H * kv->max_tiles,
                              sizeof(int32_t) * kv->max_tiles, sizeof(int32_t) * g.tiles, H,
                              hipMemcpyDeviceToHost));
      LLM_REQUIRE(i == 0 || cur == first,
                  "pa_decode_shared: a group's members map different pages on a claimed tile");
    }
  }
  const ShareTables tb = share_tables(groups, B);
  const ShareLaunch sl = share_launch(tb.ntile, H, tb.max_tiles, TS);
  const size_t meta = align16(share_tables_cap(B) * sizeof(int32_t));
  LLM_REQUIRE(workspace && workspace_bytes >= meta &&
                  reinterpret_cast<uintptr_t>(workspace) % 16 == 0,
              "pa_decode_shared: workspace smaller than pa_decode_shared_workspace_bytes or not "
              "16-byte aligned");
  int32_t* dev = static_cast<int32_t*>(workspace);
  LLM_HIP_RET(hipMemcpy(dev, tb.image.data(), sizeof(int32_t) * tb.image.size(),
                        hipMemcpyHostToDevice));
  PaShared sh;
  sh.tiles = dev;
  sh.rows = dev + tb.rows_off;
  sh.first_tile = dev + tb.first_off;
  sh.ntile = sl.ntile, sh.npre = sl.npre, sh.bps = sl.bps;
  PaRequest rq = pa_request(kv, B, H, D, T, 0);
  rq.shared_pre = sl.npre;
  return pa_decode_internal(kv, rq, q, H * D, out, nullptr, context_lens, sm_scale,
                            static_cast<uint8_t*>(workspace) + meta, workspace_bytes - meta, st,
                            nullptr, nullptr, &sh);
}
