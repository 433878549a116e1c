// Tuning build only (make tune -> libllm_decoder_hip_tune.so; never in
// libllm_decoder_hip.so): the beam-group attention experiments that measured
// slower than the shipped BEAM form of pa_split_kernel, the
// tuning table the planner and pa_decode.hip read (pa_tuning.hpp: the switches
// from the environment; the hooks at the end of pa_split.hpp: tune_launch_form
// routes a beam-group launch to the experiment switched on), the pa_decode_tune
// A/B entry of the split kernel's register-stage / cache-policy variants
// (scripts/bench_kernels.py, scripts/tune_attention.py; each variant is the
// PaSplitCfg fields it changes), pa_plan_tune, the planner's test entry,
// prefill_passes_tune, the prefill pass packer's, serve_plan_sim_tune, the
// continuous-batching scheduler's, beam_book_tune, the beam search
// bookkeeping's, oproj_head_slices_tune, the fused o_proj's W_o layout, and
// pa_rows_tune, the internal attention entries with their row outputs.
#include <cmath>

#include "tune/pa_decode_tune.hpp"
#include "tune/pa_beam_steal.hpp"
#include "beam_plan.hpp"
#include "oproj_slices.hpp"
#include "pa_tuning.hpp"
#include "prefill_pack.hpp"
#include "serve_plan.hpp"

namespace llm {

// Beam-group attention, one WAVE per (group of 4 beams, head, split): the
// wave loads each KV page ONCE into registers and runs the math of every beam
// that reads it (row_group 4, fp16 pools, pages <= 8 KiB).  A split's work is
// a list of page items: a page all 4 beams share (the group's leading tiles
// whose page ids agree in all 4 rows -- a forked prefix) is one item for all 4
// beams; a beam-private page is one item for its beam.  The items of a
// (group, head) are cut into nsplit equal runs (equal HBM bytes per wave:
// every item is one page), so no LDS, no barrier and no per-beam re-load;
// each beam keeps its own online-softmax state and the wave writes one split
// partial per beam, merged by pa_merge_row_kernel (every split holds one).
// Groups whose rows differ in context, route outside the table or do not all
// exist take the same kernel beam by beam (items of one beam, its own context,
// its own equal split of its tiles).
// Maths per beam as pa_split_kernel (log2 units, row groups of the wave merged
// at the end), so results match the plain schedule up to the split boundaries.
// MINW: waves per SIMD asked of the register allocator; U: page items per
// register stage (two stages in flight).
template <int D, int TS, int MINW = 2, int U = 1>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MINW))) void pa_beam4_kernel(PaSplitArgs a) {
  constexpr int G = 4;
  constexpr int EPL = 8;  // fp16 elements per 16-byte lane load
  constexpr int LPT = D / EPL;
  constexpr int TPI = 64 / LPT;
  constexpr int NI = TS / TPI;
  constexpr int PAGE_BYTES = TS * D * 2;
  static_assert(LPT >= 1 && LPT <= 64 && TS % TPI == 0 && NI >= 1 && PAGE_BYTES <= 8192,
                "pa_beam4_kernel: fp16 pages of 1..8 KiB");
  const int lane = lane_id();
  const int wid = blockIdx.x * 4 + wave_id_uniform();
  const int s = wid % a.nsplit;
  const int gh = wid / a.nsplit;
  const int h = gh % a.H;
  const int grp = gh / a.H;
  if (grp >= (a.B + G - 1) / G) return;
  const int b0 = grp * G;
  const int c = lane % LPT;
  const int g = lane / LPT;

  // the group's rows (wave-uniform): page-table row, context, existence
  int prow_off[G], Tg[G];
  bool live[G];
  bool share = true;
#pragma unroll
  for (int i = 0; i < G; ++i) {
    const int bi = b0 + i;
    live[i] = bi < a.B;
    int ri = -1, Ti = 0;
    if (live[i]) {
      ri = a.beam_ids ? a.beam_ids[bi] : bi;
      Ti = a.context_lens ? a.context_lens[bi] : a.T;
      Ti = min(max(Ti, 0), a.T);
    }
    const bool rok = ri >= 0 && ri < a.num_beams;
    prow_off[i] = rok ? (ri * a.H + h) * a.max_tiles : -1;
    Tg[i] = rok ? Ti : 0;  // a row outside the table reads nothing (all pages missing)
    if (!live[i] || !rok || Ti != Tg[0]) share = false;
  }

  // q of each beam (dims c*8 .. c*8+7), pre-scaled into log2 units
  float qv[G][EPL];
#pragma unroll
  for (int i = 0; i < G; ++i) {
    const float* qp = a.q + (size_t)min(b0 + i, a.B - 1) * a.q_stride + (size_t)h * D + c * EPL;
    const f32x4 q0 = *reinterpret_cast<const f32x4*>(qp);
    const f32x4 q1 = *reinterpret_cast<const f32x4*>(qp + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      qv[i][e] = q0[e] * a.qscale;
      qv[i][4 + e] = q1[e] * a.qscale;
    }
  }
  float m[G], l[G], acc[G][EPL];
#pragma unroll
  for (int i = 0; i < G; ++i) {
    m[i] = kNegSentinel;
    l[i] = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[i][e] = 0.f;
  }
  const uint32_t lane_off = (uint32_t)lane * 16u;

  // One segment = a list of <= 128 page items, lane j holding item j and 64 + j
  // (page id, and tile << 4 | beam mask); shared groups have one segment,
  // the others one per beam.
  const int nseg = share ? 1 : G;
  for (int seg = 0; seg < nseg; ++seg) {
    int i0 = 0, cnt = 0, nsh = 0, ntiles = 0;
    if (share) {
      ntiles = min((Tg[0] + TS - 1) / TS, a.max_tiles);
      for (int blk = 0; blk < ntiles; blk += 64) {  // the shared prefix, 64 tiles per round
        const int t = blk + lane;
        bool eq = t < ntiles;
        if (eq) {
          const int32_t p0 = a.page_table[prow_off[0] + t];
#pragma unroll
          for (int i = 1; i < G; ++i) eq = eq && a.page_table[prow_off[i] + t] == p0;
        }
        const uint64_t mk = __ballot(eq);
        const int run = mk == ~0ull ? 64 : __builtin_ctzll(~mk);
        nsh = blk + run;
        if (run < 64) break;
      }
      nsh = min(nsh, ntiles);
      const int items = nsh + G * (ntiles - nsh);
      i0 = (int)(((long long)items * s) / a.nsplit);
      cnt = (int)(((long long)items * (s + 1)) / a.nsplit) - i0;
    } else {
      if (prow_off[seg] < 0) continue;  // no such row / outside the table: a neutral partial
      ntiles = min((Tg[seg] + TS - 1) / TS, a.max_tiles);
      const int pps = row_pps(0, a.nsplit, ntiles);
      i0 = s * pps;
      cnt = min(pps, ntiles - i0);
    }
    cnt = min(cnt, kMaxPps);  // the host sizes nsplit so a split holds <= 128 items
    if (cnt <= 0) continue;
    const int npriv = ntiles - nsh;
    int pid[2], inf[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int j = lane + 64 * r;
      pid[r] = -1;
      inf[r] = 0;
      if (j < cnt) {
        const int k = i0 + j;
        int tile, beam, mask;
        if (!share) {
          tile = k; beam = seg; mask = 1 << seg;
        } else if (k < nsh) {
          tile = k; beam = 0; mask = 0xF;
        } else {  // beam-major: a beam's private tiles are consecutive items
          const int p = k - nsh;
          beam = p / npriv; tile = nsh + p % npriv; mask = 1 << beam;
        }
        int id = a.page_table[prow_off[beam] + tile];
        pid[r] = id >= a.num_pages ? -1 : id;
        inf[r] = (tile << 4) | mask;
      }
    }
    auto item_pid = [&](int j) {
      return j < 64 ? __builtin_amdgcn_readlane(pid[0], j) : __builtin_amdgcn_readlane(pid[1], j - 64);
    };
    auto item_inf = [&](int j) {
      return j < 64 ? __builtin_amdgcn_readlane(inf[0], j) : __builtin_amdgcn_readlane(inf[1], j - 64);
    };
    auto issue = [&](u32x4 (&kk)[NI], u32x4 (&vv)[NI], int j) {
      const int pg = j < cnt ? item_pid(min(j, kMaxPps - 1)) : -1;
      const bool ok = pg >= 0;
      const size_t off = (size_t)(ok ? pg : 0) * a.page_stride;
      const auto krs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.k_pool + off), (short)0,
                                                         ok ? PAGE_BYTES : 0, 0x00020000);
      const auto vrs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.v_pool + off), (short)0,
                                                         ok ? PAGE_BYTES : 0, 0x00020000);
#pragma unroll
      for (int i = 0; i < NI; ++i)
        kk[i] = __builtin_amdgcn_raw_buffer_load_b128(krs, lane_off + i * 1024, 0, kKvLoadAux);
#pragma unroll
      for (int i = 0; i < NI; ++i)
        vv[i] = __builtin_amdgcn_raw_buffer_load_b128(vrs, lane_off + i * 1024, 0, kKvLoadAux);
    };
    // one page item for beam bi: scores, online softmax, p.v (pa_split_kernel maths)
    auto beam_math = [&](auto full_tag, auto beam_tag, const u32x4 (&kk)[NI],
                         const u32x4 (&vv)[NI], bool ok, int tok_base, int Tb) {
      constexpr bool FULL = decltype(full_tag)::value;
      constexpr int bi = decltype(beam_tag)::value;
      float sc[NI];
      bool valid[NI];
      float mloc = kNegSentinel;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) d = fmaf(qv[bi][e], kv_at<LLM_F16>(kk[i], e), d);
        d = group_sum<LPT>(d);
        valid[i] = FULL || (ok && (tok_base + i * TPI) < Tb);
        sc[i] = valid[i] ? d : kNegSentinel;
        mloc = fmaxf(mloc, sc[i]);
      }
      const float mnew = fmaxf(m[bi], mloc);
      const float corr = __builtin_amdgcn_exp2f(m[bi] - mnew);
      l[bi] *= corr;
#pragma unroll
      for (int e = 0; e < EPL; ++e) acc[bi][e] *= corr;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const float p = valid[i] ? __builtin_amdgcn_exp2f(sc[i] - mnew) : 0.f;
        l[bi] += p;
        const u32x4 vraw = FULL || valid[i] ? vv[i] : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[bi][e] = fmaf(p, kv_at<LLM_F16>(vraw, e), acc[bi][e]);
      }
      m[bi] = mnew;
    };
    auto compute = [&](const u32x4 (&kk)[NI], const u32x4 (&vv)[NI], int j) {
      const int pg = item_pid(min(j, kMaxPps - 1));
      const int info = item_inf(min(j, kMaxPps - 1));
      const int tile = info >> 4, mask = info & 0xF;
      const bool ok = pg >= 0;
      const int Tb = share ? Tg[0] : Tg[seg];
      const bool full = ok && (tile + 1) * TS <= Tb;
      const int tok_base = tile * TS + g;
      auto each = [&](auto beam_tag) {
        constexpr int bi = decltype(beam_tag)::value;
        if (mask & (1 << bi)) {
          if (full)
            beam_math(std::true_type{}, beam_tag, kk, vv, ok, tok_base, Tb);
          else
            beam_math(std::false_type{}, beam_tag, kk, vv, ok, tok_base, Tb);
        }
      };
      each(std::integral_constant<int, 0>{});
      each(std::integral_constant<int, 1>{});
      each(std::integral_constant<int, 2>{});
      each(std::integral_constant<int, 3>{});
    };
    u32x4 kA[U][NI], vA[U][NI], kB[U][NI], vB[U][NI];
    auto issue_st = [&](u32x4 (&kk)[U][NI], u32x4 (&vv)[U][NI], int j0) {
#pragma unroll
      for (int u = 0; u < U; ++u) issue(kk[u], vv[u], j0 + u);  // past the end: no bytes
    };
    auto compute_st = [&](const u32x4 (&kk)[U][NI], const u32x4 (&vv)[U][NI], int j0) {
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (j0 + u < cnt) compute(kk[u], vv[u], j0 + u);
    };
    issue_st(kA, vA, 0);
    for (int j = 0; j < cnt; j += 2 * U) {
      issue_st(kB, vB, j + U);
      compute_st(kA, vA, j);
      if (j + U >= cnt) break;
      issue_st(kA, vA, j + 2 * U);
      compute_st(kB, vB, j + U);
    }
  }

  // Per beam: merge the TPI row groups of the wave, write the split partial.
#pragma unroll
  for (int i = 0; i < G; ++i) {
#pragma unroll
    for (int off = LPT; off < 64; off <<= 1) {
      const float mo = __shfl_xor(m[i], off, 64);
      const float lo = __shfl_xor(l[i], off, 64);
      const float mn = fmaxf(m[i], mo);
      const float ca = __builtin_amdgcn_exp2f(m[i] - mn);
      const float cb = __builtin_amdgcn_exp2f(mo - mn);
      l[i] = l[i] * ca + lo * cb;
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        const float ao = __shfl_xor(acc[i][e], off, 64);
        acc[i][e] = acc[i][e] * ca + ao * cb;
      }
      m[i] = mn;
    }
    if (!live[i]) continue;
    const size_t pidx = ((size_t)(b0 + i) * a.H + h) * a.nsplit + s;
    if (lane < LPT) {
      float* o = a.part_acc + pidx * D + c * EPL;
      *reinterpret_cast<f32x4*>(o) = f32x4{acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
      *reinterpret_cast<f32x4*>(o + 4) = f32x4{acc[i][4], acc[i][5], acc[i][6], acc[i][7]};
    }
    if (lane == 0) {
      a.part_ml[pidx * 2] = m[i];
      a.part_ml[pidx * 2 + 1] = l[i];
    }
  }
}

// Tuning build only (LLM_BEAM_MFMA=1): measured slower than the VALU BEAM form
// it was written to replace (69.8 vs 60.8 us per C4 launch;
// loads alone 60.2 us, processing alone 48.3 us, both bound by what 2 waves
// per SIMD keep in flight).  Parity-green (fp32-grade against float64).
//
// MFMA beam-group kernel (row_group 4, fp16 KV, D 128, page 16): the 4 beams
// of a sequence for one (head, split) in one workgroup, as pa_split_kernel's
// BEAM form, but the q.k and p.v products run on the matrix cores, so a page
// costs the same few instructions whether it serves 1 beam or 4 (the VALU form
// spends 4 waves x ~90 instructions on every shared page: VALU/issue-bound,
// VERDICT r1).  Per page (16 tokens):
//   S^T[token][c] = K[token][:] . Qc[:]   4 x v_mfma_f32_16x16x32_f16; columns
//       c = b (beam b, q rounded to fp16) and c = 4 + b (the fp16 residual of
//       beam b's q, scaled by 2^13), summed with one lane shift: fp32-grade scores from
//       fp16 operands (K is fp16; products are exact in fp32)
//   online softmax per beam column in fp32 (the C layout puts a beam's 16
//       scores in 4 lanes x 4 registers)
//   O^T[d][c] += V^T[d][token] . P^T[token][c]   8 x v_mfma_f32_16x16x16_f16;
//       P^T is the score tile itself (same lanes: no movement), column b holding
//       fp16(p), column 4 + b the fp16 residual of p (summed once at the end);
//       V^T comes from a per-wave LDS image of the page read with
//       ds_read_b64_tr_b16 (the hardware transpose read), XOR-swizzled rows
// The 4 waves take the split's work items round-robin: a page all 4 beams
// share (leading shared run, as the BEAM form) is one item for all 4 beam
// columns; a beam-private page is one item masked to its beam.  Each item is
// loaded once, 1 KiB contiguous per instruction, into registers (two items in
// flight per wave), then into the wave's swizzled LDS images of K (read back
// as MFMA rows) and V (read back transposed).  The 4 waves' (m, l, acc) per beam
// are combined through LDS in a fixed order and written as the split's
// partial, which pa_merge_row_kernel consumes exactly as the VALU form's.
// Rows of a workgroup whose contexts differ (or that do not exist) fall back
// to one wave per beam with its own pages (items masked to that beam).
__device__ __forceinline__ uint32_t beam_lds_off(int row, int ch) {
  // 256-byte token rows, 16-byte chunk ch: XOR swizzle so the transposed reads
  // (4 rows x 32 bytes per 16-lane group) spread over the banks
  return (uint32_t)(256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))));
}

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// Maximum over each 16-lane row (DPP, every lane of the row gets it).
__device__ __forceinline__ float row_max16(float x) {
  x = fmaxf(x, mov_dpp<0xB1>(x));   // quad_perm [1,0,3,2]
  x = fmaxf(x, mov_dpp<0x4E>(x));   // quad_perm [2,3,0,1]
  x = fmaxf(x, mov_dpp<0x141>(x));  // row_half_mirror
  return fmaxf(x, mov_dpp<0x140>(x));  // row_mirror
}
// The residual columns carry (x - fp16(x)) * 2^13: unscaled they would sit
// below fp16's normal range (~1e-5 for q, p * 2^-12 for the weights) and
// lose bits as subnormals.  Exact power-of-two scaling; |x| < 8192 keeps the
// scaled residual finite.  Measured against float64
// (scripts/debug_beam_mfma.py): 1.4e-7 .. 6.5e-7, as the VALU kernel.
// Values below fp16's smallest normal go to the residual column whole.
constexpr float kLoScale = 8192.f, kLoUnscale = 1.f / 8192.f;
constexpr float kF16MinNormal = 6.103515625e-05f;

// DBG (tuning build only): 1 = loads with a trivial consumer, 2 = processing
// with no loads (zero pages)
template <int DBG = 0>
__global__ __launch_bounds__(256) void pa_beam_mfma_kernel(PaSplitArgs a) {
  constexpr int D = 128, TS = 16;
  constexpr int PAGE_BYTES = TS * D * 2;  // 4 KiB
  __shared__ __attribute__((aligned(16))) uint8_t vimg[4][PAGE_BYTES];  // per wave
  __shared__ __attribute__((aligned(16))) uint8_t kimg[4][PAGE_BYTES];
  __shared__ __attribute__((aligned(16))) _Float16 pimg[4][16 * 16];
  __shared__ int pid_lds[4][kMaxPps];
  __shared__ int pfx_lds[4][64];

  const int lane = lane_id();
  const int w = wave_id_uniform();
  const int s = blockIdx.x % a.nsplit;
  const int gh = blockIdx.x / a.nsplit;
  const int h = gh % a.H;
  const int g0 = (gh / a.H) * 4;
  const int b = g0 + w;  // this wave's beam row
  const bool brow = b < a.B;

  // share: all 4 rows exist, route to valid page-table rows and hold equal
  // contexts (uniform over the workgroup)
  bool share = true;
  int T0 = -1;
  for (int i = 0; i < 4; ++i) {
    const int bi = g0 + i;
    if (bi >= a.B) { share = false; break; }
    const int ri = a.beam_ids ? a.beam_ids[bi] : bi;
    int Ti = a.context_lens ? a.context_lens[bi] : a.T;
    Ti = min(max(Ti, 0), a.T);
    if (ri < 0 || ri >= a.num_beams || (i > 0 && Ti != T0)) { share = false; break; }
    T0 = Ti;
  }
  const int r = brow ? (a.beam_ids ? a.beam_ids[b] : b) : -1;
  int Tb = brow ? (a.context_lens ? a.context_lens[b] : a.T) : 0;
  Tb = min(max(Tb, 0), a.T);
  const int ntiles = min((Tb + TS - 1) / TS, a.max_tiles);
  int tile0, count;
  {
    const int pps = row_pps(a.pps, a.nsplit, ntiles);
    tile0 = s * pps;
    count = min(pps, ntiles - tile0);
  }
  const int32_t* prow =
      (r >= 0 && r < a.num_beams) ? a.page_table + ((size_t)r * a.H + h) * a.max_tiles : nullptr;
  if (share && a.balance16 >= 16 && a.pps == 0 && a.nsplit > 1 && ntiles > 0) {
    // cost-balanced split boundaries over the group's shared prefix (every
    // input uniform: all splits of the group derive the same partition)
    int nsh_t = 0;
    for (int blk = 0;; blk += 64) {
      const int t = blk + lane;
      int id = -1;
      if (t < ntiles) {
        id = prow[t];
        if (id >= a.num_pages) id = -1;
      }
      pfx_lds[w][lane] = id;
      __syncthreads();
      const bool eq = t < ntiles && pfx_lds[0][lane] == pfx_lds[1][lane] &&
                      pfx_lds[0][lane] == pfx_lds[2][lane] && pfx_lds[0][lane] == pfx_lds[3][lane];
      const uint64_t mk = __ballot(eq);
      __syncthreads();
      const int run = mk == ~0ull ? 64 : __builtin_ctzll(~mk);
      nsh_t = blk + run;
      if (run < 64 || blk + 64 >= ntiles) break;
    }
    nsh_t = min(nsh_t, ntiles);
    if (nsh_t > 0 && nsh_t < ntiles) {
      const long long A = 16, P = a.balance16, ns = a.nsplit;
      const long long C = A * nsh_t + P * (ntiles - nsh_t);
      auto start = [&](int k) -> int {
        if (k <= 0) return 0;
        if (k >= ns) return ntiles;
        const long long x = (C * k + ns - 1) / ns;
        if (x <= A * nsh_t) return (int)((x + A - 1) / A);
        return (int)min<long long>(ntiles, nsh_t + (x - A * nsh_t + P - 1) / P);
      };
      if ((C + ns - 1) / ns / A + 2 <= kMaxPps) {
        tile0 = start(s);
        count = start(s + 1) - tile0;
      }
    }
  }
  count = max(count, 0);

  // this split's page ids of every beam row of the group (-1: missing)
  for (int j = lane; j < kMaxPps; j += 64) {
    int id = -1;
    if (prow && j < count) {
      id = prow[tile0 + j];
      if (id >= a.num_pages) id = -1;
    }
    pid_lds[w][j] = id;
  }
  __syncthreads();

  // work items of this wave
  int nsh = 0, nitems, it0, istep;
  if (share) {
    while (nsh < count && pid_lds[0][nsh] == pid_lds[1][nsh] && pid_lds[0][nsh] == pid_lds[2][nsh] &&
           pid_lds[0][nsh] == pid_lds[3][nsh])
      ++nsh;
    nitems = nsh + 4 * (count - nsh);
    it0 = w;
    istep = 4;
  } else {
    nitems = count;
    it0 = 0;
    istep = 1;
  }
  nsh = __builtin_amdgcn_readfirstlane(nsh);
  // item -> (tile j, page, beam mask)
  auto item = [&](int i, int& j, int& pg, int& mask) {
    if (i >= nitems) { j = 0; pg = -1; mask = 0; return; }
    if (!share) { j = i; pg = pid_lds[w][j]; mask = 1 << w; return; }
    if (i < nsh) { j = i; pg = pid_lds[0][j]; mask = 0xF; return; }
    const int i2 = i - nsh;
    const int bb = i2 & 3;
    j = nsh + (i2 >> 2);
    pg = pid_lds[bb][j];
    mask = 1 << bb;
  };

  // q operands (A of the score MFMAs, rows = beams): lane row c = lane & 15,
  // c < 4: beam g0 + c, other rows 0; qh = fp16(q), ql = its fp16 residual
  // (scaled); k-step kk holds dims 32 kk + 8 (lane >> 4) .. + 7 (the K
  // operand's k order)
  const int col = lane & 15;
  const int lgrp = lane >> 4;
  f16x8 qh[4], ql[4];
  {
    const int qb = g0 + col;
    const bool qok = col < 4 && qb < a.B;
    const float* qp = a.q + (size_t)(qok ? qb : 0) * a.q_stride + (size_t)h * D;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float v = qok ? qp[32 * kk + 8 * lgrp + e] * a.qscale : 0.f;
        const _Float16 hi = fabsf(v) >= kF16MinNormal ? (_Float16)v : (_Float16)0.f;
        qh[kk][e] = hi;
        ql[kk][e] = (_Float16)((v - (float)hi) * kLoScale);
      }
    }
  }

  // online-softmax state of beam r in register r (lanes 0..15, identical)
  float m4[4], l4[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m4[r] = kNegSentinel;
    l4[r] = 0.f;
  }
  f32x4 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  // P^T image of the wave: rows = beam columns (0..3 fp16(p), 4..7 residual,
  // 8..15 zero) x 16 tokens
  _Float16* pw = pimg[w];
  for (int i2 = 128 + lane; i2 < 256; i2 += 64) pw[i2] = (_Float16)0.f;
  uint8_t* vw = vimg[w];
  uint8_t* kw = kimg[w];

  struct Stage {
    u32x4 k[4], v[4];
  };
  auto issue = [&](Stage& st, int i) {
    int j, pg, mask;
    item(i, j, pg, mask);
    const bool ok = pg >= 0 && DBG != 2;
    const size_t off = (size_t)(ok ? pg : 0) * a.page_stride;
    const auto krs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.k_pool + off), (short)0,
                                                       ok ? PAGE_BYTES : 0, 0x00020000);
    const auto vrs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.v_pool + off), (short)0,
                                                       ok ? PAGE_BYTES : 0, 0x00020000);
    // K and V: linear 1 KiB per instruction (token 4 c + lgrp, chunk col)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      st.k[c] = __builtin_amdgcn_raw_buffer_load_b128(krs, (uint32_t)(c * 1024 + lane * 16), 0,
                                                       kKvLoadAux);
      st.v[c] = __builtin_amdgcn_raw_buffer_load_b128(vrs, (uint32_t)(c * 1024 + lane * 16), 0,
                                                       kKvLoadAux);
    }
  };
  auto process = [&](const Stage& st, int i) {
    if constexpr (DBG == 1) {
      uint32_t x = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) x ^= st.k[c][0] ^ st.v[c][3];
      acc[0][0] += (float)(x & 1u);
      return;
    }
    int j, pg, mask;
    item(i, j, pg, mask);
    const bool ok = pg >= 0;
    const int tok0 = (tile0 + j) * TS;
    // FULL (uniform): the page is present and all 16 tokens are inside the
    // context: no per-token masks (all pages of a row but its last)
    const bool full = ok && tok0 + TS <= Tb;
    // K and V images (V rows past the context or of a missing page: zeros,
    // so stale NaN / Inf cannot reach the MFMA; such K rows are masked)
    if (full) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        *reinterpret_cast<u32x4*>(kw + beam_lds_off(4 * c + lgrp, col)) = st.k[c];
        *reinterpret_cast<u32x4*>(vw + beam_lds_off(4 * c + lgrp, col)) = st.v[c];
      }
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int row = 4 * c + lgrp;
        const bool vok = ok && tok0 + row < Tb;
        *reinterpret_cast<u32x4*>(kw + beam_lds_off(row, col)) = st.k[c];
        *reinterpret_cast<u32x4*>(vw + beam_lds_off(row, col)) =
            vok ? st.v[c] : u32x4{0u, 0u, 0u, 0u};
      }
    }
    // scores S[beam r][token] in lanes 0..15 (token = lane), register r:
    // A = q rows, B = K^T (token column col, dims 32 kk + 8 lgrp .. + 7)
    f32x4 sh = f32x4{0.f, 0.f, 0.f, 0.f}, sl = sh;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const f16x8 kf = __builtin_bit_cast(
          f16x8, *reinterpret_cast<const u32x4*>(kw + beam_lds_off(col, 4 * kk + lgrp)));
      sh = __builtin_amdgcn_mfma_f32_16x16x32_f16(qh[kk], kf, sh, 0, 0, 0);
      sl = __builtin_amdgcn_mfma_f32_16x16x32_f16(ql[kk], kf, sl, 0, 0, 0);
    }
    // per-beam online softmax: the 16 tokens of beam r sit in one DPP row
    const bool tok_ok = lane < 16 && (full || (ok && tok0 + lane < Tb));
    float p[4], corr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool valid = tok_ok && ((mask >> r) & 1);
      const float sv = valid ? sh[r] + sl[r] * kLoUnscale : kNegSentinel;
      const float mnew = fmaxf(m4[r], row_max16(sv));
      corr[r] = __builtin_amdgcn_exp2f(m4[r] - mnew);
      p[r] = valid ? __builtin_amdgcn_exp2f(sv - mnew) : 0.f;
      l4[r] = l4[r] * corr[r] + group_sum<16>(p[r]);
      m4[r] = mnew;
    }
    if (lane < 16) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const _Float16 hi = p[r] >= kF16MinNormal ? (_Float16)p[r] : (_Float16)0.f;
        pw[r * 16 + lane] = hi;
        pw[(4 + r) * 16 + lane] = (_Float16)((p[r] - (float)hi) * kLoScale);
      }
    }
    // rescale the accumulators only when some beam's maximum moved (after the
    // first pages of a split, almost never): corr is exactly 1 otherwise
    if (__ballot(corr[0] != 1.f || corr[1] != 1.f || corr[2] != 1.f || corr[3] != 1.f)) {
      const float c0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(corr[0]), 0));
      const float c1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(corr[1]), 0));
      const float c2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(corr[2]), 0));
      const float c3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(corr[3]), 0));
      const int bcol = col & 3;
      const float cc = bcol == 0 ? c0 : bcol == 1 ? c1 : bcol == 2 ? c2 : c3;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] *= cc;
    }
    // P^T operand: beam column col, tokens 4 lgrp .. + 3
    const f16x4 pf = *reinterpret_cast<const f16x4*>(pw + col * 16 + 4 * lgrp);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      // V^T operand of dims 16 i .. 16 i + 15: lane 4 qq + pp of group lgrp
      // addresses token row 4 lgrp + qq, dims 16 i + 4 pp .. + 3
      const int qq = col >> 2, pp = col & 3;
      const uint32_t ad = beam_lds_off(4 * lgrp + qq, 2 * i + (pp >> 1)) + 8 * (pp & 1);
      const s16x4 vt = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4*)(vw + ad));
      acc[i] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(f16x4, vt), pf, acc[i],
                                                      0, 0, 0);
    }
  };

  {
    Stage sa, sb;
    int i = it0;
    issue(sa, i);
    while (i < nitems) {
      issue(sb, i + istep);  // past the end: nothing loaded (num_records 0)
      process(sa, i);
      i += istep;
      if (i >= nitems) break;
      issue(sa, i + istep);
      process(sb, i);
      i += istep;
    }
  }

  // beam column b: fp16 part + residual part (columns b and b + 4)
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[i][q] += __shfl_down(acc[i][q], 4, 16) * kLoUnscale;

  // combine the 4 waves' states per beam through LDS (each wave reuses its own
  // V image: acc [beam][128] then (m, l) [beam][2])
  float* red = reinterpret_cast<float*>(vw);
  if (col < 4) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) red[col * D + 16 * i + 4 * lgrp + q] = acc[i][q];
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        red[4 * D + 2 * r] = m4[r];
        red[4 * D + 2 * r + 1] = l4[r];
      }
    }
  }
  __syncthreads();
  if (brow) {
    float mv[4], M = kNegSentinel;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      mv[v] = reinterpret_cast<const float*>(vimg[v])[4 * D + 2 * w];
      M = fmaxf(M, mv[v]);
    }
    float L = 0.f, o0 = 0.f, o1 = 0.f;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float* rv = reinterpret_cast<const float*>(vimg[v]);
      const float e = __builtin_amdgcn_exp2f(mv[v] - M);
      L += rv[4 * D + 2 * w + 1] * e;
      o0 += rv[w * D + 2 * lane] * e;
      o1 += rv[w * D + 2 * lane + 1] * e;
    }
    const size_t pidx = ((size_t)b * a.H + h) * a.nsplit + s;
    *reinterpret_cast<float2*>(a.part_acc + pidx * D + 2 * lane) = float2{o0, o1};
    if (lane == 0) {
      a.part_ml[pidx * 2] = M;
      a.part_ml[pidx * 2 + 1] = L;
    }
  }
}

#ifndef BEAM4_MINW
#define BEAM4_MINW 2
#endif
#ifndef BEAM4_U
#define BEAM4_U 1
#endif

template <int D, int TS>
long long beam4_resident_waves() {
  if constexpr (TS * D * 2 > 8192) {
    return 0;
  } else {
  static long long cached = 0;
  if (cached) return cached;
  int dev = 0, cus = 0, blocks = 0;
  if (hipGetDevice(&dev) == hipSuccess &&
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, pa_beam4_kernel<D, TS, BEAM4_MINW, BEAM4_U>, 256, 0) ==
          hipSuccess &&
      cus > 0 && blocks > 0) {
    cached = (long long)cus * blocks * 4;
  } else {
    (void)hipGetLastError();
    cached = 256LL * 4 * 3;
  }
  return cached;
  }
}


long long tune_beam4_resident_for(int D, int TS) {
  auto by_ts = [&](auto d) -> long long {
    constexpr int DD = decltype(d)::value;
    return TS == 16 ? beam4_resident_waves<DD, 16>() : beam4_resident_waves<DD, 32>();
  };
  switch (D) {
    case 32: return by_ts(std::integral_constant<int, 32>{});
    case 64: return by_ts(std::integral_constant<int, 64>{});
    case 128: return by_ts(std::integral_constant<int, 128>{});
    default: return by_ts(std::integral_constant<int, 256>{});
  }
}

hipError_t tune_launch_beam4(const PaSplitArgs& a, int D, int TS, hipStream_t st) {
  const int waves4 = ((a.B + 3) / 4) * a.H * a.nsplit;
  const dim3 grid((waves4 + 3) / 4), block(256);
  auto go = [&](auto d, auto ts) {
    constexpr int DD = decltype(d)::value, TT = decltype(ts)::value;
    if constexpr (TT * DD * 2 <= 8192)
      hipLaunchKernelGGL((pa_beam4_kernel<DD, TT, BEAM4_MINW, BEAM4_U>), grid, block, 0, st, a);
  };
  auto by_ts = [&](auto d) {
    if (TS == 16) go(d, std::integral_constant<int, 16>{});
    else go(d, std::integral_constant<int, 32>{});
  };
  switch (D) {
    case 32: by_ts(std::integral_constant<int, 32>{}); break;
    case 64: by_ts(std::integral_constant<int, 64>{}); break;
    case 128: by_ts(std::integral_constant<int, 128>{}); break;
    default: by_ts(std::integral_constant<int, 256>{}); break;
  }
  return hipGetLastError();
}

hipError_t tune_launch_beam_mfma(const PaSplitArgs& a, dim3 grid, hipStream_t st) {
  static const int dbg = env_int("LLM_BEAM_MFMA_DBG", 0);
  if (dbg == 1)
    hipLaunchKernelGGL(pa_beam_mfma_kernel<1>, grid, dim3(256), 0, st, a);
  else if (dbg == 2)
    hipLaunchKernelGGL(pa_beam_mfma_kernel<2>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(pa_beam_mfma_kernel<0>, grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t tune_launch_beam_loads_only(const PaSplitArgs& a, dim3 grid, hipStream_t st) {
  // (the cost-balanced contiguous splits, as kBeamContiguous below)
  constexpr PaSplitCfg kLoadsOnly{.chunk_bytes = LLM_BEAM_CHUNK, .min_waves = LLM_BEAM_WAVES,
                                  .load_only = true, .beam = true};
  hipLaunchKernelGGL((pa_split_kernel<128, 16, kLoadsOnly>), grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

// The shipped BEAM form with its shared chunks delivered by an LDS-DMA ring
// of `ring` 8 KiB chunks (pa_split_kernel RING; LLM_BEAM_RING = 3 / 4 / 6 / 8,
// LLM_BEAM_DIAG = 2: the same with a trivial consumer).
hipError_t tune_launch_beam_ring(const PaSplitArgs& a, dim3 grid, hipStream_t st, int ring,
                                 bool load_only) {
  auto go = [&](auto r, auto lo) {
    constexpr int R = decltype(r)::value;
    constexpr bool LO = decltype(lo)::value;
    constexpr PaSplitCfg kRing{.chunk_bytes = 8192, .load_only = LO, .beam = true, .ring = R,
                               .interleave = true, .prio = true};
    hipLaunchKernelGGL((pa_split_kernel<128, 16, kRing>), grid, dim3(256), 0, st, a);
  };
  auto by_ring = [&](auto lo) {
    switch (ring) {
      case 3: go(std::integral_constant<int, 3>{}, lo); break;
      case 6: go(std::integral_constant<int, 6>{}, lo); break;
      case 8: go(std::integral_constant<int, 8>{}, lo); break;
      default: go(std::integral_constant<int, 4>{}, lo); break;
    }
  };
  if (load_only) by_ring(std::true_type{});
  else by_ring(std::false_type{});
  return hipGetLastError();
}

// The shipped BEAM form with per-wave timestamps (pa_split_kernel STAMPS,
// LLM_BEAM_STAMPS=1): entry / first KV load / shared prefix done / exit, and
// the wave's HW_ID, into a buffer pa_tune_stamps() copies out (diagnostics:
// allocates on first use, so not inside a graph capture).
static unsigned long long* g_stamps = nullptr;
static size_t g_stamps_cap = 0, g_stamps_waves = 0;

hipError_t tune_launch_beam_stamps(const PaSplitArgs& a0, dim3 grid, hipStream_t st) {
  const size_t waves = (size_t)grid.x * 4;
  if (waves > g_stamps_cap) {
    if (g_stamps) (void)hipFree(g_stamps);
    g_stamps = nullptr;
    g_stamps_cap = 0;
    if (hipMalloc(&g_stamps, waves * 5 * sizeof(unsigned long long)) != hipSuccess)
      return hipErrorOutOfMemory;
    g_stamps_cap = waves;
  }
  (void)hipMemsetAsync(g_stamps, 0, waves * 5 * sizeof(unsigned long long), st);
  PaSplitArgs a = a0;
  a.stamps = g_stamps;
  g_stamps_waves = waves;
  constexpr PaSplitCfg kStamped{.chunk_bytes = 8192, .beam = true, .stamps = true};
  constexpr PaSplitCfg kStampedIl{.chunk_bytes = 8192, .beam = true, .stamps = true, .interleave = true};
  constexpr PaSplitCfg kStampedIlPrio{.chunk_bytes = 8192, .beam = true, .stamps = true,
                                      .interleave = true, .prio = true};
  if (env_int("LLM_BEAM_INTERLEAVE", 1) == 0)
    hipLaunchKernelGGL((pa_split_kernel<128, 16, kStamped>), grid, dim3(256), 0, st, a);
  else if (env_int("LLM_BEAM_PRIO", 1) == 0)
    hipLaunchKernelGGL((pa_split_kernel<128, 16, kStampedIl>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((pa_split_kernel<128, 16, kStampedIlPrio>), grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

// The decoder's steal form (D 128, page 16) with per-wave stamps
// (pa_beam_steal_kernel STAMPS, 8 per wave; pa_tune_stamps8 copies them).
static unsigned long long* g_stamps8 = nullptr;
static size_t g_stamps8_cap = 0, g_stamps8_waves = 0;

hipError_t tune_launch_steal_stamps(const PaSplitArgs& a0, dim3 grid, hipStream_t st) {
  const size_t waves = (size_t)grid.x * 4;
  if (waves > g_stamps8_cap) {
    if (g_stamps8) (void)hipFree(g_stamps8);
    g_stamps8 = nullptr;
    g_stamps8_cap = 0;
    if (hipMalloc(&g_stamps8, waves * 8 * sizeof(unsigned long long)) != hipSuccess)
      return hipErrorOutOfMemory;
    g_stamps8_cap = waves;
  }
  (void)hipMemsetAsync(g_stamps8, 0, waves * 8 * sizeof(unsigned long long), st);
  PaSplitArgs a = a0;
  a.stamps = g_stamps8;
  g_stamps8_waves = waves;
  hipLaunchKernelGGL((pa_beam_steal_kernel<128, 16, kStealBatch, 4, true>), grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t tune_beam_mfma_occupancy(int* blocks) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, pa_beam_mfma_kernel<0>, 256, 0);
}

// ---------------------------------------------------------------------------
// The tuning table (pa_tuning.hpp): every switch read per launch (tests flip
// them in-process), except the beam balance, read once.
PaTuning pa_tuning() {
  static const int balance = [] {
    const int x = env_int("LLM_BEAM_BALANCE16", 44);
    return x >= 16 ? x : 0;
  }();
  static const int mfma_balance = [] {
    const int x = env_int("LLM_BEAM_MFMA_BALANCE16", 64);
    return x >= 16 ? x : 0;
  }();
  PaTuning t;
  t.wg_merge = env_int("LLM_WG_MERGE", 1) != 0;
  t.oproj_fuse = env_int("LLM_OPROJ_FUSE", 1) != 0;
  t.beam4 = env_int("LLM_BEAM4", 0) != 0;
  t.beam_mfma = env_int("LLM_BEAM_MFMA", 0) != 0;
  t.beam_steal = env_int("LLM_BEAM_STEAL", 0) == 1;
  t.beam_balance16 = balance;
  t.beam_mfma_balance16 = mfma_balance;
  t.beam_nsplit = env_int("LLM_BEAM_NSPLIT", 0);
  t.wgm_splits = env_int("LLM_WGM_SPLITS", 0);
  t.beam4_splits = env_int("LLM_BEAM4_SPLITS", 0);
  t.beam_smaj = env_int("LLM_BEAM_SMAJ", 1) != 0;
  return t;
}

bool tune_beam_occupancy(int D, int TS, int* blocks, hipError_t* e) {
  if (D != 128 || TS != 16 || !pa_tuning().beam_mfma) return false;
  *e = tune_beam_mfma_occupancy(blocks);
  return true;
}

unsigned* tune_steal_counters(size_t n) {
  static unsigned* buf = nullptr;
  static size_t cap = 0;
  if (!pa_tuning().beam_steal) return nullptr;
  if (n > cap) {
    if (buf) (void)hipFree(buf);
    buf = nullptr;
    cap = 0;
    if (hipMalloc(&buf, n * sizeof(unsigned)) != hipSuccess) return nullptr;
    if (hipMemset(buf, 0, n * sizeof(unsigned)) != hipSuccess) return nullptr;
    cap = n;
  }
  return buf;
}

namespace {
// the steal form (pa_beam_steal_kernel) of one (D, TS): LLM_STEAL_KB tiles per
// batch, LLM_STEAL_MINW=3 lifts the 128-VGPR cap, LLM_BEAM_STAMPS=1 stamps
template <int D, int TS>
hipError_t launch_steal(const PaSplitArgs& a, dim3 grid, hipStream_t st) {
  if constexpr (D == 128 && TS == 16) {
    if (env_int("LLM_BEAM_STAMPS", 0) == 1) return tune_launch_steal_stamps(a, grid, st);
  }
  const int kb = env_int("LLM_STEAL_KB", kStealBatch);
  if (env_int("LLM_STEAL_MINW", 0) == 3)
    hipLaunchKernelGGL((pa_beam_steal_kernel<D, TS, kStealBatch, 3>), grid, dim3(256), 0, st, a);
  else if (kb == 2) hipLaunchKernelGGL((pa_beam_steal_kernel<D, TS, 2>), grid, dim3(256), 0, st, a);
  else if (kb == 8) hipLaunchKernelGGL((pa_beam_steal_kernel<D, TS, 8>), grid, dim3(256), 0, st, a);
  else if (kb == 16) hipLaunchKernelGGL((pa_beam_steal_kernel<D, TS, 16>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((pa_beam_steal_kernel<D, TS>), grid, dim3(256), 0, st, a);
  return hipGetLastError();
}
}  // namespace

bool tune_launch_form(const PaSplitArgs& a, int D, int TS, dim3 grid, hipStream_t st,
                      hipError_t* e) {
  if (a.beam4) {  // pa_beam4_kernel: one wave per (group, head, split)
    *e = tune_launch_beam4(a, D, TS, st);
    return true;
  }
  if (a.steal && steal_shape_ok(D, TS)) {  // dynamic tile assignment (pa_beam_steal.hpp)
    if (D == 64 && TS == 16) *e = launch_steal<64, 16>(a, grid, st);
    else if (D == 128 && TS == 16) *e = launch_steal<128, 16>(a, grid, st);
    else if (D == 32 && TS == 32) *e = launch_steal<32, 32>(a, grid, st);
    else if (D == 64 && TS == 32) *e = launch_steal<64, 32>(a, grid, st);
    else if (D == 128 && TS == 32) *e = launch_steal<128, 32>(a, grid, st);
    else return false;
    return true;
  }
  if (D != 128 || TS != 16) return false;
  const PaTuning t = pa_tuning();
  if (t.beam_mfma) {
    PaSplitArgs am = a;
    am.balance16 = t.beam_mfma_balance16;
    *e = tune_launch_beam_mfma(am, grid, st);
    return true;
  }
  if (env_int("LLM_BEAM_DIAG", 0) == 1) {  // this form's loads, staging and barriers only
    *e = tune_launch_beam_loads_only(a, grid, st);
    return true;
  }
  if (env_int("LLM_BEAM_STAMPS", 0) == 1) {  // per-wave timestamps (scripts/beam_stamps.py)
    *e = tune_launch_beam_stamps(a, grid, st);
    return true;
  }
  const int ring = env_int("LLM_BEAM_RING", 0);
  if (ring > 0) {  // shared chunks through an LDS-DMA ring
    *e = tune_launch_beam_ring(a, grid, st, ring, env_int("LLM_BEAM_DIAG", 0) == 2);
    return true;
  }
  if (env_int("LLM_BEAM_PRIO", 1) == 0) {  // interleaved splits without the priority ranking
    constexpr PaSplitCfg kBeamNoPrio{.chunk_bytes = 8192, .beam = true, .interleave = true};
    hipLaunchKernelGGL((pa_split_kernel<128, 16, kBeamNoPrio>), grid, dim3(256), 0, st, a);
    *e = hipGetLastError();
    return true;
  }
  if (env_int("LLM_BEAM_INTERLEAVE", 1) == 0) {  // round 4's contiguous cost-balanced splits
    constexpr PaSplitCfg kBeamContiguous{.chunk_bytes = 8192, .beam = true};
    hipLaunchKernelGGL((pa_split_kernel<128, 16, kBeamContiguous>), grid, dim3(256), 0, st, a);
    *e = hipGetLastError();
    return true;
  }
  return false;
}

}  // namespace llm

using namespace llm;

// Tuning hook: the last steal-form stamps (8 per wave) into host; returns the
// waves copied (-1: none recorded).
extern "C" long long pa_tune_stamps8(unsigned long long* host, long long max_waves) {
  if (!g_stamps8 || !host) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  const size_t n = std::min<size_t>((size_t)max_waves, g_stamps8_waves);
  if (hipMemcpy(host, g_stamps8, n * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost) !=
      hipSuccess)
    return -1;
  return (long long)n;
}

// Tuning hook: the last LLM_BEAM_STAMPS launch's per-wave stamps (5 per wave,
// pa_split_kernel STAMPS) into host (room for max_waves); returns the waves
// copied (-1: none recorded).
extern "C" long long pa_tune_stamps(unsigned long long* host, long long max_waves) {
  if (!g_stamps || !host) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  const size_t n = std::min<size_t>((size_t)max_waves, g_stamps_waves);
  if (hipMemcpy(host, g_stamps, n * 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost) !=
      hipSuccess)
    return -1;
  return (long long)n;
}

// Tuning hook: the launch planner (pa_plan.hpp) for explicit request fields,
// so tests reach the row kinds the product ABI cannot ask for.  out_kind is a
// PaOut value, rows16 its OPROJ flag; a resident count < 0 is queried from the
// device, any other is taken as given.  The request passes pa_decode_internal's
// own checks first (over a view of these fields with placeholder pointers,
// which a plan-only call never reads).
// (pa_plan_window_tune: the same with the request's sliding window, PaRequest::window; 0: none.)
extern "C" int pa_plan_window_tune(int B, int H, int D, int T, int page_size, int max_tiles,
                                   int kv_dtype, int pages_per_split, int row_group, int window,
                                   int out_kind, int rows16, long long resident,
                                   long long beam_resident, long long beam4_resident, int* nsplit,
                                   int* form) {
  LLM_REQUIRE(nsplit && form, "pa_plan_window_tune: NULL output");
  LLM_REQUIRE(out_kind >= 0 && out_kind <= (int)PaOut::OPROJ, "pa_plan_window_tune: out_kind");
  *nsplit = *form = 0;
  static const int32_t placeholder = 0;
  pa_kv_view kv{};
  kv.k_pool = kv.v_pool = &placeholder;
  kv.page_table = &placeholder;
  kv.num_pages = 1 << 20;
  kv.num_beams = std::max(B, 1);
  kv.num_heads = H, kv.head_dim = D, kv.page_size = page_size, kv.max_tiles = max_tiles;
  kv.kv_dtype = kv_dtype;
  PaRequest rq = pa_request(&kv, B, H, D, T, pages_per_split, row_group, (PaOut)out_kind);
  rq.rows16 = rows16 != 0;
  rq.window = window;
  PaLaunch p;
  const int rc = pa_decode_internal(&kv, rq, nullptr, H * D, nullptr, nullptr, nullptr, 1.f,
                                    nullptr, 0, nullptr, nullptr, &p);
  if (rc != LLM_OK) return rc;
  if (pa_plan_device(rq, &p, resident, beam_resident, beam4_resident) != LLM_OK)
    return fail(LLM_ERR_UNSUPPORTED, "pa_plan_window_tune: more splits than a row may have");
  *nsplit = p.nsplit;
  *form = p.form();
  return LLM_OK;
}

// pa_plan_window_tune without a window.
extern "C" int pa_plan_tune(int B, int H, int D, int T, int page_size, int max_tiles, int kv_dtype,
                            int pages_per_split, int row_group, int out_kind, int rows16,
                            long long resident, long long beam_resident, long long beam4_resident,
                            int* nsplit, int* form) {
  return pa_plan_window_tune(B, H, D, T, page_size, max_tiles, kv_dtype, pages_per_split, row_group,
                             0, out_kind, rows16, resident, beam_resident, beam4_resident, nsplit,
                             form);
}

// Tuning hook: the prefill pass packer (prefill_pack.hpp) on explicit rows
// (start[i], len[i]), so a test reads the pass structure the decoder runs.
// out: (pass, row index, p0, len) per segment, the first `capacity` of them;
// returns the segment count (which may exceed capacity), -1 on bad arguments.
extern "C" int prefill_passes_tune(const int32_t* start, const int32_t* len, int nrows, int cap,
                                   int32_t* out, int capacity) {
  if (nrows < 0 || cap < 1 || capacity < 0 || (nrows && (!start || !len)) || (capacity && !out))
    return -1;
  for (int i = 0; i < nrows; ++i)
    if (start[i] < 0 || len[i] < 0) return -1;
  int n = 0, pi = 0;
  for (const PrefillPass& pass : prefill_passes(start, len, nrows, cap)) {
    for (const PrefillSeg& s : pass) {
      if (n < capacity) {
        int32_t* q = out + 4 * (size_t)n;
        q[0] = pi, q[1] = s.src, q[2] = s.p0, q[3] = s.len;
      }
      ++n;
    }
    ++pi;
  }
  return n;
}

// Tuning hook: the continuous-batching scheduler (serve_plan.hpp) run on
// explicit requests without a device, so a test reads the row decisions
// llm_decoder_serve_step executes.  All n requests (prompt_lens[i], max_new[i];
// ids 0 .. n-1) are submitted before step 1; request i ends after gen_lens[i]
// tokens (1 .. max_new[i]).  Steps count from 1 and stop when nothing is live
// or waiting.  out: int64 records (step, kind, id, row, aux), the first `room`
// of them, in the order a serve step produces them:
//   kind 0 admit   row = the row taken, aux = pages committed after it
//   kind 1 token   row = the row held during the step, aux = generated index
//   kind 2 move    row = the destination row, aux = the source row
//   kind 3 retire  row = the row given up, aux = 1 (ended before max_new, as
//                  an EOS would) or 2 (max_new tokens delivered)
// Returns the record count, -1 if a request is refused (T > max_seq_len or a
// need above num_pages), -(count) if `room` is too small (out then holds the
// first `room` records), INT_MIN on bad arguments.
extern "C" int serve_plan_sim_tune(const int32_t* prompt_lens, const int32_t* max_new,
                                   const int32_t* gen_lens, int n, int max_rows,
                                   long long num_pages, int pages_per_tile, int page_size,
                                   int window, int max_seq_len, long long* out, int room) {
  constexpr int kBad = -2147483647 - 1;
  if (n < 0 || max_rows < 1 || num_pages < 1 || pages_per_tile < 1 || page_size < 1 ||
      window < 0 || max_seq_len < 1 || room < 0 || (room && !out) ||
      (n && (!prompt_lens || !max_new || !gen_lens)))
    return kBad;
  for (int i = 0; i < n; ++i)
    if (prompt_lens[i] < 1 || max_new[i] < 1 || gen_lens[i] < 1 || gen_lens[i] > max_new[i])
      return kBad;
  ServeGeom g;
  g.max_rows = max_rows; g.num_pages = num_pages; g.pages_per_tile = pages_per_tile;
  g.page_size = page_size; g.window = window; g.max_seq_len = max_seq_len;
  ServePlan plan;
  plan.begin(g);
  for (int i = 0; i < n; ++i)
    if (plan.submit(prompt_lens[i], max_new[i]) != i) return -1;
  long long count = 0;
  auto rec = [&](long long step, long long kind, long long id, long long row, long long aux) {
    if (count < room) {
      long long* q = out + 5 * count;
      q[0] = step, q[1] = kind, q[2] = id, q[3] = row, q[4] = aux;
    }
    ++count;
  };
  for (long long step = 1; plan.live() + plan.waiting() > 0; ++step) {
    const int before = plan.live(), na = plan.admit();
    long long committed = plan.committed();
    for (int r = before + na - 1; r >= before; --r) committed -= plan.row(r).need;
    for (int r = before; r < before + na; ++r) {
      committed += plan.row(r).need;
      rec(step, 0, plan.row(r).id, r, committed);
    }
    if (plan.live() == 0) return kBad;  // (not reached: a lone request always fits)
    plan.finish_step(
        [&](int r, const ServeReq& q) {
          rec(step, 1, q.id, r, q.delivered);
          return q.delivered + 1 == gen_lens[q.id] && gen_lens[q.id] < q.max_new;
        },
        [&](int r, const ServeReq& q, int finish, const ServeMove* mv) {
          rec(step, 3, q.id, r, finish);
          if (mv) rec(step, 2, plan.row(mv->dst).id, mv->dst, mv->src);
          return 0;
        });
  }
  if (count > 2147483647LL) return kBad;
  return count > room ? -(int)count : (int)count;
}

// Tuning hook: serve_plan_sim_tune with prompts -- the scheduler with its
// prefix cache (prefix_cache != 0; serve_plan.hpp, prefix_cache.hpp) or without
// it.  tokens holds the n prompts' ids back to back (prompt_lens[i] each); no
// window.  out: int64 records (step, kind, id, row, aux, aux2), in the order a
// serve step produces them -- admissions (each with its evictions before it),
// the deferral, the publications, the state, tokens, retirements, the state:
//   kind 0 admit   aux = pages committed after it, aux2 = hit_blocks
//   kind 1 token, 2 move, 3 retire   as serve_plan_sim_tune, aux2 = 0
//   kind 4 defer   id = the head that the same-step rule kept waiting, row -1
//   kind 5 evict   id = the block, row -1, aux = its tile index, aux2 = 0
//   kind 6 publish id = the request, row = its row, aux = the block, aux2 = its
//                  tile index
//   kind 7 state after the step's admissions and publications, kind 8 state
//          after its retirements: id -1, row -1, aux = committed, aux2 =
//          idle_pages
// With the cache off the records of kinds 0 .. 3 are serve_plan_sim_tune's
// (aux2 = 0).  stats (may be NULL): positions due, positions hit, blocks
// cached at the end, idle_pages at the end, blocks evicted, deferrals.
// Returns as serve_plan_sim_tune does.
extern "C" int serve_prefix_sim_tune(const int32_t* tokens, const int32_t* prompt_lens,
                                     const int32_t* max_new, const int32_t* gen_lens, int n,
                                     int max_rows, long long num_pages, int pages_per_tile,
                                     int page_size, int max_seq_len, int prefix_cache,
                                     long long* out, int room, long long* stats) {
  constexpr int kBad = -2147483647 - 1;
  if (n < 0 || max_rows < 1 || num_pages < 1 || pages_per_tile < 1 || page_size < 1 ||
      max_seq_len < 1 || room < 0 || (room && !out) || (prefix_cache != 0 && prefix_cache != 1) ||
      (n && (!tokens || !prompt_lens || !max_new || !gen_lens)))
    return kBad;
  for (int i = 0; i < n; ++i)
    if (prompt_lens[i] < 1 || max_new[i] < 1 || gen_lens[i] < 1 || gen_lens[i] > max_new[i])
      return kBad;
  ServeGeom g;
  g.max_rows = max_rows; g.num_pages = num_pages; g.pages_per_tile = pages_per_tile;
  g.page_size = page_size; g.window = 0; g.max_seq_len = max_seq_len;
  ServePlan plan;
  plan.begin(g, prefix_cache != 0);
  {
    const int32_t* tok = tokens;
    for (int i = 0; i < n; ++i) {
      if (plan.submit(prompt_lens[i], max_new[i], tok) != i) return -1;
      tok += prompt_lens[i];
    }
  }
  long long count = 0;
  auto rec = [&](long long step, long long kind, long long id, long long row, long long aux,
                 long long aux2) {
    if (count < room) {
      long long* q = out + 6 * count;
      q[0] = step, q[1] = kind, q[2] = id, q[3] = row, q[4] = aux, q[5] = aux2;
    }
    ++count;
  };
  int32_t next_page = 0;  // stand-ins for the page ids a hold would report
  for (long long step = 1; plan.live() + plan.waiting() > 0; ++step) {
    const int before = plan.live(), na = plan.admit();
    // (the evictions of a step all precede its publications, so an evicted
    // block's id names what it named when it was published)
    for (const ServeEvict& e : plan.evictions()) rec(step, 5, e.block, -1, e.depth, 0);
    plan.evictions().clear();
    long long committed = plan.committed();
    for (int r = before + na - 1; r >= before; --r) committed -= plan.row(r).need;
    for (int r = before; r < before + na; ++r) {
      committed += plan.row(r).need;  // (cache off: as serve_plan_sim_tune counts it)
      rec(step, 0, plan.row(r).id, r, prefix_cache ? plan.row(r).committed_after : committed,
          plan.row(r).hit_blocks);
    }
    if (plan.deferred() >= 0) rec(step, 4, plan.deferred(), -1, 0, 0);
    if (plan.live() == 0) return kBad;  // (not reached: a lone request always fits)
    for (int r = before; r < before + na; ++r) {
      const size_t had = plan.row(r).blocks.size();
      plan.publish(r, [&](int, int32_t* pages) {
        for (int i = 0; i < pages_per_tile; ++i) pages[i] = next_page++;
        return 0;
      });
      for (size_t k = had; k < plan.row(r).blocks.size(); ++k)
        rec(step, 6, plan.row(r).id, r, plan.row(r).blocks[k], (long long)k);
    }
    rec(step, 7, -1, -1, plan.committed(), plan.idle_pages());
    plan.finish_step(
        [&](int r, const ServeReq& q) {
          rec(step, 1, q.id, r, q.delivered, 0);
          return q.delivered + 1 == gen_lens[q.id] && gen_lens[q.id] < q.max_new;
        },
        [&](int r, const ServeReq& q, int finish, const ServeMove* mv) {
          rec(step, 3, q.id, r, finish, 0);
          if (mv) rec(step, 2, plan.row(mv->dst).id, mv->dst, mv->src, 0);
          return 0;
        });
    rec(step, 8, -1, -1, plan.committed(), plan.idle_pages());
  }
  if (stats) {
    const ServePrefixStats& s = plan.prefix_stats();
    stats[0] = s.due, stats[1] = s.hit, stats[2] = plan.index().cached_blocks();
    stats[3] = plan.idle_pages(), stats[4] = s.evicted, stats[5] = s.deferrals;
  }
  if (count > 2147483647LL) return kBad;
  return count > room ? -(int)count : (int)count;
}

// Tuning hook: the beam search's host bookkeeping (beam_plan.hpp) run on
// explicit candidates without a device, as llm_decoder_beam_search runs it on
// the device's: cand_* [steps][num_seqs][2W] in rank order, min(max_new,
// steps) steps or until every sequence is done.  out_ids [num_seqs][W]
// [max_new], out_len / out_sum_logprob / out_score [num_seqs][W], live_parent
// / live_token [steps][num_seqs][W] (the steps run are written), *steps_run.
// Returns LLM_OK, LLM_ERR_INVALID on bad arguments, or the search's
// LLM_ERR_HIP with its text when the candidates are refused.
extern "C" int beam_book_tune(const float* cand_score, const int32_t* cand_parent,
                              const int32_t* cand_token, int steps, int num_seqs, int W, int V,
                              int max_new, int eos_token, float length_penalty, int32_t* out_ids,
                              int32_t* out_len, float* out_sum_logprob, float* out_score,
                              int32_t* live_parent, int32_t* live_token, int32_t* steps_run) {
  LLM_REQUIRE(cand_score && cand_parent && cand_token && out_ids && out_len && out_sum_logprob &&
                  out_score && live_parent && live_token && steps_run,
              "beam_book_tune: NULL");
  LLM_REQUIRE(W >= 1 && W <= 4 && V >= 2 * W, "beam_book_tune: W must be in [1, 4], V >= 2W");
  LLM_REQUIRE(steps >= 1 && num_seqs >= 1 && max_new >= 1 && eos_token >= -1 && eos_token < V &&
                  length_penalty >= 0.f && std::isfinite(length_penalty),
              "beam_book_tune: steps, num_seqs, max_new >= 1; eos_token -1 or a token id; "
              "length_penalty finite and >= 0");
  BeamPlan plan;
  plan.begin(num_seqs, W, max_new, eos_token, length_penalty, V);
  const int K = 2 * W;
  std::vector<float> score(W);
  *steps_run = 0;
  for (int st = 0; st < std::min(max_new, steps); ++st) {
    for (int s = 0; s < num_seqs; ++s) {
      const size_t c0 = ((size_t)st * num_seqs + s) * K, l0 = ((size_t)st * num_seqs + s) * W;
      if (const char* err = plan.step(s, cand_score + c0, cand_parent + c0, cand_token + c0,
                                      live_parent + l0, live_token + l0, score.data()))
        return fail(LLM_ERR_HIP, err);
    }
    *steps_run = st + 1;
    if (plan.all_done()) break;
  }
  plan.finish(out_ids, out_len, out_sum_logprob, out_score);
  return LLM_OK;
}

// Tuning hook: the fused o_proj's W_o head slices (oproj_slices.hpp) of one
// row-major fp16 [H*D][o_n] matrix, on the host, as llm_decoder_set_f16_weights
// builds them per layer: out [H][D/8][o_n][8].
extern "C" int oproj_head_slices_tune(const uint16_t* wo, int H, int D, int o_n, uint16_t* out) {
  LLM_REQUIRE(wo && out, "oproj_head_slices_tune: NULL");
  LLM_REQUIRE(H >= 1 && D >= 8 && D % 8 == 0 && o_n >= 1,
              "oproj_head_slices_tune: H, o_n >= 1, D a positive multiple of 8");
  oproj_head_slices(wo, H, D, o_n, out);
  return LLM_OK;
}

// Tuning hook: the three internal attention entries (pa_decode_internal,
// pa_prefill_internal, pa_prefill_packed_segs_internal) unchanged behind a
// plain-C struct, so tests reach what the decoder's layers get back -- the
// PaRowOutputs conversions of every launch form -- on shapes of their own
// (ctypes mirror: llm_capi.PaRowsTuneArgs; tests/test_pa_rows_gpu.py).
// No kernel code here.
struct PaRowsTuneArgs {
  int launch;  // 0 pa_decode_internal, 1 pa_prefill_internal, 2 the packed prefill
  const pa_kv_view* kv;
  const float* q;
  int q_stride;
  float sm_scale;
  int window;
  void* workspace;
  size_t workspace_bytes;
  // decode
  const int32_t* beam_ids;
  const int32_t* context_lens;
  int B, H, D, T, pages_per_split, row_group;
  int out_kind;  // PaOut: 0 F32, 1 ROW_Q, 2 ROW_F16, 3 F32_ROWS, 4 OPROJ
  // prefill: positions p0 .. p0 + m - 1 of page-table row `row`
  int row, p0, m;
  // packed prefill: the segment list (host); the workspace starts with
  // pa_prefill_packed_meta_bytes for the tile table and the contexts
  const pa_prefill_seg* segs;
  int nseg;
  // PaRowOutputs (has_rows 0: the entry gets rows = NULL) and the fp32 out
  int has_rows;
  int8_t* rows_q;
  float* inv_scale;
  void* out16;
  int pack, keep_out;
  float out_scale;
  float* out;
  int out_stride;  // prefill entries (0: H*D)
  // decode: the launch that ran (written before it runs; 0 / 0 if refused before the plan)
  int nsplit, form;
  // decode, out_kind OPROJ: PaRowOutputs' fused o_proj fields and PaRequest::rows16
  long long* o_acc;
  float* o_x;
  const void* wo_heads;
  int o_n;
  int* o_flag;
  int rows16;
};

extern "C" int pa_rows_tune(PaRowsTuneArgs* t, void* stream) {
  LLM_REQUIRE(t, "pa_rows_tune: NULL arguments");
  LLM_REQUIRE(t->launch >= 0 && t->launch <= 2, "pa_rows_tune: launch must be 0, 1 or 2");
  t->nsplit = t->form = 0;
  PaRowOutputs ro;
  ro.q = t->rows_q;
  ro.inv_scale = t->inv_scale;
  ro.out16 = t->out16;
  ro.pack = t->pack;
  ro.keep_out = t->keep_out;
  ro.out_scale = t->out_scale;
  const PaRowOutputs* rows = t->has_rows ? &ro : nullptr;
  hipStream_t st = as_stream(stream);
  if (t->launch == 1)
    return pa_prefill_internal(t->kv, t->q, t->q_stride, t->out, t->out_stride, t->row, t->p0,
                               t->m, t->sm_scale, t->workspace, t->workspace_bytes, st, rows,
                               t->window);
  if (t->launch == 2)
    return pa_prefill_packed_segs_internal(t->kv, t->q, t->q_stride, t->out, t->out_stride,
                                           t->segs, t->nseg, t->sm_scale, t->window, t->workspace,
                                           t->workspace_bytes, st, rows);
  LLM_REQUIRE(t->out_kind >= 0 && t->out_kind <= (int)PaOut::OPROJ,
              "pa_rows_tune: out_kind must be F32, ROW_Q, ROW_F16, F32_ROWS or OPROJ");
  LLM_REQUIRE(t->row_group >= 1 && t->row_group <= 4, "pa_rows_tune: row_group must be in [1, 4]");
  PaRequest rq = pa_request(t->kv, t->B, t->H, t->D, t->T, t->pages_per_split, t->row_group,
                            (PaOut)t->out_kind, t->window);
  rq.keep_out = t->keep_out != 0;
  if (rq.out == PaOut::OPROJ) {
    rq.rows16 = t->rows16 != 0;
    ro.o_acc = t->o_acc, ro.o_x = t->o_x, ro.wo_heads = t->wo_heads, ro.o_n = t->o_n;
    ro.o_flag = t->o_flag;
  }
  PaLaunch p;
  const int rc = pa_decode_internal(t->kv, rq, nullptr, t->q_stride, nullptr, nullptr, nullptr,
                                    1.f, nullptr, 0, nullptr, nullptr, &p);
  if (rc != LLM_OK) return rc;
  t->nsplit = p.nsplit;
  t->form = p.form();
  return pa_decode_internal(t->kv, rq, t->q, t->q_stride, t->out, t->beam_ids, t->context_lens,
                            t->sm_scale, t->workspace, t->workspace_bytes, st, rows);
}

// Tuning hook (not part of include/llm_decoder.h): run the split kernel of
// D=128 / TS=16 in a given variant so scripts/bench_kernels.py can compare
// register-stage sizes and cache policies in one process.
extern "C" int pa_decode_tune(int variant, const pa_kv_view* kv, const float* q, float* out,
                              const int32_t* context_lens, int B, int H, int T, int pps,
                              void* workspace, size_t workspace_bytes, void* stream) {
  LLM_REQUIRE(kv && (kv->head_dim == 128 || kv->head_dim == 64) && kv->page_size == 16 &&
                  H == kv->num_heads,
              "pa_decode_tune: D 128 (variants 0-19) or 64 (20-25), page 16 only");
  const int D = kv->head_dim;
  LLM_REQUIRE((D == 128) == (variant < 20), "pa_decode_tune: variant / head_dim mismatch");
  const int ntiles_max = std::max(1, (T + 15) / 16);
  pps = std::min(std::max(pps, 1), kMaxPps);
  const int nsplit = (ntiles_max + pps - 1) / pps;
  LLM_REQUIRE(nsplit > 1 && nsplit <= kMaxSplits, "pa_decode_tune: needs 2..128 splits");
  const size_t need = (size_t)B * H * nsplit * (D + 2) * sizeof(float);
  LLM_REQUIRE(workspace && workspace_bytes >= need, "pa_decode_tune: workspace");
  PaSplitArgs a{};
  a.k_pool = static_cast<const uint8_t*>(kv->k_pool);
  a.v_pool = static_cast<const uint8_t*>(kv->v_pool);
  a.page_table = kv->page_table;
  a.q = q; a.q_stride = H * D; a.out = out;
  a.context_lens = context_lens;
  a.B = B; a.H = H; a.T = T;
  a.num_pages = kv->num_pages; a.num_beams = kv->num_beams; a.max_tiles = kv->max_tiles;
  a.page_stride = kv_view_page_stride(*kv);
  a.pps = pps; a.nsplit = nsplit; a.group = 1; a.qscale = kLog2e;
  a.part_acc = static_cast<float*>(workspace);
  a.part_ml = a.part_acc + (size_t)B * H * nsplit * D;
  hipStream_t st = as_stream(stream);
  const dim3 grid((B * H * nsplit + 3) / 4), block(256);
  switch (variant) {  // NOLINT
    case 0: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.aux = 0}>), grid, block, 0, st, a); break;
    case 1: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{}>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.chunk_bytes = 8192, .aux = 0}>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.chunk_bytes = 8192}>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.chunk_bytes = 32768, .aux = 0}>), grid, block, 0, st, a); break;
    case 5: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.chunk_bytes = 32768}>), grid, block, 0, st, a); break;
    case 6: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.chunk_bytes = 8192, .stages = 1, .min_waves = 8}>), grid, block, 0, st, a); break;
    case 7: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.stages = 1, .min_waves = 4}>), grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.chunk_bytes = 8192, .min_waves = 4}>), grid, block, 0, st, a); break;
    case 9: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.chunk_bytes = 8192, .stages = 1, .min_waves = 6}>), grid, block, 0, st, a); break;
    case 10: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.load_only = true}>), grid, block, 0, st, a); break;
    case 11: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.chunk_bytes = 8192, .stages = 1, .min_waves = 8, .load_only = true}>), grid, block, 0, st, a); break;
    case 12: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.chunk_bytes = 32768, .load_only = true}>), grid, block, 0, st, a); break;
    // 13: variant 1 without the full-page fast path (every token takes the validity selects)
    case 13: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.fullpath = false}>), grid, block, 0, st, a); break;
    // 14-18: variant 1 with other cache-policy bits of the KV loads (gfx940-family
    // CPol: sc0 = 1, nt = 2, sc1 = 16): 14 sc0|nt, 15 sc1|nt, 16 sc0|sc1|nt,
    // 17 sc1, 18 sc0; 19: loads only with sc1|nt
    case 14: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.aux = 3}>), grid, block, 0, st, a); break;
    case 15: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.aux = 18}>), grid, block, 0, st, a); break;
    case 16: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.aux = 19}>), grid, block, 0, st, a); break;
    case 17: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.aux = 16}>), grid, block, 0, st, a); break;
    case 18: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.aux = 1}>), grid, block, 0, st, a); break;
    case 19: hipLaunchKernelGGL((pa_split_kernel<128, 16, PaSplitCfg{.aux = 18, .load_only = true}>), grid, block, 0, st, a); break;
    // D = 64 (C2): 20 production, 21 one 16 KiB stage, 22 8 KiB stages, 23 one
    // 32 KiB stage, 24 / 25 loads only (16 KiB x 2, 32 KiB x 1)
    case 20: hipLaunchKernelGGL((pa_split_kernel<64, 16, PaSplitCfg{}>), grid, block, 0, st, a); break;
    case 21: hipLaunchKernelGGL((pa_split_kernel<64, 16, PaSplitCfg{.stages = 1}>), grid, block, 0, st, a); break;
    case 22: hipLaunchKernelGGL((pa_split_kernel<64, 16, PaSplitCfg{.chunk_bytes = 8192}>), grid, block, 0, st, a); break;
    case 23: hipLaunchKernelGGL((pa_split_kernel<64, 16, PaSplitCfg{.chunk_bytes = 32768, .stages = 1}>), grid, block, 0, st, a); break;
    case 24: hipLaunchKernelGGL((pa_split_kernel<64, 16, PaSplitCfg{.load_only = true}>), grid, block, 0, st, a); break;
    case 25: hipLaunchKernelGGL((pa_split_kernel<64, 16, PaSplitCfg{.chunk_bytes = 32768, .stages = 1, .load_only = true}>), grid, block, 0, st, a); break;
    default: return fail(LLM_ERR_INVALID, "pa_decode_tune: variant");
  }
  LLM_HIP_RET(hipGetLastError());
  return pa_merge_splits_internal(a.part_acc, a.part_ml, out, context_lens, B, H, D, T, 16, pps,
                                  nsplit, kv->max_tiles, st);
}
