// Paged decode attention for gfx950 (CDNA4): the split merges, the launch of a
// plan (pa_decode_internal: validate, plan, fill PaSplitArgs, launch, merge)
// and the C entry points (pa_decode, pa_decode_grouped, pa_decode_plan).  The
// plan itself (split counts, forms) is pa_plan.hpp's, host-only; the split
// kernel, its named forms and the design notes of the scan are in
// pa_split.hpp; the tuning build's experiment kernels and A/B entries are in
// csrc/tune/pa_decode_tune.hip.
#include "pa_split.hpp"

namespace llm {

// Split merge fused with the next consumer's input conversion: one workgroup
// per row b merges all H heads into an LDS row [H*D], then writes any of
//   out   fp32 [B][H*D]            (pa_decode's output)
//   q     int8 [B][H*D] + inv_scale[b]   (per-row quantisation of the o_proj
//         input, int8_quant.cpp:5-13,59-64 — replaces a quantize_rows launch)
//   out16 fp16 [B][H*D]            (fp16 o_proj input of the FP16 decoder)
struct PaMergeRowArgs {
  const float* part_acc;
  const float* part_ml;
  float* out;
  int8_t* q;
  float* inv_scale;
  _Float16* out16;
  const int32_t* context_lens;
  int B, H, D, T, TS, pps, nsplit, max_tiles;
  int pack;  // q / out16 in packed-A order (common.hpp a_frag_off_*)
  int ctx_p0;  // >= 0 and context_lens NULL: row b's context is ctx_p0 + b + 1 (prefill)
  float out_scale;  // multiplies every merged head (LLM_FP8 pools: the V scale; else 1)
  int window;  // the split launch's (PaSplitArgs::window): splits relative to the row's window
};

// One head's split merge (flash-decoding LSE combine) by one wave, DPL =
// output dims per lane (D / 64, at least 1).  The head's split weights (m, l),
// lane-parallel (lane holds splits lane and 64 + lane), and the partials of
// its first BATCH splits are loaded together: every address depends on the
// launch's arguments only (clamped to its nsplit), so they issue with the
// caller's context_lens load and a merge costs one memory round trip (splits
// beyond the batch: one more per 8).  The row's split count ns masks the
// values afterwards (splits past ns may hold stale bits).  Summation order
// s = 0, 1, ... (sequential) for L and for every output; split s's (l, w) come
// from lane s by readlane.  acc[j] * the returned 1 / L is the output at dim
// lane + 64 j; a head with no partial returns acc = 0.
template <int DPL, int BATCH>
__device__ __forceinline__ float merge_head(const float* ml, const float* pa, int nsplit, int ns,
                                            int D, float (&acc)[DPL]) {
  const int lane = lane_id();
  const int nsl = max(nsplit - 1, 0);
  const float m0r = ml[2 * min(lane, nsl)], l0r = ml[2 * min(lane, nsl) + 1];
  const float m1r = ml[2 * min(64 + lane, nsl)], l1r = ml[2 * min(64 + lane, nsl) + 1];
  float v[BATCH][DPL];
#pragma unroll
  for (int s2 = 0; s2 < BATCH; ++s2)
#pragma unroll
    for (int j = 0; j < DPL; ++j)
      v[s2][j] = pa[(size_t)min(s2, nsl) * D + min(lane + 64 * j, D - 1)];
  const float m0 = lane < ns ? m0r : kNegSentinel;
  const float m1 = 64 + lane < ns ? m1r : kNegSentinel;
  const float l0 = lane < ns ? l0r : 0.f;
  const float l1 = 64 + lane < ns ? l1r : 0.f;
#pragma unroll
  for (int s2 = 0; s2 < BATCH; ++s2)
#pragma unroll
    for (int j = 0; j < DPL; ++j) v[s2][j] = s2 < ns ? v[s2][j] : 0.f;
#pragma unroll
  for (int j = 0; j < DPL; ++j) acc[j] = 0.f;
  const float M = ln_wave_max(fmaxf(m0, m1));
  if (ns <= 0 || M <= 0.5f * kNegSentinel) return 0.f;
  const float w0 = lane < ns ? __builtin_amdgcn_exp2f(m0 - M) : 0.f;
  const float w1 = 64 + lane < ns ? __builtin_amdgcn_exp2f(m1 - M) : 0.f;
  float L = 0.f;
#pragma unroll
  for (int s2 = 0; s2 < BATCH; ++s2)
    if (s2 < ns) {
      const float ls = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(l0), s2));
      const float ws = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w0), s2));
      L += ls * ws;
    }
  for (int s2 = BATCH; s2 < ns; ++s2) {
    const float ls = s2 < 64 ? __shfl(l0, s2, 64) : __shfl(l1, s2 - 64, 64);
    const float ws = s2 < 64 ? __shfl(w0, s2, 64) : __shfl(w1, s2 - 64, 64);
    L += ls * ws;
  }
#pragma unroll
  for (int s2 = 0; s2 < BATCH; ++s2) {
    const float ws = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w0), s2));  // 0 past ns
#pragma unroll
    for (int j = 0; j < DPL; ++j) acc[j] += v[s2][j] * ws;
  }
  for (int s0 = BATCH; s0 < ns; s0 += 8) {  // long split lists
#pragma unroll
    for (int j = 0; j < DPL; ++j) {
      const int d = lane + 64 * j;
      float u[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) u[k] = (s0 + k < ns && d < D) ? pa[(size_t)(s0 + k) * D + d] : 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int s2 = s0 + k;
        if (s2 < ns) {
          const float ws = s2 < 64 ? __shfl(w0, s2, 64) : __shfl(w1, s2 - 64, 64);
          acc[j] += u[k] * ws;
        }
      }
    }
  }
  return 1.0f / (L + 1e-6f);
}

// Split merge, fp32 output: one wave per (b, h), 4 per workgroup.  The first
// 16 splits' partials come in the first round trip (the 8-row C3 step merges
// 16 splits per head: 8.0 us per launch when the (m, l) and partial loads
// were issued split by split).
struct PaMergeArgs {
  const float* part_acc;
  const float* part_ml;
  float* out;
  const int32_t* context_lens;
  int B, H, D, T, TS, pps, nsplit, max_tiles;
  float out_scale;  // multiplies every merged head (LLM_FP8 pools: the V scale; else 1)
  int window;  // the split launch's (PaSplitArgs::window): splits relative to the row's window
};

template <int DPL>
__global__ __launch_bounds__(256) void pa_merge_kernel(PaMergeArgs a) {
  const int lane = lane_id();
  const int bh = blockIdx.x * 4 + wave_id_uniform();
  if (bh >= a.B * a.H) return;
  const int b = bh / a.H;
  int Tb = a.context_lens ? a.context_lens[b] : a.T;
  Tb = min(max(Tb, 0), a.T);
  const int ntiles = min((Tb + a.TS - 1) / a.TS, a.max_tiles);
  // pps < 0: every split holds a partial (beam launches: cost-balanced splits)
  const int ns = a.pps < 0 ? a.nsplit
                           : row_nsplits(a.pps, a.nsplit, row_span(Tb, ntiles, a.window, a.TS).n_live);
  float acc[DPL];
  const float inv = a.out_scale * merge_head<DPL, 16>(a.part_ml + (size_t)bh * a.nsplit * 2,
                                                      a.part_acc + (size_t)bh * a.nsplit * a.D,
                                                      a.nsplit, ns, a.D, acc);
  float* o = a.out + (size_t)bh * a.D;
#pragma unroll
  for (int j = 0; j < DPL; ++j) {
    const int d = lane + 64 * j;
    if (d < a.D) o[d] = acc[j] * inv;
  }
}

// Splits per first round trip of pa_merge_row_kernel's heads.
constexpr int kMergeBatch = 8;

template <int DPL>
__global__ __launch_bounds__(1024) void pa_merge_row_kernel(PaMergeRowArgs a) {
  extern __shared__ float row[];  // [H*D]
  __shared__ float sh[16];
  const int lane = lane_id();
  const int w = wave_id_uniform();
  const int nw = blockDim.x >> 6;
  const int b = blockIdx.x;
  const int hid = a.H * a.D;
  int Tb = a.context_lens ? a.context_lens[b] : a.ctx_p0 >= 0 ? a.ctx_p0 + b + 1 : a.T;
  Tb = min(max(Tb, 0), a.T);
  const int ntiles = min((Tb + a.TS - 1) / a.TS, a.max_tiles);
  // pps < 0: every split holds a partial (beam launches: cost-balanced splits)
  const int ns = a.pps < 0 ? a.nsplit
                           : row_nsplits(a.pps, a.nsplit, row_span(Tb, ntiles, a.window, a.TS).n_live);
  for (int h = w; h < a.H; h += nw) {
    const size_t bh = (size_t)b * a.H + h;
    float acc[DPL];
    const float inv = a.out_scale * merge_head<DPL, kMergeBatch>(a.part_ml + bh * a.nsplit * 2,
                                                                 a.part_acc + bh * a.nsplit * a.D,
                                                                 a.nsplit, ns, a.D, acc);
    float* dst = row + h * a.D;
#pragma unroll
    for (int j = 0; j < DPL; ++j) {
      const int d = lane + 64 * j;
      if (d < a.D) dst[d] = acc[j] * inv;
    }
  }
  __syncthreads();
  float am = 0.f;
  // packed int8 o_proj input only (the decode step): 4 values per thread, one
  // dword store each (4 consecutive k are 4 consecutive bytes of a fragment)
  const bool quad = a.q && a.pack && !a.out && !a.out16 && hid % 64 == 0;
  if (quad) {
    for (int i4 = threadIdx.x; i4 < hid / 4; i4 += blockDim.x) {
      const f32x4 v = reinterpret_cast<const f32x4*>(row)[i4];
      am = fmaxf(am, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    }
  } else {
    for (int i = threadIdx.x; i < hid; i += blockDim.x) {
      const float v = row[i];
      am = fmaxf(am, fabsf(v));
      if (a.out) a.out[(size_t)b * hid + i] = v;
      if (a.out16)
        a.out16[a.pack ? a_frag_off_f16(b, i, hid >> 5) : (size_t)b * hid + i] = (_Float16)v;
    }
  }
  if (!a.q) return;
  am = ln_wave_max(am);  // DPP (wave_max shuffles through LDS)
  if (lane == 0) sh[w] = am;
  __syncthreads();
  am = sh[0];
  for (int i = 1; i < nw; ++i) am = fmaxf(am, sh[i]);
  const float scale = 127.f / (am + 1e-6f);
  if (quad) {
    for (int i4 = threadIdx.x; i4 < hid / 4; i4 += blockDim.x)
      *reinterpret_cast<uint32_t*>(a.q + a_frag_off_i8(b, 4 * i4, hid >> 6)) =
          ln_quant4(reinterpret_cast<const f32x4*>(row)[i4], scale);
  } else {
    for (int i = threadIdx.x; i < hid; i += blockDim.x) {
      float y = roundf(__fmul_rn(row[i], scale));
      y = fminf(fmaxf(y, -128.f), 127.f);
      a.q[a.pack ? a_frag_off_i8(b, i, hid >> 6) : (size_t)b * hid + i] = (int8_t)(int)y;
    }
  }
  if (threadIdx.x == 0) a.inv_scale[b] = 1.0f / scale;
}

namespace {

// Resident waves of the whole chip for a 256-thread kernel (its occupancy x
// the CU count); 0 where the query fails.  occupancy(&blocks) -> hipError_t.
template <class Q>
long long chip_waves(Q&& occupancy) {
  int dev = 0, cus = 0, blocks = 0;
  if (hipGetDevice(&dev) == hipSuccess &&
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
      occupancy(&blocks) == hipSuccess && cus > 0 && blocks > 0)
    return (long long)cus * blocks * 4;
  (void)hipGetLastError();
  return 0;
}

// ... of the plain split kernel of one shape, cached (kFallbackResident
// without a device), and of the beam-group form (0 where the plain schedule
// runs instead: pages above 8 KiB).
template <int D, int TS, int KVT>
long long resident_waves() {
  static long long cached = 0;
  if (cached) return cached;
  cached = chip_waves([](int* blocks) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(
        blocks, pa_split_kernel<D, TS, pa_cfg_split(D, TS, KVT)>, 256, 0);
  });
  if (!cached) cached = kFallbackResident;
  return cached;
}

template <int D, int TS>
long long beam_resident_waves() {
  if constexpr (split_stages(D, TS, 2) != 2) {
    return 0;
  } else {
    static long long cached = -1;
    if (cached >= 0) return cached;
    return cached = chip_waves([](int* blocks) {
      hipError_t e;
      if (tune_beam_occupancy(D, TS, blocks, &e)) return e;
      return hipOccupancyMaxActiveBlocksPerMultiprocessor(
          blocks, pa_split_kernel<D, TS, pa_cfg_beam()>, 256, 0);
    });
  }
}

}  // namespace


// The FP16 decoder's o_proj fused into the workgroup merge (decoder_step.cpp
// oproj_fusable); LLM_OPROJ_FUSE=0 (tuning build) restores the o_proj GEMM.
bool oproj_fuse_on() { return pa_tuning().oproj_fuse; }
bool beam_steal_on() { return pa_tuning().beam_steal; }

namespace {

// The experiment forms of beam-group launches (pa_beam4_kernel,
// pa_beam_mfma_kernel, the steal form, ...) exist only in the tuning build
// (csrc/tune/pa_decode_tune.hip, switched by pa_tuning.hpp).  All measured
// slower than the LDS-staged BEAM form of pa_split_kernel (C4 launch with
// merge: beam4 69.2 us at 16 splits, 74.2 with two pages per register stage,
// 82.3 at 12 splits, against 67.6 us; MFMA 69.8 vs 60.8 us; steal 76-92 vs
// 65.3 us).

template <int D, int TS, PaSplitCfg C>
hipError_t launch_form(const PaSplitArgs& a, dim3 grid, dim3 block, hipStream_t st) {
  hipLaunchKernelGGL((pa_split_kernel<D, TS, C>), grid, block, 0, st, a);
  return hipGetLastError();
}

// The split launch of a plan, in the form the plan names.
template <int D, int TS, int KVT>
hipError_t launch_split(const PaSplitArgs& a, const PaLaunch& p, hipStream_t st) {
  const int waves = ((a.B + a.group - 1) / a.group) * a.group * a.H * a.nsplit;
  const dim3 grid((waves + 3) / 4), block(256);
  if (p.wgm) {  // one workgroup per (b, h), one wave per split (2..8)
    const dim3 wgrid(a.B * a.H), wblock(64 * a.nsplit);
    if constexpr (KVT == LLM_F16) {
      if constexpr (D <= kOprojMaxD) {
        if (p.oproj) return launch_form<D, TS, pa_cfg_wgm_oproj(D, TS)>(a, wgrid, wblock, st);
      }
      return launch_form<D, TS, pa_cfg_wgm(D, TS)>(a, wgrid, wblock, st);
    } else if constexpr (KVT == LLM_FP8 && fp8_wgm_shape_ok(D, TS)) {
      // the decoder's own forms: the workgroup merge as well (no fused o_proj:
      // the planner keeps o_proj and fp16 rows to fp16 pools)
      return launch_form<D, TS, pa_cfg_wgm_fp8(D, TS)>(a, wgrid, wblock, st);
    } else {
      return hipErrorInvalidValue;  // (no plan: other pools keep split + merge)
    }
  }
  // other KV element types than fp16: the standard schedule (no beam-prefetch form)
  if constexpr (KVT == LLM_F16) {
    if (p.beam) {
      hipError_t te;
      if (tune_launch_form(a, D, TS, grid, st, &te)) return te;  // tuning build: an experiment form
      return launch_form<D, TS, pa_cfg_beam()>(a, grid, block, st);
    }
  }
  if (p.direct) return launch_form<D, TS, pa_cfg_split(D, TS, KVT, true)>(a, grid, block, st);
  return launch_form<D, TS, pa_cfg_split(D, TS, KVT)>(a, grid, block, st);
}

bool supported(int D, int TS, int kvt) {
  return pa_for_shape(D, TS, kvt, false, [](auto, auto, auto) { return true; });
}

}  // namespace

int pa_plan_device(const PaRequest& rq, PaLaunch* launch, long long resident,
                   long long beam_resident, long long beam4_resident) {
  *launch = PaLaunch{};
  const int D = rq.D, TS = rq.TS;
  if (!supported(D, TS, rq.kv_dtype)) return LLM_ERR_UNSUPPORTED;
  const PaTuning tn = pa_tuning();
  const bool beam_group = rq.row_group == 4 && rq.kv_dtype == LLM_F16;
  if (rq.pps_fixed > 0) {  // fixed splits are sized without the chip
    resident = beam_resident = beam4_resident = 0;
  } else {
    if (resident < 0)
      resident = pa_for_shape(D, TS, rq.kv_dtype, kFallbackResident, [](auto d, auto ts, auto k) {
        return resident_waves<decltype(d)::value, decltype(ts)::value, decltype(k)::value>();
      });
    if (beam_resident < 0)
      beam_resident = !beam_group ? 0 : pa_for_shape(D, TS, LLM_F16, 0LL, [](auto d, auto ts, auto) {
        return beam_resident_waves<decltype(d)::value, decltype(ts)::value>();
      });
    if (beam4_resident < 0)
      beam4_resident = beam_group && tn.beam4 && !tn.beam_mfma && split_stages(D, TS, 2) == 2
                           ? tune_beam4_resident_for(D, TS) : 0;
  }
  return pa_plan(rq, tn, resident, beam_resident, beam4_resident, launch);
}

int pa_pages_per_split(int B, int H, int T, int TS, int max_tiles) {
  const int ntiles = std::max(1, std::min((T + TS - 1) / TS, max_tiles));
  const int ns = choose_nsplit(B, H, ntiles, 0, kFallbackResident);
  return (ntiles + ns - 1) / ns;
}


}  // namespace llm

using namespace llm;

extern "C" int pa_decode_pages_per_split(int B, int H, int T, int page_size, int max_tiles) {
  if (B < 0 || H <= 0 || T < 0 || page_size <= 0 || max_tiles <= 0) return -1;
  return pa_pages_per_split(B, H, T, page_size, max_tiles);
}

extern "C" size_t pa_decode_workspace_bytes(int B, int H, int D, int max_tiles,
                                            int pages_per_split) {
  if (B <= 0 || H <= 0 || D <= 0 || max_tiles <= 0) return 0;
  const size_t nsplit = pages_per_split > 0
                            ? (size_t)choose_nsplit(B, H, max_tiles, pages_per_split, 0)
                            : (size_t)max_nsplit(B, H, max_tiles);
  return (size_t)B * H * nsplit * (size_t)(D + 2) * sizeof(float);
}

int llm::pa_merge_splits_internal(const float* part_acc, const float* part_ml, float* out,
                                  const int32_t* context_lens, int B, int H, int D, int T, int TS,
                                  int pps, int nsplit, int max_tiles, hipStream_t st,
                                  float out_scale, int window) {
  PaMergeArgs mg{part_acc, part_ml, out, context_lens, B, H, D, T, TS, pps, nsplit, max_tiles,
                 out_scale, window};
  const dim3 grid((B * H + 3) / 4);
  if (D <= 64)
    hipLaunchKernelGGL(pa_merge_kernel<1>, grid, dim3(256), 0, st, mg);
  else if (D <= 128)
    hipLaunchKernelGGL(pa_merge_kernel<2>, grid, dim3(256), 0, st, mg);
  else
    hipLaunchKernelGGL(pa_merge_kernel<4>, grid, dim3(256), 0, st, mg);
  LLM_HIP_RET(hipGetLastError());
  return LLM_OK;
}

int llm::pa_merge_rows_internal(const float* part_acc, const float* part_ml, float* out,
                                const PaRowOutputs* rows, const int32_t* context_lens, int ctx_p0,
                                int B, int H, int D, int T, int TS, int pps, int nsplit,
                                int max_tiles, hipStream_t st, float out_scale, int window) {
  PaMergeRowArgs mg{part_acc, part_ml, out, rows ? rows->q : nullptr,
                    rows ? rows->inv_scale : nullptr,
                    rows ? static_cast<_Float16*>(rows->out16) : nullptr, context_lens, B, H, D, T,
                    TS, pps, nsplit, max_tiles, rows ? rows->pack : 0, ctx_p0, out_scale, window};
  const int threads = 64 * std::min(16, H);  // one wave per head (heads > 16 loop)
  const size_t lds = (size_t)H * D * sizeof(float);
  if (D <= 64)
    hipLaunchKernelGGL(pa_merge_row_kernel<1>, dim3(B), dim3(threads), lds, st, mg);
  else if (D <= 128)
    hipLaunchKernelGGL(pa_merge_row_kernel<2>, dim3(B), dim3(threads), lds, st, mg);
  else
    hipLaunchKernelGGL(pa_merge_row_kernel<4>, dim3(B), dim3(threads), lds, st, mg);
  LLM_HIP_RET(hipGetLastError());
  return LLM_OK;
}

int llm::pa_decode_internal(const pa_kv_view* kv, const PaRequest& rq, const float* q, int q_stride,
                            float* out, const int32_t* beam_ids, const int32_t* context_lens,
                            float sm_scale, void* workspace, size_t workspace_bytes,
                            hipStream_t st, const PaRowOutputs* rows, PaLaunch* plan) {
  const int B = rq.B, H = rq.H, D = rq.D, T = rq.T;
  LLM_REQUIRE(kv != nullptr, "pa_decode: kv view is NULL");
  LLM_REQUIRE(B >= 0 && H > 0 && D > 0 && T >= 0, "pa_decode: bad B/H/D/T");
  LLM_REQUIRE(rq.window >= 0, "pa_decode: window must be >= 0 (0: off)");
  if (rq.window > 0 && rq.row_group > 1)
    return fail(LLM_ERR_UNSUPPORTED, "pa_decode: a sliding window needs ungrouped rows "
                                     "(row_group 1)");
  if (plan) *plan = PaLaunch{};
  if (B == 0) return LLM_OK;
  // the FP16 decoder's fused o_proj (PaRowOutputs::o_acc): workgroup-merge launches only
  const bool oproj = rq.out == PaOut::OPROJ, f32_rows = rq.out == PaOut::F32_ROWS;
  const bool out16 = rq.out == PaOut::ROW_F16 || (oproj && rq.rows16);
  const bool row_out = rq.out == PaOut::ROW_Q || out16;
  LLM_REQUIRE(plan || (q != nullptr && (out != nullptr || row_out || oproj)), "pa_decode: q/out NULL");
  LLM_REQUIRE(plan || rq.out == PaOut::F32 || f32_rows || rows, "pa_decode: row outputs need PaRowOutputs");
  LLM_REQUIRE(!oproj || (D <= kOprojMaxD && H <= 64 &&
                         (plan || (rows->o_acc && rows->wo_heads && rows->o_x && rows->o_flag &&
                                   rows->o_n > 0))),
              "pa_decode: fused o_proj needs W_o head slices, an output, a range flag, o_n > 0, "
              "head_dim <= 128 and at most 64 heads");
  LLM_REQUIRE(plan || rq.out != PaOut::ROW_Q || (rows->q && rows->inv_scale),
              "pa_decode: row quantisation needs q and inv_scale");
  LLM_REQUIRE(plan || !out16 || rows->out16, "pa_decode: fp16 rows need out16");
  LLM_REQUIRE(!row_out || (size_t)H * D * 4 <= 65536, "pa_decode: row outputs need H*D <= 16384");
  LLM_REQUIRE(!rows || !rows->pack || (H * D) % 64 == 0, "pa_decode: packed row outputs need H*D % 64 == 0");
  LLM_REQUIRE(kv->k_pool && kv->v_pool && kv->page_table, "pa_decode: kv pointers NULL");
  LLM_REQUIRE(kv_elem_size(kv->kv_dtype) > 0,
              "pa_decode: kv_dtype must be LLM_F16, LLM_BF16, LLM_F32, LLM_I8 or LLM_FP8");
  LLM_REQUIRE(kv->num_heads == H, "pa_decode: H != kv->num_heads");
  LLM_REQUIRE(kv->head_dim == D, "pa_decode: D != kv->head_dim");
  LLM_REQUIRE(kv->num_pages > 0 && kv->num_beams > 0 && kv->max_tiles > 0,
              "pa_decode: empty kv view");
  LLM_REQUIRE(rq.TS == kv->page_size && rq.max_tiles == kv->max_tiles && rq.kv_dtype == kv->kv_dtype,
              "pa_decode: the request is not of this kv view (pa_request)");
  if (!supported(D, kv->page_size, kv->kv_dtype))
    return fail(LLM_ERR_UNSUPPORTED, "pa_decode: unsupported head_dim/page_size/kv_dtype (D in "
                                     "{32,64,128,256}, page_size in {16,32}, one page of "
                                     "1..16 KiB)");
  const size_t page_stride = kv_view_page_stride(*kv);
  LLM_REQUIRE(page_stride >= (size_t)kv->page_size * D * kv_elem_size(kv->kv_dtype) &&
                  page_stride % 16 == 0,
              "pa_decode: page_stride must be 0 or >= one page and a multiple of 16");
  LLM_REQUIRE((long long)kv->num_pages * (long long)page_stride < (1LL << 47),
              "pa_decode: pool too large");
  const int TS = kv->page_size;
  PaLaunch p;
  if (pa_plan_device(rq, &p) != LLM_OK)
    return fail(LLM_ERR_UNSUPPORTED,
                "pa_decode: at most 128 splits of at most 128 pages per row (raise "
                "pages_per_split, or pass 0; T <= 16384 pages)");
  if (plan) return *plan = p, LLM_OK;
  LLM_REQUIRE(!p.direct || out != nullptr, "pa_decode: single-split launch needs the fp32 out");
  if (oproj && !p.oproj)
    return fail(LLM_ERR_UNSUPPORTED,
                "pa_decode: the fused o_proj needs the workgroup-merge form over fp16 pools");

  PaSplitArgs a{};
  a.k_pool = static_cast<const uint8_t*>(kv->k_pool);
  a.v_pool = static_cast<const uint8_t*>(kv->v_pool);
  a.page_table = kv->page_table;
  a.q = q, a.q_stride = q_stride, a.out = out;
  a.beam_ids = beam_ids, a.context_lens = context_lens;
  a.B = B, a.H = H, a.T = T;
  a.num_pages = kv->num_pages, a.num_beams = kv->num_beams, a.max_tiles = kv->max_tiles;
  a.page_stride = page_stride;
  a.pps = p.pps, a.nsplit = p.nsplit, a.group = std::max(1, std::min(rq.row_group, 4));
  a.qscale = sm_scale * kLog2e;
  const float out_scale = rows && kv->kv_dtype == LLM_FP8 ? rows->out_scale : 1.f;
  a.out_scale = out_scale;
  a.window = rq.window;
  if (!p.direct && !p.wgm) {  // (the workgroup merge keeps its splits' states in LDS)
    LLM_REQUIRE(workspace != nullptr && workspace_bytes >= p.workspace_bytes,
                "pa_decode: workspace too small (see pa_decode_workspace_bytes)");
    a.part_acc = static_cast<float*>(workspace);
    a.part_ml = a.part_acc + (size_t)B * H * p.nsplit * D;
  }
  const PaTuning tn = pa_tuning();
  a.balance16 = tn.beam_balance16;
  // beam-group workgroups in split-major order (PaSplitArgs::smaj).  Same box,
  // C4 (profiles/r06/c4_smaj_ab.txt): 12,719-12,737 against 12,604-12,617
  // tok/s; the launch's HBM bytes 1.031 -> 1.014x algorithmic
  // (profiles/pmc_attention_c4.json), the exits by dispatch slot unchanged
  a.smaj = a.group == 4 && tn.beam_smaj ? 1 : 0;
  a.beam4 = p.beam4 ? 1 : 0;
  if (p.steal && a.group == 4)  // the caller's counters, or the tuning build's (standalone launches)
    a.steal = rows && rows->beam_ctr ? rows->beam_ctr
                                     : tune_steal_counters(2 * (size_t)((B + 3) / 4) * H);
  if (p.wgm) {
    a.wgm = 1;
    a.out16 = rows ? static_cast<_Float16*>(rows->out16) : nullptr;
    a.pack = rows ? rows->pack : 0;
    a.out = f32_rows || (rows && rows->keep_out) ? out : nullptr;
    if (oproj) {
      a.o_acc = rows->o_acc, a.o_x = rows->o_x, a.o_n = rows->o_n, a.o_flag = rows->o_flag;
      a.wo_heads = static_cast<const _Float16*>(rows->wo_heads);
    }
  }
  const hipError_t e =
      pa_for_shape(D, TS, kv->kv_dtype, hipErrorInvalidValue, [&](auto d, auto ts, auto k) {
        return launch_split<decltype(d)::value, decltype(ts)::value, decltype(k)::value>(a, p, st);
      });
  if (e != hipSuccess) return fail(LLM_ERR_HIP, std::string("pa_split launch: ") + hipGetErrorString(e));
  if (p.wgm) return LLM_OK;
  // the beam kernel ran (p.beam): every split holds a partial
  if (row_out && !p.direct)
    return pa_merge_rows_internal(a.part_acc, a.part_ml, rows->keep_out ? out : nullptr, rows,
                                  context_lens, -1, B, H, D, T, TS, p.beam ? -1 : p.pps, p.nsplit,
                                  kv->max_tiles, st, out_scale, rq.window);
  if (!p.direct) {
    const int r = pa_merge_splits_internal(a.part_acc, a.part_ml, out, context_lens, B, H, D, T,
                                           TS, p.beam ? -1 : p.pps, p.nsplit, kv->max_tiles, st,
                                           out_scale, rq.window);
    if (r != LLM_OK) return r;
  }
  if (row_out) {  // single split: out is final; convert it in a row pass
    if (rows->q)
      LLM_HIP_RET(launch_quantize_rows(out, B, H * D, rows->q, rows->inv_scale, st, rows->pack));
    if (rows->out16)
      LLM_HIP_RET(launch_to_f16(out, (size_t)B * H * D, rows->out16, st, rows->pack ? H * D : 0));
  }
  return LLM_OK;
}

extern "C" int pa_decode_grouped(const pa_kv_view* kv, const float* q, float* out,
                                 const int32_t* beam_ids, const int32_t* context_lens, int B,
                                 int H, int D, int T, float sm_scale, int pages_per_split,
                                 int row_group, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  LLM_REQUIRE(row_group >= 1 && row_group <= 4, "pa_decode_grouped: row_group must be in [1, 4]");
  return pa_decode_internal(kv, pa_request(kv, B, H, D, T, pages_per_split, row_group), q, H * D,
                            out, beam_ids, context_lens, sm_scale, workspace, workspace_bytes,
                            as_stream(stream));
}

extern "C" int pa_decode_plan(const pa_kv_view* kv, int B, int H, int D, int T,
                              int pages_per_split, int row_group, int* nsplit, int* form) {
  LLM_REQUIRE(nsplit && form, "pa_decode_plan: NULL output");
  LLM_REQUIRE(row_group >= 1 && row_group <= 4, "pa_decode_plan: row_group must be in [1, 4]");
  PaLaunch p;
  const int rc = pa_decode_internal(kv, pa_request(kv, B, H, D, T, pages_per_split, row_group),
                                    nullptr, H * D, nullptr, nullptr, nullptr, 1.f, nullptr, 0,
                                    nullptr, nullptr, &p);
  *nsplit = p.nsplit;
  *form = p.form();
  return rc;
}

extern "C" int pa_decode(const pa_kv_view* kv, const float* q, float* out,
                         const int32_t* beam_ids, const int32_t* context_lens, int B, int H,
                         int D, int T, float sm_scale, int pages_per_split, void* workspace,
                         size_t workspace_bytes, void* stream) {
  return pa_decode_internal(kv, pa_request(kv, B, H, D, T, pages_per_split), q, H * D, out,
                            beam_ids, context_lens, sm_scale, workspace, workspace_bytes,
                            as_stream(stream));
}

extern "C" int pa_decode_window_plan(const pa_kv_view* kv, int B, int H, int D, int T,
                                     int pages_per_split, int window, int* nsplit, int* form) {
  LLM_REQUIRE(nsplit && form, "pa_decode_window_plan: NULL output");
  PaLaunch p;
  const int rc = pa_decode_internal(kv, pa_request(kv, B, H, D, T, pages_per_split, 1, PaOut::F32,
                                                   window),
                                    nullptr, H * D, nullptr, nullptr, nullptr, 1.f, nullptr, 0,
                                    nullptr, nullptr, &p);
  *nsplit = p.nsplit;
  *form = p.form();
  return rc;
}

extern "C" int pa_decode_window(const pa_kv_view* kv, const float* q, float* out,
                                const int32_t* beam_ids, const int32_t* context_lens, int B,
                                int H, int D, int T, float sm_scale, int pages_per_split,
                                int window, void* workspace, size_t workspace_bytes,
                                void* stream) {
  return pa_decode_internal(kv, pa_request(kv, B, H, D, T, pages_per_split, 1, PaOut::F32, window),
                            q, H * D, out, beam_ids, context_lens, sm_scale, workspace,
                            workspace_bytes, as_stream(stream));
}
