// Paged decode attention: the launch planner.  Host-only and pure (no HIP
// headers, no device calls): a PaRequest says what the caller wants, pa_plan
// turns it, the tuning table and the kernels' resident-wave counts into the
// PaLaunch that pa_decode_internal (pa_decode.hip) fills and launches, that
// pa_decode_plan reports and that the decoder's form predicates read.
#pragma once

#include <algorithm>

#include "llm_decoder.h"
#include "pa_tuning.hpp"

namespace llm {

constexpr int kWgmMaxSplits = 8;  // one merge batch (pa_merge_row_kernel's kMergeBatch)
constexpr int kOprojMaxD = 128;   // fused o_proj: two W_o column slices of D fp16 in VGPRs

constexpr int kMaxPps = 128;     // page ids held in two registers per lane
constexpr int kMaxSplits = 128;  // split weights held in two registers per merge lane
constexpr int kMinPps = 8;
constexpr int kMaxWavesPerCu = 32;  // 8 per SIMD x 4 SIMDs (gfx950)
// Resident waves assumed where the occupancy query fails: 256 CUs x 3 waves/SIMD.
constexpr long long kFallbackResident = 256LL * 4 * 3;

// Register stages of a split-kernel instantiation (es = bytes per KV element):
// pages above 8 KiB hold a whole stage per page already (two would not fit
// the VGPR file).
constexpr int split_stages(int D, int TS, int es) { return TS * D * es > 8192 ? 1 : 2; }

// LLM_FP8 pools merge in the workgroup for pages up to 2 KiB (64 or 128 dims x
// 16 tokens, 64 x 32: C3's and C5's shape among them).  Larger pages hold more
// decoded elements live per stage than the form's 512-thread bound (256 VGPRs)
// leaves room for -- 128 x 32 and 256 x 16 spill 76-80 bytes per lane, 256 x 32
// 224 -- so they keep split + merge.
constexpr bool fp8_wgm_shape_ok(int D, int TS) { return D * TS <= 2048; }

// What the caller wants back from the launch.
enum class PaOut {
  F32,       // fp32 [B][H][D] (pa_decode's output)
  ROW_Q,     // per-row int8 + inv_scale rows (the INT8 o_proj input)
  ROW_F16,   // fp16 rows (the FP16 o_proj input)
  F32_ROWS,  // fp32 rows for a consumer that quantises them itself
  OPROJ,     // the FP16 decoder's o_proj, fused into the workgroup merge
};

struct PaRequest {
  int B = 0, H = 0, D = 0, T = 0, TS = 0, max_tiles = 0;
  int kv_dtype = LLM_F16;
  int pps_fixed = 0;  // pages per split (> 0: fixed, clamped to kMaxPps; 0: chosen here)
  int row_group = 1;
  PaOut out = PaOut::F32;
  bool rows16 = false;    // OPROJ: the fp16 rows as well (the decoder's taps)
  bool steal_ctr = false;  // beam groups: the caller owns steal counters (PaRowOutputs::beam_ctr)
  bool keep_out = true;   // row outputs: a split launch writes the fp32 rows as well
  // sliding window: row b attends to its last `window` tokens only (0: off, the
  // whole context); ungrouped rows only
  int window = 0;
};

struct PaLaunch {
  int nsplit = 0;  // splits per (row, head)
  int pps = 0;     // the request's fixed pages per split, clamped (0: ceil(tiles / nsplit))
  bool direct = false, wgm = false, beam = false, beam4 = false, steal = false, oproj = false;
  bool steal_ctr = false;  // steal: the request's own counters (else the tuning build's)
  bool merge_row = false;  // split + merge forms: pa_merge_row_kernel (row outputs)
  size_t workspace_bytes = 0;  // split partials (none: direct and workgroup-merge launches)
  int form() const {  // LLM_PA_FORM_* (0 for no launch: nsplit 0)
    if (nsplit <= 0) return 0;
    return (direct ? LLM_PA_FORM_DIRECT : wgm ? LLM_PA_FORM_WG_MERGE
            : merge_row ? LLM_PA_FORM_SPLIT_MERGE_ROW : LLM_PA_FORM_SPLIT_MERGE) |
           (beam ? LLM_PA_FORM_BEAM : 0) | (oproj ? LLM_PA_FORM_OPROJ : 0) |
           (steal && steal_ctr ? LLM_PA_FORM_STEAL : 0);
  }
};

// Upper bound of the split count of any launch over rows of <= ntiles tiles
// (workspace sizing; host-only, no device query).
inline long long max_nsplit(int B, int H, int ntiles) {
  ntiles = std::max(ntiles, 1);
  const long long bh = std::max(1LL, (long long)B * H);
  const long long cap = 256LL * kMaxWavesPerCu;  // largest resident-wave count
  const long long lo = (ntiles + kMaxPps - 1) / kMaxPps;
  return std::min<long long>(
      kMaxSplits,
      std::max(lo, std::min<long long>((ntiles + kMinPps - 1) / kMinPps, lo + (cap + bh - 1) / bh + 1)));
}

// Splits per (b, h): the smallest NS that is a whole number of resident-wave
// rounds (B*H*NS ~ k * resident) with splits of <= kMaxPps pages, so every wave
// carries the same page count and the last round is not a ragged tail; never
// below kMinPps pages per split.  Small launches, where a full round would
// leave each wave under kShortPps pages, use fewer, longer splits instead,
// as long as at least kMinLaunchWaves waves remain: a split's fixed cost
// (page ids, q, its partial and its share of the merge) outweighs an idle
// part of the chip there.  Measured (scripts/sweep_attention_pps.py), round
// rule -> this rule: C2 (16 x 12 heads, 2048 tokens) 25.1 -> 21.3 us;
// 64 x 12 x 2048: 72.7 -> 66.6 us; 8 x 16 x 4096: 49.3 -> 46.1 us;
// 1 x 16 x 8192: 32.8 -> 26.4 us; 4 x 12 x 1024 unchanged (9.9 us).
constexpr int kShortPps = 32;
constexpr long long kMinLaunchWaves = 512;
// Workgroup-merge launches (PaSplitArgs::wgm) have no merge launch to feed, so
// their splits stay long: C2 (130 tiles) 3 splits, not 5.  Same-box C2 sweep
// (scripts/gpu_wgm_splits.sh, forced splits 2 / 3 / 4 / 5 / 6 / 8):
// 27.4-28.0k / 29.6-30.1k / 29.1-29.2k / 28.4k / 28.6-28.9k / 28.2-29.0k tok/s.
constexpr int kWgmShortPps = 64;
inline int choose_nsplit(int B, int H, int ntiles, int pps_fixed, long long resident,
                         int short_pps = kShortPps) {
  ntiles = std::max(ntiles, 1);
  if (pps_fixed > 0) {
    const int pps = std::min(pps_fixed, kMaxPps);
    return (ntiles + pps - 1) / pps;
  }
  const long long bh = std::max(1LL, (long long)B * H);
  const long long lo = (ntiles + kMaxPps - 1) / kMaxPps;
  long long ns = lo;
  for (long long k = 1; k <= 64; ++k) {
    const long long cand = (k * resident + bh - 1) / bh;
    if (cand >= lo) { ns = cand; break; }
  }
  ns = std::min<long long>(ns, std::max(1, (ntiles + kMinPps - 1) / kMinPps));
  if ((ntiles + ns - 1) / ns < short_pps)
    ns = std::min(ns, std::max<long long>((ntiles + short_pps - 1) / short_pps,
                                          (kMinLaunchWaves + bh - 1) / bh));
  ns = std::max(ns, lo);
  return (int)std::min(ns, max_nsplit(B, H, ntiles));
}

// The launch of a request.  resident / beam_resident / beam4_resident: the
// chip's resident waves of the plain split kernel, of the beam form (0 where
// the plain schedule runs instead) and of the tuning build's pa_beam4_kernel;
// read only for dynamic splits (pps_fixed 0).  LLM_ERR_UNSUPPORTED: the row
// needs more than kMaxSplits splits of kMaxPps pages, or a window is asked
// for grouped rows.
inline int pa_plan(const PaRequest& rq, const PaTuning& tn, long long resident,
                   long long beam_resident, long long beam4_resident, PaLaunch* out) {
  const int B = rq.B, H = rq.H, D = rq.D, TS = rq.TS, row_group = rq.row_group, kvt = rq.kv_dtype;
  const bool oproj = rq.out == PaOut::OPROJ, f32_rows = rq.out == PaOut::F32_ROWS;
  const bool out16 = rq.out == PaOut::ROW_F16 || (oproj && rq.rows16);
  // tiles at or past max_tiles have no page-table entry: they are missing (masked)
  int ntiles_max = std::max(1, std::min((rq.T + TS - 1) / TS, rq.max_tiles));
  // a window of W tokens, wherever it starts in its first page, touches at
  // most ceil(W / TS) + 1 tiles: the splits are sized for those
  if (rq.window > 0) ntiles_max = std::min(ntiles_max, (rq.window - 1) / TS + 2);
  *out = PaLaunch{};
  if (rq.window > 0 && row_group > 1) return LLM_ERR_UNSUPPORTED;
  const int pps_fixed = rq.pps_fixed > 0 ? std::min(rq.pps_fixed, kMaxPps) : 0;
  // the beam-group form: fp16 pages of two register stages
  const bool beam_shape = kvt == LLM_F16 && split_stages(D, TS, 2) == 2;
  // beam-group launches size their splits for the beam kernel's occupancy
  // (4 waves per SIMD against the plain kernel's 2: C4 8 splits, not 4)
  const long long resident_launch =
      pps_fixed <= 0 && row_group == 4 && kvt == LLM_F16 ? std::max(resident, beam_resident)
                                                         : resident;
  // fp16 o_proj input only (the FP16 decoder's attention): with at most one
  // merge batch of splits per (b, h) the splits merge inside the split
  // launch's workgroup (C2: 12 merge launches per step fewer), with long splits
  // fp32 rows for a quantising consumer (the INT8 decoder's o_proj prologue)
  // merge in the workgroup too, with a split count that divides the CU's 8
  // resident waves (2 / 4 / 8 waves per workgroup: a 6-wave workgroup would
  // leave 2 of the 8 slots idle): C3 6 -> 8 splits
  int nsplit = choose_nsplit(B, H, ntiles_max, pps_fixed, resident_launch);
  // fp32 rows whose launch is exactly one resident round of more splits than
  // a workgroup merge holds (C3's model at 8 rows per GPU: 128 (row, head)
  // pairs x 16 splits of 33 pages = 2,048 waves): half the splits, twice as
  // long, still split + merge.  Standalone (scripts/tune_attention.py --B 8,
  // profiles/r05/attention_b8_split_sweep.txt): 85.6 -> 84.3 us, the
  // loads-only form 83.7 / 83.4 us at either count.
  const bool half_round = f32_rows && row_group == 1 && pps_fixed <= 0 &&
                          (kvt == LLM_F16 || kvt == LLM_FP8) &&
                          nsplit > kWgmMaxSplits &&
                          (long long)B * H * nsplit == resident_launch &&
                          (ntiles_max + nsplit - 1) / nsplit <= 2 * kShortPps;
  if (half_round) nsplit = (nsplit + 1) / 2;
  // fp16 pools, and fp8 pools for the fp32-row merge (the INT8 decoder's): the
  // fused o_proj and the fp16 row output of the workgroup merge are fp16-KV
  // forms, so an FP16-weights decoder on fp8 pages runs split + merge-row
  const bool wgm_kvt = kvt == LLM_F16 ||
                       (kvt == LLM_FP8 && !oproj && !out16 && fp8_wgm_shape_ok(D, TS));
  const bool wgm_ok = (out16 || oproj || f32_rows) && row_group == 1 && wgm_kvt && tn.wg_merge &&
                      !half_round;
  if (wgm_ok && pps_fixed <= 0 && !f32_rows) {
    const int nw = choose_nsplit(B, H, ntiles_max, 0, resident_launch, kWgmShortPps);
    if (nw >= 2 && nw <= kWgmMaxSplits) nsplit = nw;
  }
  if (wgm_ok && pps_fixed <= 0 && f32_rows && nsplit >= 2) {
    int nw = 2;
    while (nw < nsplit && nw < kWgmMaxSplits) nw *= 2;
    if (nw >= nsplit && (long long)nw * kMaxPps >= ntiles_max) nsplit = nw;
  }
  // tuning build: forced split counts of beam-group launches and of the
  // workgroup-merge eligible ones (fp16 row outputs, dynamic splits)
  if (row_group == 4 && pps_fixed <= 0) {
    const int f = tn.beam_nsplit;
    if (f >= 2 && (long long)f * kMaxPps >= ntiles_max) nsplit = std::min(f, kMaxSplits);
  }
  if ((out16 || oproj || f32_rows) && row_group == 1 && pps_fixed <= 0) {
    const int f = tn.wgm_splits;
    if (f >= 2 && f <= kWgmMaxSplits && (long long)f * kMaxPps >= ntiles_max) nsplit = f;
  }
  // beam groups of 4 rows (fp16 pages <= 8 KiB, dynamic splits): pa_beam4_kernel,
  // one wave per (group, head, split), splits sized for its own occupancy (a
  // whole number of resident rounds over (group, head) pairs), each split
  // holding <= 128 page items; fixed pages_per_split keeps the BEAM form
  bool use_beam4 = false;
  if (row_group == 4 && pps_fixed <= 0 && beam_shape && tn.beam4 && !tn.beam_mfma) {
    const long long groups = (long long)((B + 3) / 4) * H;
    const long long need = (4LL * ntiles_max + kMaxPps - 1) / kMaxPps;
    long long ns = (beam4_resident + groups - 1) / groups;
    ns = std::max(std::max(ns, need), 2LL);
    ns = std::min(ns, max_nsplit(B, H, ntiles_max));
    if (tn.beam4_splits >= 2) ns = std::min<long long>(tn.beam4_splits, max_nsplit(B, H, ntiles_max));
    if (ns >= need && ns >= 2) {
      use_beam4 = true;
      nsplit = (int)ns;
    }
  }
  if (nsplit > kMaxSplits || (long long)nsplit * (pps_fixed > 0 ? pps_fixed : kMaxPps) < ntiles_max)
    return LLM_ERR_UNSUPPORTED;
  const int group = std::max(1, std::min(row_group, 4));  // PaSplitArgs::group
  PaLaunch p;
  p.nsplit = nsplit;
  p.pps = pps_fixed;
  p.direct = nsplit <= 1;
  p.wgm = wgm_ok && !p.direct && group == 1 && nsplit <= kWgmMaxSplits;
  p.oproj = oproj && p.wgm;
  p.beam = group == 4 && !p.direct && beam_shape;
  p.beam4 = use_beam4;
  // beam groups of 4 fp16 rows with counters: dynamic tile assignment
  p.steal = tn.beam_steal && row_group >= 4 && !p.direct && kvt == LLM_F16 && pps_fixed <= 0 &&
            !use_beam4 && !tn.beam_mfma && steal_shape_ok(D, TS);
  p.steal_ctr = rq.steal_ctr;
  p.merge_row = rq.out == PaOut::ROW_Q || out16;
  p.workspace_bytes =
      p.direct || p.wgm ? 0 : (size_t)B * H * nsplit * (size_t)(D + 2) * sizeof(float);
  *out = p;
  return LLM_OK;
}

}  // namespace llm
