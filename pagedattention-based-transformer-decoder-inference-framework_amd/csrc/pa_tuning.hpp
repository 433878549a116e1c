// The A/B switches of the attention launches (pa_decode.hip), in ONE table.
// The product library is compiled against the constant defaults below: every
// switch folds away.  The tuning build (make tune, -DLLM_TUNING=1) reads them
// from the environment per launch and may route a beam-group launch to one of
// the experiment kernels (csrc/tune/pa_decode_tune.hip, through the hooks at
// the end of pa_split.hpp); nothing else in the product sources depends on
// LLM_TUNING for attention.  No HIP types here: the planner (pa_plan.hpp) reads
// the table on the host.
#pragma once

namespace llm {

struct PaTuning {
  bool wg_merge = true;        // LLM_WG_MERGE=0: split + merge launches, no workgroup merge
  bool oproj_fuse = true;      // LLM_OPROJ_FUSE=0: the FP16 o_proj GEMM launch again
  bool beam4 = false;          // LLM_BEAM4=1: pa_beam4_kernel for beam groups
  bool beam_mfma = false;      // LLM_BEAM_MFMA=1: pa_beam_mfma_kernel for beam groups
  bool beam_steal = false;     // LLM_BEAM_STEAL=1: tiles assigned while the launch runs
  int beam_balance16 = 44;     // LLM_BEAM_BALANCE16: private-tile cost, 1/16ths (0: off);
                               // sweep in DESIGN.md §9 (C4 launch 84 -> 66 us)
  int beam_mfma_balance16 = 64;  // LLM_BEAM_MFMA_BALANCE16
  int beam_nsplit = 0;         // LLM_BEAM_NSPLIT: forced split count of beam-group launches
  int wgm_splits = 0;          // LLM_WGM_SPLITS: forced split count of workgroup-merge launches
  int beam4_splits = 0;        // LLM_BEAM4_SPLITS: forced split count of pa_beam4_kernel
  bool beam_smaj = true;       // LLM_BEAM_SMAJ=0: beam workgroups in (group, head)-major order
};

// The steal form's exchange splits a shared page's 2 NI pieces of 1 KiB over
// the 4 waves: NI = TS D / 512 even (fp16 pages of 2, 4 or 8 KiB).
constexpr bool steal_shape_ok(int D, int TS) {
  return D >= 8 && D <= 512 && (TS * D) % 1024 == 0 && TS * D * 2 <= 8192;
}

#if LLM_TUNING
PaTuning pa_tuning();
#else
constexpr PaTuning pa_tuning() { return PaTuning{}; }
#endif

}  // namespace llm
