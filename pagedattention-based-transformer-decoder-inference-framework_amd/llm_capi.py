"""ctypes binding of the C ABI (include/llm_decoder.h) exported by
libllm_decoder_hip.so.

This is the thin Python face of the drop-in boundary used by the tests and
bench.py to call individual entry points (pa_decode, i8_gemm, ...) on device
buffers they own (torch tensors, via data_ptr()).  The decoder-level surface
of the reference (CUDADecoder / INT8Decoder / PageTable / KVTileCache) is the
pybind11 module ``llm_decoder`` built next to this file.

There is no fallback: if the HIP library is missing, load() raises.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "libllm_decoder_hip.so"
TUNE_LIB_PATH = HERE / "libllm_decoder_hip_tune.so"  # `make tune`: A/B hooks, never the product

(LLM_OK, LLM_ERR_INVALID, LLM_ERR_UNSUPPORTED, LLM_ERR_HIP, LLM_ERR_OOM, LLM_ERR_IO,
 LLM_ERR_RANGE) = range(7)
LLM_F16, LLM_I8, LLM_F32, LLM_BF16, LLM_FP8 = 0, 1, 2, 3, 4
LLM_ACT_NONE, LLM_ACT_RELU, LLM_ACT_GELU = 0, 1, 2
LLM_EVICT_NONE, LLM_EVICT_LRU = 0, 1

c_int, c_float, c_void_p, c_size_t = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
c_ll = ctypes.c_longlong
c_i32p = ctypes.POINTER(ctypes.c_int32)


class PaKvView(ctypes.Structure):
    _fields_ = [("k_pool", c_void_p), ("v_pool", c_void_p), ("page_table", c_void_p),
                ("num_pages", ctypes.c_int32), ("page_size", ctypes.c_int32),
                ("head_dim", ctypes.c_int32), ("num_beams", ctypes.c_int32),
                ("num_heads", ctypes.c_int32), ("max_tiles", ctypes.c_int32),
                ("kv_dtype", ctypes.c_int32), ("page_stride", ctypes.c_int64)]


class PaPrefillSeg(ctypes.Structure):
    """pa_prefill_seg: len rows at positions p0 .. of page-table row `row`."""
    _fields_ = [("row", ctypes.c_int32), ("p0", ctypes.c_int32), ("len", ctypes.c_int32)]


class WeightGemmTuneArgs(ctypes.Structure):
    """weight_gemm_tune's argument (csrc/tune/gemm_tune.hip, tuning library only):
    every field of the decoder's WeightGemm and, with has_kv, of KvAppendView
    (csrc/gemm.hpp); zero-initialised fields are the structs' defaults except
    ln_eps, kv_dtype (LLM_F16 is 0) and the inverse scales."""
    _fields_ = [("dtype", c_int), ("A", c_void_p), ("lda", c_int), ("a_packed", c_int),
                ("W_packed", c_void_p), ("M", c_int), ("N", c_int), ("K", c_int),
                ("sa", c_void_p), ("sw", c_void_p), ("bias", c_void_p), ("act", c_int),
                ("C", c_void_p), ("c_cols", c_int), ("c_ld", c_int), ("C16", c_void_p),
                ("ln_x", c_void_p), ("ln_emb", c_void_p), ("ln_tok", c_void_p), ("ln_V", c_int),
                ("ln_g", c_void_p), ("ln_b", c_void_p), ("ln_eps", c_float),
                ("act_out", c_void_p), ("sa_out", c_void_p), ("w_keep", c_int),
                ("ln_quant_only", c_int), ("ksplit2", c_int), ("has_kv", c_int),
                ("kv_pos", c_void_p), ("kv_page_table", c_void_p), ("kv_rows", c_void_p),
                ("kv_k_pool", c_void_p), ("kv_v_pool", c_void_p), ("kv_num_beams", c_int),
                ("kv_max_tiles", c_int), ("kv_page_size", c_int), ("kv_num_pages", c_int),
                ("kv_H", c_int), ("kv_D", c_int), ("kv_page_stride", c_ll),
                ("kv_dtype", c_int), ("kv_k_inv_scale", c_float), ("kv_v_inv_scale", c_float),
                ("kv_rope", c_void_p), ("kv_rope_len", c_int)]


class PaRowsTuneArgs(ctypes.Structure):
    """pa_rows_tune's argument (csrc/tune/pa_decode_tune.hip, tuning library
    only): which internal attention entry to call (launch 0 decode, 1 prefill,
    2 packed prefill), its arguments, the PaRowOutputs fields (has_rows 0:
    rows = NULL), for decode the launch that ran (nsplit, form), and the fused
    o_proj's fields (out_kind PA_OUT_OPROJ)."""
    _fields_ = [("launch", c_int), ("kv", ctypes.POINTER(PaKvView)), ("q", c_void_p),
                ("q_stride", c_int), ("sm_scale", c_float), ("window", c_int),
                ("workspace", c_void_p), ("workspace_bytes", c_size_t),
                ("beam_ids", c_void_p), ("context_lens", c_void_p), ("B", c_int), ("H", c_int),
                ("D", c_int), ("T", c_int), ("pages_per_split", c_int), ("row_group", c_int),
                ("out_kind", c_int), ("row", c_int), ("p0", c_int), ("m", c_int),
                ("segs", ctypes.POINTER(PaPrefillSeg)), ("nseg", c_int), ("has_rows", c_int),
                ("rows_q", c_void_p), ("inv_scale", c_void_p), ("out16", c_void_p),
                ("pack", c_int), ("keep_out", c_int), ("out_scale", c_float), ("out", c_void_p),
                ("out_stride", c_int), ("nsplit", c_int), ("form", c_int),
                ("o_acc", c_void_p), ("o_x", c_void_p), ("wo_heads", c_void_p), ("o_n", c_int),
                ("o_flag", c_void_p), ("rows16", c_int)]


class PaDecodeOptions(ctypes.Structure):
    _fields_ = [("temperature", ctypes.c_float), ("top_k", ctypes.c_int),
                ("top_p", ctypes.c_float), ("eos_token", ctypes.c_int),
                ("eos_threshold", ctypes.c_float), ("probs_out", c_void_p),
                ("scores_out", c_void_p)]


class LlmBeamOptions(ctypes.Structure):
    """llm_beam_options: the trace pointers are host arrays ([steps][num_seqs][2W]
    candidates, [steps][num_seqs][W] live beams) except trace_logits_dev."""
    _fields_ = [("beam_width", ctypes.c_int), ("max_new_tokens", ctypes.c_int),
                ("eos_token", ctypes.c_int), ("length_penalty", ctypes.c_float),
                ("trace_cand_parent", c_void_p), ("trace_cand_token", c_void_p),
                ("trace_cand_score", c_void_p), ("trace_live_parent", c_void_p),
                ("trace_live_token", c_void_p), ("trace_logits_dev", c_void_p),
                ("steps_run", ctypes.POINTER(ctypes.c_int))]


LLM_FINISH_EOS, LLM_FINISH_LENGTH = 1, 2
LLM_MAX_TOP_LOGPROBS = 8


class LlmRequestOptions(ctypes.Structure):
    """llm_request_options of llm_decoder_submit."""
    _fields_ = [("max_new_tokens", ctypes.c_int), ("eos_token", ctypes.c_int),
                ("temperature", ctypes.c_float), ("top_k", ctypes.c_int),
                ("top_p", ctypes.c_float), ("seed", ctypes.c_uint64)]


class LlmServeEvent(ctypes.Structure):
    """llm_serve_event of llm_decoder_serve_step."""
    _fields_ = [("id", ctypes.c_longlong), ("token", ctypes.c_int32), ("index", ctypes.c_int32),
                ("row", ctypes.c_int32), ("finish", ctypes.c_int32)]


class LlmServeOptions(ctypes.Structure):
    """llm_serve_options of llm_decoder_serve_begin_opts."""
    _fields_ = [("prefix_cache", ctypes.c_int)]


class LlmPrefixStats(ctypes.Structure):
    """llm_prefix_stats of llm_decoder_serve_prefix_stats."""
    _fields_ = [(n, ctypes.c_longlong) for n in
                ("positions_due", "positions_hit", "cached_blocks", "idle_pages",
                 "evicted_blocks", "deferrals")]


class LlmError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"[llm status {status}] {msg}")
        self.status = status


# name -> (restype, argtypes)
_SIGS = {
    "llm_last_error": (ctypes.c_char_p, []),
    "llm_abi_version": (c_int, []),
    "llm_fp8_e4m3_encode": (c_int, [c_void_p, c_size_t, c_float, c_void_p]),
    "llm_fp8_e4m3_decode": (c_int, [c_void_p, c_size_t, c_float, c_void_p]),
    "llm_decoder_create_kv": (c_int, [c_void_p, c_int, ctypes.POINTER(c_void_p)]),
    "llm_decoder_set_kv_scales": (c_int, [c_void_p, c_void_p, c_void_p]),
    "llm_decoder_kv_dtype": (c_int, [c_void_p]),
    "llm_rope_table": (c_int, [ctypes.c_double, c_int, c_int, c_void_p]),
    "rope_rows": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int,
                          c_void_p]),
    "llm_decoder_set_rope": (c_int, [c_void_p, c_void_p]),
    "llm_decoder_rope": (c_int, [c_void_p]),
    "llm_decoder_prefill_kernel": (c_int, [c_void_p]),
    "llm_decoder_destroy": (None, [c_void_p]),
    "llm_decoder_begin_synthetic": (c_int, [c_void_p, c_int, c_int, ctypes.c_uint64, c_int]),
    "pa_decode_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "pa_decode_pages_per_split": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "pa_decode_plan": (c_int, [ctypes.POINTER(PaKvView), c_int, c_int, c_int, c_int, c_int, c_int,
                               c_i32p, c_i32p]),
    "pa_decode_window_plan": (c_int, [ctypes.POINTER(PaKvView), c_int, c_int, c_int, c_int, c_int,
                                      c_int, c_i32p, c_i32p]),
    # tuning library only: the launch planner on explicit request fields
    "pa_plan_tune": (c_int, [c_int] * 11 + [c_ll] * 3 + [c_i32p, c_i32p]),
    # ... and with a sliding window (after row_group)
    "pa_plan_window_tune": (c_int, [c_int] * 12 + [c_ll] * 3 + [c_i32p, c_i32p]),
    # tuning library only: the prefill pass packer (csrc/prefill_pack.hpp)
    "prefill_passes_tune": (c_int, [c_i32p, c_i32p, c_int, c_int, c_i32p, c_int]),
    "pa_decode": (c_int, [ctypes.POINTER(PaKvView), c_void_p, c_void_p, c_void_p, c_void_p,
                          c_int, c_int, c_int, c_int, c_float, c_int, c_void_p, c_size_t,
                          c_void_p]),
    "pa_decode_window": (c_int, [ctypes.POINTER(PaKvView), c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p,
                                 c_size_t, c_void_p]),
    "pa_decode_grouped": (c_int, [ctypes.POINTER(PaKvView), c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_int,
                                  c_void_p, c_size_t, c_void_p]),
    "pa_decode_ex": (c_int, [ctypes.POINTER(PaKvView), c_void_p, c_void_p, c_void_p, c_void_p,
                             c_int, c_int, c_int, c_int, ctypes.POINTER(PaDecodeOptions),
                             c_void_p, c_size_t, c_void_p]),
    "pa_prefill_workspace_bytes": (c_size_t, [ctypes.POINTER(PaKvView), c_int, c_int]),
    "pa_decode_ex_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "pa_prefill": (c_int, [ctypes.POINTER(PaKvView), c_void_p, c_int, c_void_p, c_int, c_int,
                           c_int, c_int, c_float, c_void_p, c_size_t, c_void_p]),
    "pa_prefill_window": (c_int, [ctypes.POINTER(PaKvView), c_void_p, c_int, c_void_p, c_int, c_int,
                                  c_int, c_int, c_float, c_int, c_void_p, c_size_t, c_void_p]),
    "pa_prefill_packed_window": (c_int, [ctypes.POINTER(PaKvView), c_void_p, c_int, c_void_p,
                                         c_int, ctypes.POINTER(PaPrefillSeg), c_int, c_float,
                                         c_int, c_void_p, c_size_t, c_void_p]),
    "pa_prefill_packed_tiles": (c_int, [ctypes.POINTER(PaKvView), ctypes.POINTER(PaPrefillSeg),
                                        c_int, c_i32p, c_int]),
    "pa_prefill_packed_workspace_bytes": (c_size_t, [ctypes.POINTER(PaKvView),
                                                     ctypes.POINTER(PaPrefillSeg), c_int, c_int]),
    "pa_prefill_packed": (c_int, [ctypes.POINTER(PaKvView), c_void_p, c_int, c_void_p, c_int,
                                  ctypes.POINTER(PaPrefillSeg), c_int, c_float, c_void_p,
                                  c_size_t, c_void_p]),
    "llm_decoder_prefill_rows": (c_int, [c_void_p, c_i32p, c_i32p, c_i32p, c_int]),
    "llm_decoder_set_packed_prefill": (c_int, [c_void_p, c_int]),
    "llm_decoder_packed_prefill": (c_int, [c_void_p]),
    "gemm_packed_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gemm_pack_weights": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "i8_gemm": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                        c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "i8_matmul_s8": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float,
                             c_float, c_float, c_void_p, c_int, c_void_p]),
    "f16_gemm": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                         c_int, c_void_p]),
    "lm_head": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "lm_head_logprobs": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                 c_int, c_void_p]),
    "logprob_rows": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_void_p]),
    "argmax_rows": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "sample_rows": (c_int, [c_void_p, c_int, c_int, c_float, c_int, c_float, ctypes.c_uint64,
                            c_int, c_void_p, c_void_p]),
    "sample_rows_each": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p]),
    "sample_uniform_host": (c_float, [ctypes.c_uint64, c_int, c_int]),
    # continuous batching (llm_decoder_serve_*)
    "llm_decoder_serve_begin": (c_int, [c_void_p]),
    "llm_decoder_serve_end": (c_int, [c_void_p]),
    "llm_decoder_serve_begin_opts": (c_int, [c_void_p, ctypes.POINTER(LlmServeOptions)]),
    "llm_decoder_serve_prefix_stats": (c_int, [c_void_p, ctypes.POINTER(LlmPrefixStats)]),
    "llm_decoder_submit": (c_int, [c_void_p, c_i32p, c_int, ctypes.POINTER(LlmRequestOptions),
                                   ctypes.POINTER(c_ll)]),
    "llm_decoder_submit_logprobs": (c_int, [c_void_p, c_i32p, c_int,
                                            ctypes.POINTER(LlmRequestOptions), c_int,
                                            ctypes.POINTER(c_ll)]),
    "llm_decoder_serve_logprobs": (c_int, [c_void_p, ctypes.POINTER(c_float),
                                           ctypes.POINTER(c_float), c_i32p, c_i32p]),
    "llm_decoder_score": (c_int, [c_void_p, c_i32p, c_i32p, c_int, c_int,
                                  ctypes.POINTER(c_float)]),
    "llm_decoder_cancel": (c_int, [c_void_p, c_ll]),
    "llm_decoder_serve_step": (c_int, [c_void_p, c_void_p, ctypes.POINTER(LlmServeEvent), c_int,
                                       ctypes.POINTER(c_int)]),
    "llm_decoder_serve_stats": (c_int, [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                                        ctypes.POINTER(c_ll), ctypes.POINTER(c_ll)]),
    # tuning library only: the continuous-batching scheduler (csrc/serve_plan.hpp)
    "serve_plan_sim_tune": (c_int, [c_i32p, c_i32p, c_i32p, c_int, c_int, c_ll, c_int, c_int,
                                    c_int, c_int, ctypes.POINTER(c_ll), c_int]),
    # tuning library only: ... with prompts and the prefix cache (csrc/prefix_cache.hpp)
    "serve_prefix_sim_tune": (c_int, [c_i32p, c_i32p, c_i32p, c_i32p, c_int, c_int, c_ll, c_int,
                                      c_int, c_int, c_int, ctypes.POINTER(c_ll), c_int,
                                      ctypes.POINTER(c_ll)]),
    # tuning library only: the beam search's host bookkeeping (csrc/beam_plan.hpp)
    "beam_book_tune": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 6 + [c_float] +
                       [c_void_p] * 7),
    "beam_select_rows": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                 c_void_p, c_void_p]),
    "kv_cache_reorder": (c_int, [c_void_p, c_int, c_int, c_i32p, c_int]),
    "kv_cache_cow_copies": (c_ll, [c_void_p]),
    "llm_decoder_beam_search": (c_int, [c_void_p, c_i32p, c_i32p, c_int, c_int,
                                        ctypes.POINTER(LlmBeamOptions), c_i32p, c_i32p,
                                        ctypes.POINTER(c_float), ctypes.POINTER(c_float)]),
    "quantize_rows": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "layernorm_quant": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p,
                                c_void_p, c_void_p, c_void_p]),
    # tuning library only (csrc/tune/row_ops_tune.hip): the row launchers in the
    # forms the decoder runs them (pack, embedding source, zero_x, fp16 output)
    "layernorm_quant_tune": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p,
                                     c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                     c_void_p, c_void_p]),
    "layernorm_f16_tune": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p,
                                   c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "quantize_rows_tune": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "to_f16_tune": (c_int, [c_void_p, c_size_t, c_void_p, c_int, c_void_p]),
    # tuning library only (csrc/tune/gemm_tune.hip): the decoder's weight_gemm,
    # its prologue predicates, the form launch_gemm picks and the forced forms
    "weight_gemm_tune": (c_int, [ctypes.POINTER(WeightGemmTuneArgs), c_void_p]),
    # tuning library only (csrc/tune/pa_decode_tune.hip): the internal attention
    # entries with their row outputs
    "pa_rows_tune": (c_int, [ctypes.POINTER(PaRowsTuneArgs), c_void_p]),
    # tuning library only: the fused o_proj's W_o head slices (csrc/oproj_slices.hpp), host only
    "oproj_head_slices_tune": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p]),
    "gemm_ln_fusable_tune": (c_int, [c_int, c_int, c_int]),
    "gemm_quant_prologue_ok_tune": (c_int, [c_int, c_int, c_int]),
    "gemm_form_tune": (c_int, [c_int] * 9 + [c_i32p]),
    "f16_gemm_tune": (c_int, [c_int] * 4 + [c_void_p, c_int, c_void_p, c_void_p] + [c_int] * 3 +
                      [c_void_p]),
    "kv_cache_create": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_ll,
                                ctypes.POINTER(c_void_p)]),
    "kv_cache_create_typed": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_ll, c_int,
                                      ctypes.POINTER(c_void_p)]),
    "kv_cache_destroy": (None, [c_void_p]),
    "kv_cache_view": (c_int, [c_void_p, c_int, ctypes.POINTER(PaKvView)]),
    "kv_cache_num_pages": (c_ll, [c_void_p]),
    "kv_cache_free_pages": (c_ll, [c_void_p]),
    "kv_cache_assign": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int]),
    "kv_cache_lookup": (c_int, [c_void_p, c_int, c_int, c_int, c_int]),
    "kv_cache_remove": (c_int, [c_void_p, c_int, c_int, c_int, c_int]),
    "kv_cache_register_tile": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_i32p]),
    "kv_cache_set_eviction": (c_int, [c_void_p, c_int]),
    "kv_cache_reserve": (c_int, [c_void_p, c_int, c_int]),
    "kv_cache_fork": (c_int, [c_void_p, c_int, c_int]),
    "kv_cache_release": (c_int, [c_void_p, c_int]),
    "kv_cache_hold_tile": (c_int, [c_void_p, c_int, c_int, c_i32p]),
    "kv_cache_attach_tile": (c_int, [c_void_p, c_int, c_int, c_i32p]),
    "kv_cache_drop_pages": (c_int, [c_void_p, c_i32p]),
    "kv_cache_release_before": (c_int, [c_void_p, c_int, c_int]),
    "llm_decoder_set_window": (c_int, [c_void_p, c_int]),
    "llm_decoder_window": (c_int, [c_void_p]),
    "kv_cache_clear": (c_int, [c_void_p]),
    "kv_cache_sync": (c_int, [c_void_p, c_void_p]),
    "kv_cache_write_tokens": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "kv_cache_k_pool": (c_void_p, [c_void_p]),
    "kv_cache_v_pool": (c_void_p, [c_void_p]),
    "kv_cache_page_stride": (ctypes.c_longlong, [c_void_p]),
    "kv_cache_page_table": (c_void_p, [c_void_p, c_int]),
    "kv_cache_save": (c_int, [c_void_p, ctypes.c_char_p]),
    "kv_cache_load": (c_int, [c_void_p, ctypes.c_char_p]),
    "kv_cache_inspect": (c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_longlong)]),
    "kv_cache_save_pools": (c_int, [c_void_p, ctypes.c_char_p]),
    "kv_cache_load_pools": (c_int, [c_void_p, ctypes.c_char_p]),
    "kv_cache_save_tiles": (c_int, [c_void_p, c_int, c_int, ctypes.c_char_p]),
    "kv_cache_load_tiles": (c_int, [c_void_p, c_int, c_int, ctypes.c_char_p]),
    "kv_tiles_inspect": (c_int, [ctypes.c_char_p, ctypes.c_longlong, ctypes.POINTER(c_int)]),
    "llm_decoder_oproj_status": (c_int, [c_void_p, ctypes.POINTER(c_int),
                                         ctypes.POINTER(ctypes.c_longlong)]),
}

_lib = None


def declared_symbols() -> list[str]:
    """Every function name declared in include/llm_decoder.h."""
    import re
    hdr = (HERE.parent / "include" / "llm_decoder.h").read_text()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = re.findall(r"\b([a-z_][a-z0-9_]*)\s*\(", hdr)
    skip = {"if", "for", "while", "sizeof", "return", "defined"}
    return sorted({n for n in names if n not in skip})


def load(path: str | Path | None = None) -> ctypes.CDLL:
    """Load the HIP C-ABI library (raises if it is missing: no fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # LLM_CAPI_LIB: another build of the same library (same-box A/B of build flags)
    p = Path(path) if path else Path(os.environ.get("LLM_CAPI_LIB", LIB_PATH))
    if not p.exists():
        raise FileNotFoundError(
            f"{p} not found: build it with `make -C {HERE}` (or __graft_entry__.build())")
    lib = ctypes.CDLL(str(p), mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in _SIGS.items():
        if not hasattr(lib, name):  # export completeness is asserted by tests/test_capi_symbols.py
            continue
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    if path is None:
        _lib = lib
    return lib


_tune = None


def load_tune() -> ctypes.CDLL:
    """The tuning build (pa_decode_tune, i8_gemm_tune, i8_gemm_stamps and the
    env overrides), loaded RTLD_LOCAL beside the product library; for scripts
    and the variant tests only."""
    global _tune
    if _tune is None:
        if not TUNE_LIB_PATH.exists():
            raise FileNotFoundError(f"{TUNE_LIB_PATH} not found: `make -C {HERE} tune`")
        _tune = ctypes.CDLL(str(TUNE_LIB_PATH), mode=ctypes.RTLD_LOCAL)
        for name, (res, args) in _SIGS.items():
            if hasattr(_tune, name):
                f = getattr(_tune, name)
                f.restype = res
                f.argtypes = args
    return _tune


def check(status: int, lib: ctypes.CDLL | None = None) -> None:
    if status != LLM_OK:
        msg = (lib or load()).llm_last_error()
        raise LlmError(status, msg.decode() if msg else "")


def stream_ptr(stream=None):
    """hipStream_t of a torch stream (current stream by default) as void*."""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def ptr(t) -> ctypes.c_void_p:
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def kv_dtype_of(t) -> int:
    """llm_dtype of a torch KV pool tensor (fp16, bf16, fp32, int8 or float8_e4m3fn)."""
    import torch
    m = {torch.float16: LLM_F16, torch.bfloat16: LLM_BF16, torch.float32: LLM_F32,
         torch.int8: LLM_I8, torch.float8_e4m3fn: LLM_FP8}
    if t.dtype not in m:
        raise TypeError(f"KV pool dtype {t.dtype} is not one of fp16/bf16/fp32/int8/float8_e4m3fn")
    return m[t.dtype]


def fp8_encode(x, scale: float = 1.0):
    """llm_fp8_e4m3_encode of a float32 numpy array: uint8 array of the same shape."""
    import numpy as np
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty(x.shape, dtype=np.uint8)
    check(load().llm_fp8_e4m3_encode(x.ctypes.data, x.size, scale, out.ctypes.data))
    return out


def fp8_decode(b, scale: float = 1.0):
    """llm_fp8_e4m3_decode of a uint8 numpy array: float32 array of the same shape."""
    import numpy as np
    b = np.ascontiguousarray(b, dtype=np.uint8)
    out = np.empty(b.shape, dtype=np.float32)
    check(load().llm_fp8_e4m3_decode(b.ctypes.data, b.size, scale, out.ctypes.data))
    return out


def kv_view(k_pool, v_pool, page_table, *, num_beams=None) -> PaKvView:
    """View over torch device tensors k/v [num_pages][ts][D] (fp16, bf16, fp32,
    int8 or float8_e4m3fn, both the same) and page table int32 [num_beams][H][max_tiles].
    Pages may be strided (e.g. k = kv[:, 0], v = kv[:, 1] of one
    [num_pages][2][ts][D] tensor: K and V pages interleaved) as long as each
    page is contiguous; the view's page_stride is then the page-to-page step."""
    nb, H, mt = page_table.shape
    for t in (k_pool, v_pool):
        if t.dim() != 3 or t.stride(2) != 1 or t.stride(1) != t.shape[2]:
            raise ValueError("KV pools must be [num_pages][ts][D] with contiguous pages")
    if k_pool.stride(0) != v_pool.stride(0):
        raise ValueError("k_pool and v_pool must share one page stride")
    v = PaKvView()
    v.k_pool, v.v_pool, v.page_table = k_pool.data_ptr(), v_pool.data_ptr(), page_table.data_ptr()
    v.num_pages, v.page_size, v.head_dim = k_pool.shape[0], k_pool.shape[1], k_pool.shape[2]
    v.num_beams, v.num_heads, v.max_tiles = num_beams or nb, H, mt
    if k_pool.dtype != v_pool.dtype:
        raise TypeError("k_pool and v_pool must have the same dtype")
    v.kv_dtype = kv_dtype_of(k_pool)
    dense = k_pool.shape[1] * k_pool.shape[2]
    v.page_stride = 0 if k_pool.stride(0) == dense else k_pool.stride(0) * k_pool.element_size()
    return v


def pa_decode(q, k_pool, v_pool, page_table, *, T, beam_ids=None, context_lens=None,
              sm_scale=1.0, pages_per_split=0, out=None, stream=None, row_group=1, lib=None,
              window=None):
    """Paged decode attention on torch device tensors; returns out [B][H][D] fp32.
    row_group > 1 uses the beam-aware schedule (pa_decode_grouped).  lib: the
    library to call (default the product build; load_tune() for variant tests).
    window (not None): pa_decode_window, row b attends to its last `window` tokens."""
    import torch
    lib = lib or load()
    B, H, D = q.shape
    if out is None:
        out = torch.empty((B, H, D), dtype=torch.float32, device=q.device)
    view = kv_view(k_pool, v_pool, page_table)
    ws_bytes = lib.pa_decode_workspace_bytes(B, H, D, page_table.shape[2], pages_per_split)
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=q.device)
    if window is not None:
        if row_group > 1:
            raise ValueError("pa_decode: a window needs row_group 1")
        check(lib.pa_decode_window(ctypes.byref(view), ptr(q), ptr(out), ptr(beam_ids),
                                   ptr(context_lens), B, H, D, T, sm_scale, pages_per_split,
                                   window, ptr(ws), ws_bytes, stream_ptr(stream)), lib)
    elif row_group > 1:
        check(lib.pa_decode_grouped(ctypes.byref(view), ptr(q), ptr(out), ptr(beam_ids),
                                    ptr(context_lens), B, H, D, T, sm_scale, pages_per_split,
                                    row_group, ptr(ws), ws_bytes, stream_ptr(stream)))
    else:
        check(lib.pa_decode(ctypes.byref(view), ptr(q), ptr(out), ptr(beam_ids),
                            ptr(context_lens), B, H, D, T, sm_scale, pages_per_split, ptr(ws),
                            ws_bytes, stream_ptr(stream)))
    return out


def pa_decode_plan(k_pool, v_pool, page_table, *, B, T, pages_per_split=0, row_group=1,
                   window=None, lib=None):
    """(nsplit, form) of the pa_decode / pa_decode_grouped call with these
    arguments, or of pa_decode_window when window is not None."""
    lib = lib or load()
    view = kv_view(k_pool, v_pool, page_table)
    H, D = page_table.shape[1], k_pool.shape[2]
    ns, form = ctypes.c_int32(0), ctypes.c_int32(0)
    if window is not None:
        check(lib.pa_decode_window_plan(ctypes.byref(view), B, H, D, T, pages_per_split, window,
                                        ctypes.byref(ns), ctypes.byref(form)), lib)
    else:
        check(lib.pa_decode_plan(ctypes.byref(view), B, H, D, T, pages_per_split, row_group,
                                 ctypes.byref(ns), ctypes.byref(form)), lib)
    return ns.value, form.value


def pa_decode_ex(q, k_pool, v_pool, page_table, *, T, beam_ids=None, context_lens=None,
                 temperature=1.0, top_k=0, top_p=1.0, eos_token=-1, eos_threshold=0.0,
                 want_probs=False, stream=None):
    """pa_decode_ex on torch device tensors.  Returns out [B][H][D] fp32, or
    (out, probs [B][H][T], scores [B][H][T]) when want_probs."""
    import torch
    lib = load()
    B, H, D = q.shape
    out = torch.empty((B, H, D), dtype=torch.float32, device=q.device)
    probs = torch.empty((B, H, T), dtype=torch.float32, device=q.device) if want_probs else None
    scores = torch.empty((B, H, T), dtype=torch.float32, device=q.device) if want_probs else None
    view = kv_view(k_pool, v_pool, page_table)
    opt = PaDecodeOptions(temperature=temperature, top_k=top_k, top_p=top_p, eos_token=eos_token,
                          eos_threshold=eos_threshold,
                          probs_out=None if probs is None else probs.data_ptr(),
                          scores_out=None if scores is None else scores.data_ptr())
    ws_bytes = max(lib.pa_decode_workspace_bytes(B, H, D, page_table.shape[2], 0),
                   lib.pa_decode_ex_workspace_bytes(B, H, T))
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=q.device)
    check(lib.pa_decode_ex(ctypes.byref(view), ptr(q), ptr(out), ptr(beam_ids), ptr(context_lens),
                           B, H, D, T, ctypes.byref(opt), ptr(ws), ws_bytes, stream_ptr(stream)))
    return (out, probs, scores) if want_probs else out


def pa_prefill(q, k_pool, v_pool, page_table, *, row, p0, sm_scale=1.0, out=None,
               split=True, stream=None, window=None):
    """Causal attention of a prompt chunk (pa_prefill): q [m][H][D] (or a
    [m][stride] row view whose first H*D floats are the heads) at positions
    p0 .. p0+m-1 of page-table row `row`; returns out [m][H][D] fp32.
    split=False runs the one-pass form (no workspace).  window (not None):
    pa_prefill_window, query i sees positions max(0, p0+i-window+1) .. p0+i."""
    import torch
    lib = load()
    m = q.shape[0]
    H, D = page_table.shape[1], k_pool.shape[2]
    q_stride = q.stride(0)
    if q.stride(-1) != 1:
        raise ValueError("q rows must be contiguous")
    if out is None:
        out = torch.empty((m, H, D), dtype=torch.float32, device=q.device)
    view = kv_view(k_pool, v_pool, page_table)
    ws_bytes = lib.pa_prefill_workspace_bytes(ctypes.byref(view), p0, m) if split else 0
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=q.device) if ws_bytes else None
    if window is not None:
        check(lib.pa_prefill_window(ctypes.byref(view), ptr(q), q_stride, ptr(out), out.stride(0),
                                    row, p0, m, sm_scale, window, ptr(ws), ws_bytes,
                                    stream_ptr(stream)))
        return out
    check(lib.pa_prefill(ctypes.byref(view), ptr(q), q_stride, ptr(out), out.stride(0), row, p0,
                         m, sm_scale, ptr(ws), ws_bytes, stream_ptr(stream)))
    return out


def prefill_segs(segs):
    """A ctypes pa_prefill_seg array of (row, p0, len) tuples."""
    return (PaPrefillSeg * max(len(segs), 1))(*[PaPrefillSeg(*map(int, s)) for s in segs])


def pa_prefill_packed(q, k_pool, v_pool, page_table, *, segs, sm_scale=1.0, out=None,
                      split=True, stream=None, window=None):
    """Causal attention of prompt chunks of several sequences in one launch
    (pa_prefill_packed): q [m][H][D] (or a [m][stride] row view whose first
    H*D floats are the heads), m = sum of the segment lengths, segs =
    [(row, p0, len), ...] in packed order; returns out [m][H][D] fp32.
    split=False gives the workspace of the one-pass form.  window (not None):
    pa_prefill_packed_window."""
    import torch
    lib = load()
    m = q.shape[0]
    H, D = page_table.shape[1], k_pool.shape[2]
    if q.stride(-1) != 1:
        raise ValueError("q rows must be contiguous")
    if m != sum(int(s[2]) for s in segs):
        raise ValueError("q rows must equal the sum of the segment lengths")
    if out is None:
        out = torch.empty((m, H, D), dtype=torch.float32, device=q.device)
    view = kv_view(k_pool, v_pool, page_table)
    arr = prefill_segs(segs)
    ws_bytes = lib.pa_prefill_packed_workspace_bytes(ctypes.byref(view), arr, len(segs),
                                                     1 if split else 0)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=q.device)
    if window is not None:
        check(lib.pa_prefill_packed_window(ctypes.byref(view), ptr(q), q.stride(0), ptr(out),
                                           out.stride(0), arr, len(segs), sm_scale, window,
                                           ptr(ws), ws_bytes, stream_ptr(stream)))
        return out
    check(lib.pa_prefill_packed(ctypes.byref(view), ptr(q), q.stride(0), ptr(out), out.stride(0),
                                arr, len(segs), sm_scale, ptr(ws), ws_bytes, stream_ptr(stream)))
    return out


# csrc/pa_plan.hpp PaOut
PA_OUT_F32, PA_OUT_ROW_Q, PA_OUT_ROW_F16, PA_OUT_F32_ROWS, PA_OUT_OPROJ = range(5)
PA_ROWS_SENTINEL = 0x5A  # every byte of the int8 / fp16 row buffers (and of o_x) before the call


def oproj_head_slices(wo, H, D):
    """oproj_head_slices_tune (tuning library, host only): a host fp16 W_o
    [H*D][o_n] as the fused o_proj's head slices, uint16 [H][D/8][o_n][8]."""
    import numpy as np
    wo = np.ascontiguousarray(wo, dtype=np.float16)
    if wo.ndim != 2 or wo.shape[0] != H * D:
        raise ValueError("W_o must be [H*D][o_n]")
    tune = load_tune()
    out = np.empty((H, D // 8, wo.shape[1], 8), np.uint16)
    check(tune.oproj_head_slices_tune(wo.ctypes.data, H, D, wo.shape[1], out.ctypes.data), tune)
    return out


def pa_rows(q, k_pool, v_pool, page_table, *, launch, out_kind, T=0, beam_ids=None,
            context_lens=None, pages_per_split=0, row_group=1, row=0, p0=0, segs=None,
            sm_scale=1.0, window=0, pack=1, keep_out=1, out_scale=1.0, want_out=True,
            split=True, has_rows=True, omit=(), stream=None, wo=None, o_n=None, o_acc=None,
            o_flag=None, rows16=0, sync=True):
    """pa_rows_tune (tuning library): one of the internal attention entries with
    its row outputs, on torch device tensors.  launch "decode" (q [B][H][D]),
    "prefill" (q [m][H][D] at positions p0 .. of page-table row `row`) or
    "packed" (segs [(row, p0, len), ...]); out_kind PA_OUT_ROW_Q / ROW_F16 /
    F32_ROWS says which row buffers the entry gets (the prefill entries take
    it from the pointers alone); omit: names of buffers ("q", "inv_scale",
    "out16") passed as NULL all the same.  want_out=False passes out = NULL;
    split=False gives the prefill entries no split workspace (one pass).
    Returns a dict: status, error (text of a refusal), out fp32 [rows][H*D]
    (pre-filled with NaN) or None, q8 int8 and out16 int16 bit patterns of
    rows16 * H*D elements when packed (rows16 = rows rounded up to 16; every
    byte pre-filled with PA_ROWS_SENTINEL) else rows * H*D, inv_scale fp32
    [rows] (NaN), nsplit, form (decode).
    out_kind PA_OUT_OPROJ (decode; the FP16 decoder's fused o_proj): wo is the
    host fp16 W_o [H*D][o_n], sliced by oproj_head_slices and uploaded; o_n
    overrides the column count the launch is told; o_acc int64 [(rows + 1) *
    o_n] and o_flag int32 [1] are the caller's buffers of an earlier launch, or
    allocated as zeros; rows16 asks for out16 as well; omit may name "o_flag".
    The dict then also holds x fp32 [rows + 1][o_n] (every byte pre-filled
    with PA_ROWS_SENTINEL; the last row is never the launch's), o_acc as the
    launch left it and o_flag.  sync=False returns without waiting for the
    launch (launches back to back on one stream)."""
    import torch
    tune = load_tune()
    rows = q.shape[0]
    H, D = page_table.shape[1], k_pool.shape[2]
    hid = H * D
    if q.stride(-1) != 1:
        raise ValueError("q rows must be contiguous")
    dev = q.device
    view = kv_view(k_pool, v_pool, page_table)
    a = PaRowsTuneArgs()
    a.launch = {"decode": 0, "prefill": 1, "packed": 2}[launch]
    a.kv = ctypes.pointer(view)
    a.q, a.q_stride, a.sm_scale, a.window = q.data_ptr(), q.stride(0), sm_scale, window
    seg_arr = None
    if launch == "decode":
        ws_bytes = tune.pa_decode_workspace_bytes(rows, H, D, page_table.shape[2], pages_per_split)
        a.beam_ids = None if beam_ids is None else beam_ids.data_ptr()
        a.context_lens = None if context_lens is None else context_lens.data_ptr()
        a.B, a.H, a.D, a.T = rows, H, D, T
        a.pages_per_split, a.row_group = pages_per_split, row_group
    elif launch == "prefill":
        ws_bytes = tune.pa_prefill_workspace_bytes(ctypes.byref(view), p0, rows) if split else 0
        a.row, a.p0, a.m = row, p0, rows
    else:
        seg_arr = prefill_segs(segs)
        ws_bytes = tune.pa_prefill_packed_workspace_bytes(ctypes.byref(view), seg_arr, len(segs),
                                                          1 if split else 0)
        a.segs, a.nseg = seg_arr, len(segs)
    a.out_kind = out_kind
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev) if ws_bytes else None
    a.workspace, a.workspace_bytes = (None, 0) if ws is None else (ws.data_ptr(), ws_bytes)
    n_el = ((rows + 15) // 16 * 16 if pack else rows) * hid
    fill16 = PA_ROWS_SENTINEL * 0x0101
    out = torch.full((rows, hid), float("nan"), dtype=torch.float32, device=dev) if want_out else None
    q8 = inv = out16 = None
    if out_kind == PA_OUT_ROW_Q:
        q8 = torch.full((n_el,), PA_ROWS_SENTINEL, dtype=torch.int8, device=dev)
        inv = torch.full((rows,), float("nan"), dtype=torch.float32, device=dev)
    elif out_kind == PA_OUT_ROW_F16 or (out_kind == PA_OUT_OPROJ and rows16):
        out16 = torch.full((n_el,), fill16, dtype=torch.int16, device=dev)
    given = lambda name, t: None if t is None or name in omit else t.data_ptr()
    x = heads = None
    if out_kind == PA_OUT_OPROJ:
        heads = torch.from_numpy(oproj_head_slices(wo, H, D).view("int16")).to(dev)
        cols = heads.shape[2]
        x = torch.full(((rows + 1) * cols * 4,), PA_ROWS_SENTINEL, dtype=torch.uint8,
                       device=dev).view(torch.float32).view(rows + 1, cols)
        if o_acc is None:
            o_acc = torch.zeros(((rows + 1) * cols,), dtype=torch.int64, device=dev)
        if o_flag is None:
            o_flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        a.o_acc, a.o_x, a.wo_heads = o_acc.data_ptr(), x.data_ptr(), heads.data_ptr()
        a.o_n, a.o_flag, a.rows16 = cols if o_n is None else o_n, given("o_flag", o_flag), rows16
    a.has_rows = 1 if has_rows else 0
    a.rows_q, a.inv_scale, a.out16 = given("q", q8), given("inv_scale", inv), given("out16", out16)
    a.pack, a.keep_out, a.out_scale = pack, keep_out, out_scale
    a.out = None if out is None else out.data_ptr()
    status = tune.pa_rows_tune(ctypes.byref(a), stream_ptr(stream))
    if sync:
        torch.cuda.synchronize()
    msg = tune.llm_last_error() if status != LLM_OK else b""
    res = dict(status=status, error=(msg or b"").decode(), out=out, q8=q8, inv_scale=inv,
               out16=out16, nsplit=a.nsplit, form=a.form)
    if out_kind == PA_OUT_OPROJ:
        res.update(x=x, o_acc=o_acc, o_flag=o_flag, wo_heads=heads)  # (wo_heads: kept alive)
    return res


def pack_weights(W, dtype: int, stream=None):
    """Repack a device [K][N] int8 / fp16 weight into MFMA fragment order."""
    import torch
    lib = load()
    K, N = W.shape
    nbytes = lib.gemm_packed_bytes(dtype, K, N)
    P = torch.empty(nbytes, dtype=torch.uint8, device=W.device)
    check(lib.gemm_pack_weights(dtype, ptr(W), ptr(P), K, N, stream_ptr(stream)))
    return P


def i8_gemm(A, W_packed, N, *, sa=None, sw=None, bias=None, act=0, want_acc=True, stream=None):
    import torch
    lib = load()
    M, K = A.shape
    acc = torch.empty((M, N), dtype=torch.int32, device=A.device) if want_acc else None
    C = torch.empty((M, N), dtype=torch.float32, device=A.device)
    check(lib.i8_gemm(ptr(A), A.stride(0), ptr(W_packed), ptr(acc), ptr(C), M, N, K, ptr(sa),
                      ptr(sw), ptr(bias), act, stream_ptr(stream)))
    return acc, C


_ACT_NAMES = {"": LLM_ACT_NONE, "relu": LLM_ACT_RELU, "gelu": LLM_ACT_GELU}


def dnnl_matmul_int8(A, B, C, BATCH, M, N, K, scaleA, scaleB, scaleC=1.0, bias=None,
                     activation="", stream=None) -> bool:
    """dnnl_matmul_int8 (attention_cpu/dnnl_matmul_int8.hpp:5-13) over device tensors:
    A int8 [BATCH][M][K], B int8 [BATCH][K][N], C int8 [BATCH][M][N] (written),
    bias fp32 [N] or None, activation "" / "relu" / "gelu".  Like the reference it
    returns False on any failure (and an unknown activation string is ignored, as
    the reference's post-op chain ignores it, dnnl_matmul_int8.cpp:44-50)."""
    import torch
    lib = load()
    act = _ACT_NAMES.get(activation, LLM_ACT_NONE)
    for t, n in ((A, BATCH * M * K), (B, BATCH * K * N), (C, BATCH * M * N)):
        if t.dtype != torch.int8 or not t.is_contiguous() or t.numel() < n:
            return False
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() < N):
        return False
    return lib.i8_matmul_s8(ptr(A), ptr(B), ptr(C), BATCH, M, N, K, scaleA, scaleB, scaleC,
                            ptr(bias), act, stream_ptr(stream)) == LLM_OK


def f16_gemm(A, W_packed, N, *, bias=None, act=0, stream=None):
    import torch
    lib = load()
    M, K = A.shape
    C = torch.empty((M, N), dtype=torch.float32, device=A.device)
    check(lib.f16_gemm(ptr(A), A.stride(0), ptr(W_packed), ptr(C), M, N, K, ptr(bias), act,
                       stream_ptr(stream)))
    return C


def lm_head(x, E, stream=None):
    import torch
    lib = load()
    M, K = x.shape
    V = E.shape[0]
    out = torch.empty((M, V), dtype=torch.float32, device=x.device)
    check(lib.lm_head(ptr(x), ptr(E), ptr(out), M, V, K, stream_ptr(stream)))
    return out


def lm_head_logprobs(x, E, targets, want_stats=True, stream=None):
    """lm_head_logprobs on torch device tensors: x fp32 [M][K], E fp16 [V][K],
    targets int32 [M] -> (logprob [M], stats [M][3] = {m, lse, x_target} or None)."""
    import torch
    lib = load()
    M, K = x.shape
    V = E.shape[0]
    lp = torch.empty((M,), dtype=torch.float32, device=x.device)
    stats = torch.empty((M, 3), dtype=torch.float32, device=x.device) if want_stats else None
    check(lib.lm_head_logprobs(ptr(x), ptr(E), ptr(targets), ptr(lp), ptr(stats), M, V, K,
                               stream_ptr(stream)))
    return lp, stats


def logprob_rows(logits, chosen=None, top_n=0, want_stats=True, stream=None):
    """logprob_rows on torch device tensors: fp32 logits [R][V], chosen int32 [R]
    or None -> (chosen_lp [R] or None, top_lp [R][top_n], top_id [R][top_n],
    stats [R][2] = {m, lse} or None)."""
    import torch
    lib = load()
    R, V = logits.shape
    dev = logits.device
    clp = torch.empty((R,), dtype=torch.float32, device=dev) if chosen is not None else None
    tlp = torch.empty((R, top_n), dtype=torch.float32, device=dev)
    tid = torch.empty((R, top_n), dtype=torch.int32, device=dev)
    stats = torch.empty((R, 2), dtype=torch.float32, device=dev) if want_stats else None
    check(lib.logprob_rows(ptr(logits), R, V, ptr(chosen), top_n, ptr(clp), ptr(tlp), ptr(tid),
                           ptr(stats), stream_ptr(stream)))
    return clp, tlp, tid, stats


def argmax_rows(logits, stream=None):
    import torch
    lib = load()
    R, V = logits.shape
    out = torch.empty(R, dtype=torch.int32, device=logits.device)
    check(lib.argmax_rows(ptr(logits), R, V, ptr(out), stream_ptr(stream)))
    return out


def sample_rows(logits, temperature=1.0, top_k=0, top_p=1.0, seed=0, counter=0, stream=None):
    """Device sampling of one token per row of fp32 logits [R][V] -> int32 [R]."""
    import torch
    lib = load()
    R, V = logits.shape
    out = torch.empty(R, dtype=torch.int32, device=logits.device)
    check(lib.sample_rows(ptr(logits), R, V, temperature, top_k, top_p, seed, counter, ptr(out),
                          stream_ptr(stream)))
    return out


def sample_rows_each(logits, temperature=None, top_k=None, top_p=None, seed=None, counter=None,
                     stream=None):
    """sample_rows_each on torch device tensors: fp32 logits [R][V] and per-row
    device arrays (temperature / top_p float32, top_k / counter int32, seed
    int64 holding the uint64 bits; None: the entry's default) -> int32 [R]."""
    import torch
    lib = load()
    R, V = logits.shape
    out = torch.empty(R, dtype=torch.int32, device=logits.device)
    check(lib.sample_rows_each(ptr(logits), R, V, ptr(temperature), ptr(top_k), ptr(top_p),
                               ptr(seed), ptr(counter), ptr(out), stream_ptr(stream)))
    return out


SERVE_ADMIT, SERVE_TOKEN, SERVE_MOVE, SERVE_RETIRE = range(4)


def serve_plan_sim(prompt_lens, max_new, gen_lens, *, max_rows, num_pages, pages_per_tile,
                   page_size, window=0, max_seq_len):
    """serve_plan_sim_tune (tuning library): the records (step, kind, id, row,
    aux) of a serving run in which every request is submitted before step 1
    and request i ends after gen_lens[i] tokens; None if a request is refused."""
    tune = load_tune()
    n = len(prompt_lens)
    arr = ctypes.c_int32 * max(n, 1)
    args = (arr(*prompt_lens), arr(*max_new), arr(*gen_lens), n, max_rows, num_pages,
            pages_per_tile, page_size, window, max_seq_len)
    count = tune.serve_plan_sim_tune(*args, None, 0)
    if count == -1:
        return None
    if count == -2 ** 31:
        raise ValueError("serve_plan_sim: bad arguments")
    room = abs(count)
    out = (c_ll * (5 * max(room, 1)))()
    got = tune.serve_plan_sim_tune(*args, out, room)
    assert got == room, (got, room)
    return [tuple(out[5 * i:5 * i + 5]) for i in range(room)]


SERVE_DEFER, SERVE_EVICT, SERVE_PUBLISH, SERVE_STATE_ADMITTED, SERVE_STATE_END = range(4, 9)
PREFIX_STATS = ("positions_due", "positions_hit", "cached_blocks", "idle_pages", "evicted_blocks",
                "deferrals")


def serve_prefix_sim(prompts, max_new, gen_lens, *, max_rows, num_pages, pages_per_tile,
                     page_size, max_seq_len, prefix_cache=True):
    """serve_prefix_sim_tune (tuning library): serve_plan_sim on prompts (lists
    of token ids), with the prefix cache or without.  Returns (records, stats):
    records (step, kind, id, row, aux, aux2) -- see the entry for the kinds --
    and the PREFIX_STATS counters as a dict; None if a request is refused."""
    tune = load_tune()
    n = len(prompts)
    flat = [t for p in prompts for t in p]
    arr = ctypes.c_int32 * max(n, 1)
    args = ((ctypes.c_int32 * max(len(flat), 1))(*flat), arr(*[len(p) for p in prompts]),
            arr(*max_new), arr(*gen_lens), n, max_rows, num_pages, pages_per_tile, page_size,
            max_seq_len, int(prefix_cache))
    count = tune.serve_prefix_sim_tune(*args, None, 0, None)
    if count == -1:
        return None
    if count == -2 ** 31:
        raise ValueError("serve_prefix_sim: bad arguments")
    room = abs(count)
    out = (c_ll * (6 * max(room, 1)))()
    stats = (c_ll * 6)()
    got = tune.serve_prefix_sim_tune(*args, out, room, stats)
    assert got == room, (got, room)
    return ([tuple(out[6 * i:6 * i + 6]) for i in range(room)], dict(zip(PREFIX_STATS, stats)))


def kv_hold_tile(cache, beam, tile, n_pages):
    """kv_cache_hold_tile: the tile's n_pages = L * H page ids, one more
    reference taken on each."""
    pages = (ctypes.c_int32 * n_pages)()
    check(load().kv_cache_hold_tile(cache, beam, tile, pages))
    return list(pages)


def kv_attach_tile(cache, beam, tile, pages):
    """kv_cache_attach_tile: map held pages into an unmapped tile of `beam`."""
    check(load().kv_cache_attach_tile(cache, beam, tile, (ctypes.c_int32 * len(pages))(*pages)))


def kv_drop_pages(cache, pages):
    """kv_cache_drop_pages: give back the references of a hold."""
    check(load().kv_cache_drop_pages(cache, (ctypes.c_int32 * len(pages))(*pages)))


def beam_book(cand_score, cand_parent, cand_token, W, V, max_new, eos_token, length_penalty):
    """beam_book_tune (tuning library): llm_decoder_beam_search's host
    bookkeeping on candidate arrays [steps][num_seqs][2W] (float32, int32,
    int32).  Returns (status, dict) with ids [S][W][max_new], length,
    sum_logprob, score [S][W], live_parent / live_token [steps_run][S][W] and
    steps; the dict is None unless the status is LLM_OK."""
    import numpy as np
    tune = load_tune()
    cs = np.ascontiguousarray(cand_score, np.float32)
    cp = np.ascontiguousarray(cand_parent, np.int32)
    ct = np.ascontiguousarray(cand_token, np.int32)
    steps, S, K = cs.shape
    assert cp.shape == cs.shape == ct.shape
    ids = np.zeros((S, W, max_new), np.int32)
    length = np.zeros((S, W), np.int32)
    sums, score = np.zeros((S, W), np.float32), np.zeros((S, W), np.float32)
    lp = np.zeros((steps, S, W), np.int32)
    lt = np.zeros_like(lp)
    run = np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data_as(c_void_p)
    rc = tune.beam_book_tune(p(cs), p(cp), p(ct), steps, S, W, V, max_new, eos_token,
                             length_penalty, p(ids), p(length), p(sums), p(score), p(lp), p(lt),
                             p(run))
    if rc != LLM_OK:
        return rc, None
    n = int(run[0])
    return rc, dict(ids=ids, length=length, sum_logprob=sums, score=score, live_parent=lp[:n],
                    live_token=lt[:n], steps=n)


def beam_select(logits, score_in, W, stream=None):
    """beam_select_rows on torch device tensors: fp32 logits [num_seqs * W][V] and
    cumulative scores [num_seqs * W] (-inf: beam not live) -> (cand_score fp32,
    cand_parent int32, cand_token int32), each [num_seqs][2W], best first."""
    import torch
    lib = load()
    R, V = logits.shape
    if W < 1 or R % W:
        raise ValueError("beam_select: rows must be num_seqs * W")
    S = R // W
    cs = torch.empty((S, 2 * W), dtype=torch.float32, device=logits.device)
    cp = torch.empty((S, 2 * W), dtype=torch.int32, device=logits.device)
    ct = torch.empty((S, 2 * W), dtype=torch.int32, device=logits.device)
    check(lib.beam_select_rows(ptr(logits), ptr(score_in), S, W, V, ptr(cs), ptr(cp), ptr(ct),
                               stream_ptr(stream)))
    return cs, cp, ct


def kv_cache_reorder(kv_handle, first_beam, parent, n_tokens) -> None:
    """kv_cache_reorder on a kv_cache handle (KVTileCache.handle, decoder.kv_handle)."""
    arr = (ctypes.c_int32 * len(parent))(*parent)
    check(load().kv_cache_reorder(c_void_p(kv_handle), first_beam, len(parent), arr, n_tokens))


def kv_cache_release_before(kv_handle, beam, n_tokens) -> None:
    """kv_cache_release_before on a kv_cache handle: the pages of `beam`'s tiles
    wholly below token n_tokens go back to the pool, their entries read -1."""
    check(load().kv_cache_release_before(c_void_p(kv_handle), beam, n_tokens))


def quantize_rows(x, stream=None):
    import torch
    lib = load()
    R, C = x.shape
    q = torch.empty((R, C), dtype=torch.int8, device=x.device)
    s = torch.empty(R, dtype=torch.float32, device=x.device)
    check(lib.quantize_rows(ptr(x), R, C, ptr(q), ptr(s), stream_ptr(stream)))
    return q, s


def layernorm_quant(x, gamma, beta, eps=1e-5, quant=True, stream=None):
    import torch
    lib = load()
    R, C = x.shape
    out = torch.empty((R, C), dtype=torch.float32, device=x.device)
    q = torch.empty((R, C), dtype=torch.int8, device=x.device) if quant else None
    s = torch.empty(R, dtype=torch.float32, device=x.device) if quant else None
    check(lib.layernorm_quant(ptr(x), R, C, ptr(gamma), ptr(beta), eps, ptr(out), ptr(q), ptr(s),
                              stream_ptr(stream)))
    return out, q, s


def rope_table(theta: float, head_dim: int, num_pos: int):
    """llm_rope_table: float32 [num_pos][head_dim] of (cos, sin) pairs."""
    import numpy as np
    out = np.empty((max(num_pos, 0), max(head_dim, 0)), dtype=np.float32)
    check(load().llm_rope_table(theta, head_dim, num_pos, out.ctypes.data))
    return out
