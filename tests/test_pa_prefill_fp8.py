"""CPU checks of the MFMA prefill's FP8 surface (no device calls): the
workspace sizing of pa_prefill takes LLM_FP8 views exactly as LLM_F16 ones
(the launch plan does not read the element type), still refuses the head dims
and element types it has no kernel for, and the library exports
llm_decoder_prefill_kernel.  Fake views as in tests/test_capi_symbols.py: the
sizing entries read the view's fields and never its pointers."""
import ctypes


def _view(kv_dtype, D=64, H=2, ts=16, max_tiles=40):
    import llm_capi
    return llm_capi.PaKvView(k_pool=1, v_pool=1, page_table=1, num_pages=1, page_size=ts,
                             head_dim=D, num_beams=1, num_heads=H, max_tiles=max_tiles,
                             kv_dtype=kv_dtype)


def test_fp8_workspace_equals_fp16():
    import llm_capi
    lib = llm_capi.load()
    f8, f16 = _view(llm_capi.LLM_FP8), _view(llm_capi.LLM_F16)
    b8 = lib.pa_prefill_workspace_bytes(ctypes.byref(f8), 0, 600)
    b16 = lib.pa_prefill_workspace_bytes(ctypes.byref(f16), 0, 600)
    assert b8 > 0
    assert b8 == b16
    # 600 tokens on 16-token pages: 38 tiles; 10 query blocks x 2 heads ask for
    # 51 splits, the 2-block minimum gives 4 tiles each: 10 splits of (D + 2) floats
    assert b8 == 600 * 2 * 10 * (64 + 2) * 4
    for p0, m in ((0, 1), (7680, 512), (1000, 200), (31, 1)):
        for D, ts in ((64, 16), (128, 16), (128, 32), (64, 32)):
            a = _view(llm_capi.LLM_FP8, D=D, ts=ts, max_tiles=600)
            b = _view(llm_capi.LLM_F16, D=D, ts=ts, max_tiles=600)
            assert (lib.pa_prefill_workspace_bytes(ctypes.byref(a), p0, m) ==
                    lib.pa_prefill_workspace_bytes(ctypes.byref(b), p0, m)), (p0, m, D, ts)


def test_unsupported_views_size_to_zero():
    import llm_capi
    lib = llm_capi.load()
    assert lib.pa_prefill_workspace_bytes(ctypes.byref(_view(llm_capi.LLM_FP8, D=256)), 0, 600) == 0
    assert lib.pa_prefill_workspace_bytes(ctypes.byref(_view(llm_capi.LLM_I8)), 0, 600) == 0
    # and the launch entry refuses them on the host, before any pointer is read
    pf = (ctypes.c_void_p(16), 0, ctypes.c_void_p(16), 0, 0, 0, 8, 1.0, None, 0, None)
    for v in (_view(llm_capi.LLM_FP8, D=256), _view(llm_capi.LLM_FP8, D=32),
              _view(llm_capi.LLM_I8)):
        assert lib.pa_prefill(ctypes.byref(v), *pf) == llm_capi.LLM_ERR_UNSUPPORTED


def test_prefill_kernel_symbol():
    import llm_capi
    lib = llm_capi.load()
    assert hasattr(lib, "llm_decoder_prefill_kernel")
    assert "llm_decoder_prefill_kernel" in llm_capi.declared_symbols()
    assert lib.llm_decoder_prefill_kernel(None) == -1  # NULL: no decoder to ask
