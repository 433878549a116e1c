"""Sliding-window attention, the host side: the planner under a window, the
exported entries and the refusals that need no device.

The planner sizes a windowed launch's splits for the tiles a window can touch,
ceil(W / TS) + 1, so its plan is the window-off plan of a context of that many
tiles: pa_plan_window_tune(T, W) == pa_plan_tune(T'), T' = min(T, (ceil(W / TS)
+ 1) * TS), with the resident-wave counts the planner falls back to without a
device (test_pa_plan.py's)."""
import ctypes
import itertools

import pytest

import llm_capi
from _window import t_prime
from test_pa_plan import CPU_BEAM_RESIDENT, CPU_RESIDENT, KINDS

NEW_ENTRIES = ["pa_decode_window", "pa_decode_window_plan", "pa_prefill_window",
               "pa_prefill_packed_window", "kv_cache_release_before", "llm_decoder_set_window",
               "llm_decoder_window"]


def _plan(tune, B, H, D, T, ts, max_tiles, kind, *, W=None, rg=1, pps=0, kvt=llm_capi.LLM_F16):
    out, rows16 = KINDS[kind]
    ns, form = ctypes.c_int32(-1), ctypes.c_int32(-1)
    tail = (out, rows16, CPU_RESIDENT, CPU_BEAM_RESIDENT, 0, ctypes.byref(ns), ctypes.byref(form))
    if W is None:
        rc = tune.pa_plan_tune(B, H, D, T, ts, max_tiles, kvt, pps, rg, *tail)
    else:
        rc = tune.pa_plan_window_tune(B, H, D, T, ts, max_tiles, kvt, pps, rg, W, *tail)
    return rc, ns.value, form.value


GRID = list(itertools.product([1, 5, 64], [4, 16], [64, 128], [16, 32], [40, 1500, 8192]))


@pytest.mark.parametrize("kind", ["f32", "row_q", "row_f16", "f32_rows", "oproj"])
def test_window_plan_is_the_plan_of_the_window_tiles(kind):
    tune = llm_capi.load_tune()
    for B, H, D, ts, T in GRID:
        mt = (T + ts - 1) // ts
        off = _plan(tune, B, H, D, T, ts, mt, kind)
        assert off[0] == llm_capi.LLM_OK
        # W = 0 is the window-off plan itself
        assert _plan(tune, B, H, D, T, ts, mt, kind, W=0) == off
        for W in (1, 16, 17, 700, 4096, 10000):
            want = _plan(tune, B, H, D, t_prime(T, W, ts), ts, mt, kind)
            got = _plan(tune, B, H, D, T, ts, mt, kind, W=W)
            assert got == want, (B, H, D, ts, T, W, got, want)
            if W >= T:
                assert got == off
            # fixed pages_per_split: the split count follows the window's tiles too
            assert (_plan(tune, B, H, D, T, ts, mt, kind, W=W, pps=8) ==
                    _plan(tune, B, H, D, t_prime(T, W, ts), ts, mt, kind, pps=8))


def test_window_with_row_groups_is_unsupported():
    tune = llm_capi.load_tune()
    for rg in (2, 4):
        rc, ns, form = _plan(tune, 8, 4, 64, 1500, 16, 94, "f32", W=100, rg=rg)
        assert rc == llm_capi.LLM_ERR_UNSUPPORTED and ns == 0
        assert b"window" in tune.llm_last_error()
        assert _plan(tune, 8, 4, 64, 1500, 16, 94, "f32", W=0, rg=rg)[0] == llm_capi.LLM_OK
    assert _plan(tune, 8, 4, 64, 1500, 16, 94, "f32", W=-1)[0] == llm_capi.LLM_ERR_INVALID


def test_library_exports_the_window_entries():
    lib = llm_capi.load()
    declared = llm_capi.declared_symbols()
    for name in NEW_ENTRIES:
        assert name in declared, f"{name} is not declared in include/llm_decoder.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in llm_capi._SIGS
    assert lib.llm_abi_version() == 3
    assert hasattr(llm_capi.load_tune(), "pa_plan_window_tune")
    import llm_decoder
    for cls in (llm_decoder.CUDADecoder, llm_decoder.INT8Decoder):
        assert hasattr(cls, "set_window") and hasattr(cls, "window")
    assert hasattr(llm_decoder.KVTileCache, "release_before")
    assert hasattr(llm_decoder.PageTable, "release_before")


def test_invalid_window_arguments_are_refused_on_the_host():
    """Fake pointers: every call here returns before anything is dereferenced or
    launched (as test_capi_symbols.py's refusals)."""
    lib = llm_capi.load()
    fake = llm_capi.PaKvView(k_pool=1, v_pool=1, page_table=1, num_pages=1, page_size=16,
                             head_dim=64, num_beams=1, num_heads=1, max_tiles=4,
                             kv_dtype=llm_capi.LLM_F16)
    p1 = ctypes.c_void_p(16)
    dec = (p1, p1, None, None, 1, 1, 64, 16, 1.0, 0)
    assert lib.pa_decode_window(ctypes.byref(fake), *dec, -1, None, 0, None) == llm_capi.LLM_ERR_INVALID
    assert b"window" in lib.llm_last_error()
    assert lib.pa_decode_window(None, *dec, 4, None, 0, None) == llm_capi.LLM_ERR_INVALID
    ns, form = ctypes.c_int32(-1), ctypes.c_int32(-1)
    assert lib.pa_decode_window_plan(ctypes.byref(fake), 1, 1, 64, 16, 0, -5, ctypes.byref(ns),
                                     ctypes.byref(form)) == llm_capi.LLM_ERR_INVALID
    assert ns.value == 0
    # a plan needs no device when the splits are fixed: W = 20 touches <= 3 tiles
    assert lib.pa_decode_window_plan(ctypes.byref(fake), 1, 1, 64, 64, 1, 20, ctypes.byref(ns),
                                     ctypes.byref(form)) == llm_capi.LLM_OK
    assert ns.value == 3
    # B = 0 is a successful no-op, as pa_decode's
    assert lib.pa_decode_window(ctypes.byref(fake), None, None, None, None, 0, 1, 64, 16, 1.0, 0,
                                4, None, 0, None) == llm_capi.LLM_OK
    pf = (p1, 0, p1, 0, 0, 0, 8, 1.0)
    assert lib.pa_prefill_window(ctypes.byref(fake), *pf, -1, None, 0, None) == llm_capi.LLM_ERR_INVALID
    assert b"window" in lib.llm_last_error()
    assert lib.pa_prefill_window(ctypes.byref(fake), p1, 0, None, 0, 0, 0, 8, 1.0, 4, None, 0,
                                 None) == llm_capi.LLM_ERR_INVALID  # out is NULL
    seg = llm_capi.prefill_segs([(0, 0, 8)])
    ws = ctypes.c_void_p(16)
    assert lib.pa_prefill_packed_window(ctypes.byref(fake), p1, 0, p1, 0, seg, 1, 1.0, -1, ws,
                                        1 << 20, None) == llm_capi.LLM_ERR_INVALID
    assert b"window" in lib.llm_last_error()
    assert lib.kv_cache_release_before(None, 0, 16) == llm_capi.LLM_ERR_INVALID
    assert lib.llm_decoder_set_window(None, 4) == llm_capi.LLM_ERR_INVALID
    assert lib.llm_decoder_window(None) == -1
