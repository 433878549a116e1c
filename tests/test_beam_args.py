"""Host-side argument checks of the beam-search entry points: rejected with
LLM_ERR_INVALID before anything touches a device (no GPU needed), and the
plain-Python restatement of the search (tests/_beam.py) on a hand-made case."""
import ctypes

import numpy as np

from _beam import bookkeeping, final_score, select_ref


def test_beam_select_rows_rejections():
    import llm_capi
    lib = llm_capi.load()
    p = ctypes.c_void_p(16)
    call = lambda S, W, V: lib.beam_select_rows(p, p, S, W, V, p, p, p, None)
    assert call(1, 0, 100) == llm_capi.LLM_ERR_INVALID
    assert b"W must be in [1, 4]" in lib.llm_last_error()
    assert call(1, 5, 100) == llm_capi.LLM_ERR_INVALID
    assert call(1, 4, 7) == llm_capi.LLM_ERR_INVALID          # V < 2W
    assert b"V < 2W" in lib.llm_last_error()
    assert call(1, 1, 1) == llm_capi.LLM_ERR_INVALID
    assert call(1, 2, 65537) == llm_capi.LLM_ERR_INVALID      # V > 65536
    assert b"65536" in lib.llm_last_error()
    assert call(-1, 2, 100) == llm_capi.LLM_ERR_INVALID
    assert lib.beam_select_rows(None, p, 1, 2, 100, p, p, p, None) == llm_capi.LLM_ERR_INVALID
    assert call(0, 2, 100) == llm_capi.LLM_OK                 # no rows: a no-op


def test_reorder_and_search_reject_null():
    import llm_capi
    lib = llm_capi.load()
    par = (ctypes.c_int32 * 2)(0, 0)
    assert lib.kv_cache_reorder(None, 0, 2, par, 4) == llm_capi.LLM_ERR_INVALID
    assert lib.kv_cache_cow_copies(None) == -1
    opt = llm_capi.LlmBeamOptions(beam_width=2, max_new_tokens=4, eos_token=-1, length_penalty=1.0)
    assert lib.llm_decoder_beam_search(None, None, None, 0, 1, ctypes.byref(opt), None, None, None,
                                       None) == llm_capi.LLM_ERR_INVALID


def test_reference_bookkeeping_by_hand():
    """W = 2, EOS = 9: step 0 extends beam 0 twice; step 1 finishes one
    hypothesis at rank 0, ignores the EOS at rank 2, and re-parents."""
    cs = np.array([[[-1.0, -2.0, -3.0, -4.0]],
                   [[-1.5, -2.5, -2.75, -5.0]]], np.float32)
    cp = np.array([[[0, 0, 0, 0]], [[1, 0, 0, 1]]], np.int32)
    ct = np.array([[[4, 5, 6, 7]], [[9, 3, 9, 2]]], np.int32)
    r = bookkeeping(cs, cp, ct, W=2, max_new=2, eos_token=9, length_penalty=1.0)
    assert r["live_parent"].tolist() == [[[0, 0]], [[0, 1]]]
    assert r["live_token"].tolist() == [[[4, 5]], [[3, 2]]]
    # pool: finished [5, 9] (-1.5 / 2), live [4, 3] (-2.5 / 2), live [5, 2] (-5 / 2)
    assert r["ids"] == [[[5, 9], [4, 3]]]
    assert r["sum_logprob"].tolist() == [[-1.5, -2.5]] and r["score"].tolist() == [[-0.75, -1.25]]
    r0 = bookkeeping(cs, cp, ct, W=2, max_new=2, eos_token=9, length_penalty=0.0)
    assert r0["score"].tolist() == [[-1.5, -2.5]]
    assert final_score(-3.0, 4, 0.5) == np.float32(-1.5)


def test_reference_selection_order():
    """(score desc, parent asc, token asc) and raw-logit ranking inside a row."""
    lg = np.zeros((2, 6), np.float32)
    lg[:, 4] = 1.0
    s, p, t = select_ref(lg, np.zeros(2, np.float32), 2)
    assert p[0, :4].tolist() == [0, 1, 0, 0] and t[0, :4].tolist() == [4, 4, 0, 1]
    s, p, t = select_ref(lg, np.array([0, -np.inf], np.float32), 2)
    assert p[0, :4].tolist() == [0, 0, 0, 0] and t[0, :4].tolist() == [4, 0, 1, 2]
