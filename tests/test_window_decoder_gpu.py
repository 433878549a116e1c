"""Sliding-window attention through the decoders (llm_decoder_set_window):
every layer's attention at position p reads positions max(0, p - W + 1) .. p
in decode steps, prompt chunks and packed prefill passes, and the pages wholly
below a row's window go back to the pool as the row advances.

Dims and bars are tests/test_decoder_gpu.py's (L <= 2, H 4, D 64, V 1000;
LOGIT_TOL, TIE_TOL, FREE_RUN_TOL, one int8 LSB, 1e-5 on the row scales).  The
oracle knows no window: the one-layer test compares against window-off
decoders fed the window's tokens only, the teacher-forced test replaces the
oracle's stage-1 figures by tests/_window.py::stage1_stats (anchored on a
window-off decoder first, where it must reproduce the oracle's own)."""
import ctypes
import os

import numpy as np
import pytest

from _fp8 import FORM_SPLIT_MERGE_ROW, FORM_WG_MERGE, f16_model, make_decoder
from _rope import KvHistory
from _util import assert_parity, decoder_kv_at, rel_err
from _window import stage1_stats, t_prime
from test_decoder_gpu import (FREE_RUN_TOL, LOGIT_TOL, TIE_TOL, _int8_model, _prefill_vs_stepping,
                              _Taps)
from test_wg_merge_gpu import _Cfg, _F16W, _model

pytestmark = pytest.mark.gpu
FORM_OPROJ = 32  # LLM_PA_FORM_OPROJ (tests/_fp8.py names the forms it uses; not this flag)


def _torch():
    import torch
    return torch


def _windowed(dec, W):
    dec.set_window(W)
    assert dec.window == W
    return dec


def _prefill_then_step(dec, toks, V):
    """Logits of the last token of `toks` after prefilling the others (row 0)."""
    torch = _torch()
    dec.begin_synthetic(1, 0, 0, False)
    if len(toks) > 1:
        dec.prefill(0, [int(t) for t in toks[:-1]])
    lg = torch.empty((1, V), device="cuda")
    dec.step([int(toks[-1])], logits_ptr=lg.data_ptr())
    torch.cuda.synchronize()
    return lg[0].cpu().numpy().copy()


@pytest.mark.parametrize("cls,kv", [("INT8Decoder", "float16"), ("INT8Decoder", "fp8"),
                                    ("CUDADecoder", "float16"), ("CUDADecoder", "fp8")])
def test_one_layer_window_equals_short_history(gpu, oracle, cls, kv):
    """One layer, no rotary table: a token's K / V depend on the token alone, so
    a window-W decoder that consumed tokens[:p + 1] must give the logits of a
    window-off decoder that consumed tokens[p - W + 1 : p + 1] only (both
    prefill, then one step), at p = W - 1, W, W + 1, 2 W + 3, 5 W with W = 8,
    within LOGIT_TOL.  And the test can fail: the window-off decoder fed ONE
    token more (tokens[p - W : p + 1], an off-by-one window) exceeds the bar
    at some checkpoint."""
    W, V, S = 8, 1000, 64
    if cls == "INT8Decoder":
        w = _int8_model(oracle, L=1, H=4, D=64, V=V, S=S, seed=21)
    else:
        w = f16_model(np.random.default_rng(21), 1, 4, 64, V, S)
    toks = np.random.default_rng(8).integers(0, V, 5 * W + 1)
    win = _windowed(make_decoder(w, 1, kv_dtype=kv, cls=cls), W)
    off = make_decoder(w, 1, kv_dtype=kv, cls=cls)
    assert off.window == 0
    worst_off_by_one = 0.0
    for p in (W - 1, W, W + 1, 2 * W + 3, 5 * W):
        got = _prefill_then_step(win, toks[:p + 1], V)
        want = _prefill_then_step(off, toks[max(0, p - W + 1):p + 1], V)
        err = rel_err(got, want)
        print(f"{cls} {kv} p {p}: window vs short history {err:.3e}")
        assert err < LOGIT_TOL, (p, err)
        if p >= W:
            wrong = _prefill_then_step(off, toks[p - W:p + 1], V)
            worst_off_by_one = max(worst_off_by_one, rel_err(got, wrong))
    print(f"{cls} {kv}: one token more differs by {worst_off_by_one:.3e}")
    assert worst_off_by_one > LOGIT_TOL, worst_off_by_one


def test_narrow_window_changes_stepping(gpu):
    """Three rows stepped from position 0 on a one-layer FP16 model, window 8
    against window off: the same logits while the contexts are within the
    window (steps 0 .. 7: the same keys, the same one-split launch), different
    ones from the step that crosses it on, every step."""
    torch = _torch()
    V, B, W = 1000, 3, 8
    wf = f16_model(np.random.default_rng(21), 1, 4, 64, V, 64)

    def run(window):
        dec = _windowed(make_decoder(wf, B, kv_dtype="float16", cls="CUDADecoder"), window)
        dec.begin_synthetic(B, 0, 0, False)
        lg = torch.empty((B, V), device="cuda")
        rng = np.random.default_rng(2)
        out = []
        for _ in range(30):
            dec.step([int(t) for t in rng.integers(0, V, B)], logits_ptr=lg.data_ptr())
            torch.cuda.synchronize()
            out.append(lg.cpu().numpy().copy())
        return np.stack(out)

    off, win = run(0), run(W)
    np.testing.assert_array_equal(win[:W], off[:W])
    diffs = [rel_err(win[s], off[s]) for s in range(W, 30)]
    print("window 8 against off, steps 8 ..:", " ".join(f"{d:.1e}" for d in diffs))
    assert min(diffs) > LOGIT_TOL, diffs


def _forced_window_steps(dec, oracle, w, prompts, steps, W, table=None, attn_scale=1.0):
    """tests/test_rope_decoder_gpu.py::_forced_rope_steps with the window in
    the stage-1 restatement: GPU (taps on) and the teacher-forced oracle in
    lockstep, the oracle's cache fed the K / V the GPU appended.  W = 0: a
    window-off decoder, on which stage1_stats must give the oracle's own
    stage-1 figures (table None only: the oracle does not rotate)."""
    from oracle.oracle import OracleDecoder
    torch = _torch()
    c = w["cfg"]
    B, L, H, D, hid, V = len(prompts), c["L"], c["H"], c["D"], c["hid"], c["V"]
    odec = OracleDecoder(oracle, w, B)
    taps = _Taps(dec, w, B)
    hist = KvHistory(L, B, H, D, c["max_seq"])
    dec.begin_synthetic(B, 0, 0, False)
    logits = torch.empty((B, V), device="cuda")
    nxt = [0] * B
    worst, n_vals, n_flips = 0.0, 0, 0
    for s in range(steps):
        tok = [int(p[s]) if s < len(p) else int(nxt[b]) for b, p in enumerate(prompts)]
        pos = np.full(B, s, np.int32)
        g_next = dec.step(tok, logits_ptr=logits.data_ptr())
        torch.cuda.synchronize()
        fq, fs = taps.read(B)
        kv = decoder_kv_at(dec, B, pos, L)
        hist.append(kv, pos)
        _, st1 = stage1_stats(oracle, w, fq, fs, hist, s, W, table, attn_scale)
        o_logits, o_next, stats, _ = odec.step_attn(np.array(tok, np.int32), pos, fq, fs,
                                                    attn_scale=attn_scale, forced_kv=kv)
        if W == 0 and table is None:  # the anchor
            np.testing.assert_array_equal(st1[:, :2], stats[:, 1, :2])
            assert np.max(np.abs(st1[:, 2] - stats[:, 1, 2])) < 1e-7, (st1, stats[:, 1])
        stats[:, 1] = st1  # the oracle attends to the whole history: its stage 1 is replaced
        gl = logits.cpu().numpy()
        err = rel_err(gl, o_logits)
        assert err < LOGIT_TOL, (s, err)
        assert_parity(gl, o_logits, LOGIT_TOL, axis=1, what=f"step {s} logits")
        worst = max(worst, err)
        assert stats[:, :, 1].max() <= 1, (s, stats)    # at most one int8 LSB
        assert stats[:, :, 2].max() < 1e-5, (s, stats)  # row scales agree
        n_flips += int(stats[:, :, 0].sum())
        n_vals += B * L * (3 * hid + c["inter"])
        for b in range(B):
            if g_next[b] != o_next[b]:
                gap = o_logits[b][o_next[b]] - o_logits[b][g_next[b]]
                assert gap <= TIE_TOL * np.abs(o_logits[b]).max(), (s, b, gap)
        nxt = list(g_next)
    dec.set_taps(0, 0)
    return worst, n_vals, n_flips


@pytest.mark.parametrize("rope", [False, True])
def test_int8_teacher_forced_window(gpu, oracle, rope, scale=1.0):
    import llm_decoder
    W = 20
    w = _int8_model(oracle, L=2, H=4, D=64, V=1000, S=64)
    rng = np.random.default_rng(0)
    prompts = [list(rng.integers(0, 1000, n)) for n in (5, 17, 1)]
    table = None
    if not rope:  # anchor: the helper on a window-off decoder
        _forced_window_steps(make_decoder(w, 3, kv_dtype="float16", attn_scale=scale), oracle, w,
                             prompts, 8, 0, attn_scale=scale)
    dec = _windowed(make_decoder(w, 3, kv_dtype="float16", attn_scale=scale), W)
    if rope:
        dec.set_rope(theta=10000.0)
        table = llm_decoder.rope_table(10000.0, 64, 64)
    worst, n_vals, n_flips = _forced_window_steps(dec, oracle, w, prompts, 48, W, table, scale)
    assert n_flips < 1e-3 * n_vals, (n_flips, n_vals)
    print(f"window forced lockstep (rope {rope}, attn_scale {scale}): worst logit rel err {worst:.2e}, "
          f"int8 flips {n_flips}/{n_vals}")


# --------------------------------------------------------------------------
# launch forms of a windowed FP16 decoder, through the tuning library
# --------------------------------------------------------------------------
def _run_window(lib, w, L, H, D, V, S, B, ctx, steps, W, wgm=True, splits=0, fuse=True):
    """test_wg_merge_gpu.py::_run on a decoder with window W: (logits of `steps`
    steps, llm_decoder_attention_plan before the first step)."""
    import llm_capi
    torch = _torch()
    os.environ["LLM_WG_MERGE"] = "1" if wgm else "0"
    os.environ["LLM_WGM_SPLITS"] = str(splits)
    os.environ["LLM_OPROJ_FUSE"] = "1" if fuse else "0"
    vp, ip = ctypes.c_void_p, ctypes.c_int
    for name, args in (("llm_decoder_create", [ctypes.POINTER(_Cfg), ctypes.POINTER(vp)]),
                       ("llm_decoder_set_f16_weights", [vp, ctypes.POINTER(_F16W)]),
                       ("llm_decoder_begin_synthetic", [vp, ip, ip, ctypes.c_uint64, ip]),
                       ("llm_decoder_step", [vp] * 5), ("llm_decoder_sync", [vp]),
                       ("llm_decoder_set_window", [vp, ip]), ("llm_decoder_window", [vp]),
                       ("llm_decoder_attention_plan", [vp, ctypes.POINTER(ip), ctypes.POINTER(ip)]),
                       ("llm_decoder_destroy", [vp])):
        getattr(lib, name).argtypes = args
    lib.llm_decoder_destroy.restype = None
    cfg = _Cfg(L, H, D, H * D, V, S, 0, 16, llm_capi.LLM_F16, B, 1.0, 0)
    dec = vp()
    llm_capi.check(lib.llm_decoder_create(ctypes.byref(cfg), ctypes.byref(dec)), lib)
    try:
        ww = _F16W(*[w[k].ctypes.data for k in ("emb", "ln1_g", "ln1_b", "ln2_g", "ln2_b", "wqkv",
                                                 "wo", "w1", "w2", "b1", "b2")])
        llm_capi.check(lib.llm_decoder_set_f16_weights(dec, ctypes.byref(ww)), lib)
        llm_capi.check(lib.llm_decoder_set_window(dec, W), lib)
        assert lib.llm_decoder_window(dec) == W
        llm_capi.check(lib.llm_decoder_begin_synthetic(dec, B, ctx, 77, 1), lib)
        ns, form = ip(-1), ip(-1)
        llm_capi.check(lib.llm_decoder_attention_plan(dec, ctypes.byref(ns), ctypes.byref(form)), lib)
        rng = np.random.default_rng(5)
        out = []
        logits = torch.empty((B, V), device="cuda")
        for _ in range(steps):
            tok = rng.integers(0, V, B).astype(np.int32)
            llm_capi.check(lib.llm_decoder_step(dec, tok.ctypes.data, logits.data_ptr(), None, None),
                           lib)
            llm_capi.check(lib.llm_decoder_sync(dec), lib)
            out.append(logits.cpu().numpy().copy())
        return np.stack(out), (ns.value, form.value)
    finally:
        lib.llm_decoder_destroy(dec)
        for k in ("LLM_WG_MERGE", "LLM_WGM_SPLITS", "LLM_OPROJ_FUSE"):
            os.environ.pop(k, None)


def test_windowed_launch_forms_agree(gpu):
    """A windowed FP16 decoder at context 1500, W = 700: the workgroup merge
    against split + merge-row at forced splits 3 and 8 (same bits), the fused
    o_proj against the o_proj GEMM (test_wg_merge_gpu.py::test_fused_oproj's
    1e-3 on step 0), the product library against the tuning library at its own
    plan (same bits), and llm_decoder_attention_plan = the plan of T'."""
    import llm_capi
    tune, prod = llm_capi.load_tune(), llm_capi.load()
    L, H, D, V, S, B, ctx, W = 2, 12, 64, 512, 2100, 16, 1500, 700
    w = _model(np.random.default_rng(3), L, H, D, V)
    bits = lambda a: a.view(np.uint32)
    for ns in (3, 8):
        on, plan_on = _run_window(tune, w, L, H, D, V, S, B, ctx, 3, W, True, ns, fuse=False)
        off, plan_off = _run_window(tune, w, L, H, D, V, S, B, ctx, 3, W, False, ns, fuse=False)
        assert np.isfinite(on).all()
        assert plan_on == (ns, FORM_WG_MERGE) and plan_off == (ns, FORM_SPLIT_MERGE_ROW)
        assert np.array_equal(bits(on), bits(off)), (ns, np.abs(on - off).max())
        fused, plan_f = _run_window(tune, w, L, H, D, V, S, B, ctx, 3, W, True, ns, fuse=True)
        assert plan_f == (ns, FORM_WG_MERGE | FORM_OPROJ)
        assert rel_err(fused[0], on[0]) < 1e-3, (ns, rel_err(fused[0], on[0]))
        assert not np.array_equal(bits(fused), bits(on))  # the fused form ran
    auto, plan_t = _run_window(tune, w, L, H, D, V, S, B, ctx, 3, W)
    mine, plan_p = _run_window(prod, w, L, H, D, V, S, B, ctx, 3, W)
    assert plan_p == plan_t
    assert np.array_equal(bits(mine), bits(auto))
    # the window-off decoder whose max_seq_len is T' plans what the windowed one plans
    _, plan_short = _run_window(prod, w, L, H, D, V, t_prime(S, W, 16), B, 40, 1, 0)
    assert plan_p == plan_short, (plan_p, plan_short)
    # and the window changes the result (700 of 1500 tokens attended)
    full, plan_full = _run_window(prod, w, L, H, D, V, S, B, ctx, 1, 0)
    assert rel_err(mine[0], full[0]) > 1e-3


# --------------------------------------------------------------------------
# prefill against stepping
# --------------------------------------------------------------------------
def _gap(la, nxt):
    return float((la.max() - la[nxt]) / np.abs(la).max())


def test_windowed_prefill_matches_stepping_fp16(gpu):
    """A 600-token prompt at W = 100 (the second chunk starts beyond the
    window) and two shorter ones, on the FP16 CUDADecoder (no int8 rounding:
    1e-3, as test_prefill_mfma_fp16_decoder): per-row prefill and the packed
    pass of the three ragged rows against token-by-token stepping, and
    generate_batch's ids (both prefill modes) against stepping's."""
    torch = _torch()
    rng = np.random.default_rng(4)
    L, H, D, V, S, W = 2, 4, 64, 300, 700, 100
    w = f16_model(rng, L, H, D, V, S)
    make = lambda n: _windowed(make_decoder(w, n, kv_dtype="float16", cls="CUDADecoder"), W)
    assert make(1).prefill_kernel == "mfma"
    prompts = [rng.integers(0, V, n).tolist() for n in (600, 37, 230)]
    la, lb, nxt = _prefill_vs_stepping(make, prompts, V)
    for r in range(3):
        err = rel_err(lb[r], la[r])
        print(f"row {r} ({len(prompts[r])} tokens): per-row prefill vs stepping {err:.3e}")
        assert err < 1e-3, (r, err)
        assert _gap(la[r], nxt[r]) <= 1e-3
    # the packed pass
    pk = make(3)
    pk.begin_synthetic(3, 0, 0, False)
    pk.prefill_batch([0, 1, 2], [p[:-1] for p in prompts])
    lp = torch.empty((3, V), device="cuda")
    nxp = pk.step([p[-1] for p in prompts], logits_ptr=lp.data_ptr(), want_next=True)
    torch.cuda.synchronize()
    lp = lp.cpu().numpy()
    for r in range(3):
        err = rel_err(lp[r], la[r])
        print(f"row {r}: packed prefill vs stepping {err:.3e}")
        assert err < 1e-3, (r, err)
        assert _gap(la[r], nxp[r]) <= 1e-3
    # the window matters here: the window-off decoder's logits differ
    off = make_decoder(w, 1, kv_dtype="float16", cls="CUDADecoder")
    off.begin_synthetic(1, 0, 0, False)
    off.prefill(0, prompts[0][:-1])
    lo = torch.empty((1, V), device="cuda")
    off.step([prompts[0][-1]], logits_ptr=lo.data_ptr())
    torch.cuda.synchronize()
    assert rel_err(lo[0].cpu().numpy(), la[0]) > 1e-3
    # generate_batch: greedy ids of stepping the prompts and then the ids fed back
    n_new = 6
    short = [prompts[1], prompts[2][:150]]
    ids, logs = [[], []], [[], []]
    for r, p in enumerate(short):  # rows in their own decoders: ragged prompts
        one = make(1)
        one.begin_synthetic(1, 0, 0, False)
        l1 = torch.empty((1, V), device="cuda")
        tok = None
        for t in p:
            tok = one.step([t], logits_ptr=l1.data_ptr(), want_next=True)[0]
        for _ in range(n_new):
            torch.cuda.synchronize()
            logs[r].append(l1[0].cpu().numpy().copy())
            ids[r].append(int(tok))
            tok = one.step([tok], logits_ptr=l1.data_ptr(), want_next=True)[0]
    for packed in (False, True):
        g = make(2)
        g.packed_prefill = packed
        out = g.generate_batch(short, n_new)
        for r, p in enumerate(short):
            assert out[r][:len(p)] == p
            for i, (a, b) in enumerate(zip(out[r][len(p):], ids[r])):
                if a != b:  # a near tie ends the comparison of the row
                    assert logs[r][i][b] - logs[r][i][a] <= 1e-3 * np.abs(logs[r][i]).max(), (r, i)
                    break


def test_windowed_prefill_decode_kernel_and_int8(gpu, oracle):
    """D = 256 prefills through the decode kernel, which takes the window from
    the same launch (FP16 decoder, twice LOGIT_TOL between the two paths as
    test_prefill_decode_kernel_fallback); the INT8 decoder's MFMA prefill at
    its free-running bar."""
    import llm_decoder
    rng = np.random.default_rng(4)
    L, H, D, V, S, W = 2, 2, 256, 400, 700, 100
    wf = f16_model(rng, L, H, D, V, S)
    make_f16 = lambda n: _windowed(make_decoder(wf, n, kv_dtype="float16", cls="CUDADecoder"), W)
    assert make_f16(1).prefill_kernel == "decode"
    prompts = [rng.integers(0, V, 600).tolist(), rng.integers(0, V, 9).tolist()]
    la, lb, nxt = _prefill_vs_stepping(make_f16, prompts, V)
    for r in range(2):
        err = rel_err(lb[r], la[r])
        print(f"D 256 row {r}: prefill vs stepping {err:.3e}")
        assert err < 2 * LOGIT_TOL, (r, err)
        assert _gap(la[r], nxt[r]) <= LOGIT_TOL
    w = _int8_model(oracle, L=2, H=4, D=64, V=500, S=1024, seed=12)
    make_i8 = lambda n: _windowed(make_decoder(w, n, kv_dtype="float16"), W)
    prompts = [rng.integers(0, 500, 600).tolist(), rng.integers(0, 500, 37).tolist()]
    la, lb, nxt = _prefill_vs_stepping(make_i8, prompts, 500)
    for r in range(2):
        err = rel_err(lb[r], la[r])
        print(f"INT8 row {r}: prefill vs stepping {err:.3e}, id gap {_gap(la[r], nxt[r]):.3e}")
        assert err < FREE_RUN_TOL, (r, err)
        assert _gap(la[r], nxt[r]) <= FREE_RUN_TOL


# --------------------------------------------------------------------------
# page release
# --------------------------------------------------------------------------
def test_bounded_pool_carries_rows_to_max_seq_len(gpu, oracle):
    """max_seq_len 2048, W = 64, 2 rows, a pool of ceil((W + 512) / 16) + 2 tiles
    per (row, layer, head): a 600-token prefill and stepping to position 2047
    never run out of pages, and the pages in use while stepping stay within
    ceil(W / 16) + 1 tiles per (row, layer, head) -- a window of W tokens
    touches no more, and everything below it was released.  The same pool
    without a window runs out."""
    import llm_capi
    lib = llm_capi.load()
    S, W, B, L, H, ts = 2048, 64, 2, 2, 4, 16
    per = (W + 512 + ts - 1) // ts + 2
    pages = per * B * L * H
    w = _int8_model(oracle, L=L, H=H, D=64, V=500, S=S, seed=12)
    rng = np.random.default_rng(6)
    prompt = [rng.integers(0, 500, 600).tolist() for _ in range(B)]
    dec = _windowed(make_decoder(w, B, kv_dtype="float16", num_pages=pages), W)
    kvh = ctypes.c_void_p(dec.kv_handle)
    assert lib.kv_cache_num_pages(kvh) == pages
    dec.begin_synthetic(B, 0, 0, False)
    # after a prompt of n tokens a row holds the tiles from the one with its last
    # pass's first visible token (p0 - W + 1, p0 = the last 512-token chunk's
    # start) to the one with token n - 1, in every layer and head
    n = len(prompt[0])
    p0 = (n - 1) // 512 * 512
    row_pages = ((n + ts - 1) // ts - max(0, p0 - W + 1) // ts) * L * H
    for r in range(B):
        dec.prefill(r, prompt[r])
        assert lib.kv_cache_free_pages(kvh) == pages - (r + 1) * row_pages
    live_bound = ((W + ts - 1) // ts + 1) * B * L * H
    tok = [1, 2]
    low = pages
    for pos in range(600, S):
        tok = dec.step(tok, want_next=True)
        low = min(low, lib.kv_cache_free_pages(kvh))
    assert dec.context_len(0) == S and dec.context_len(1) == S
    print(f"pool {pages} pages, fewest free while stepping {low}, bound {pages - live_bound}")
    assert low >= pages - live_bound, (low, pages, live_bound)
    with pytest.raises(RuntimeError, match="max_seq_len"):
        dec.step(tok)
    lo_tile = (S - W) // ts  # the last step attended to tokens S - W .. S - 1
    for l in range(L):
        for r in range(B):
            for h in range(H):
                ent = [lib.kv_cache_lookup(kvh, l, r, h, t) for t in range(S // ts)]
                assert all(e == -1 for e in ent[:lo_tile]), (l, r, h)
                assert all(e >= 0 for e in ent[lo_tile:]), (l, r, h)
    # no window: the prefill fills the pool and the steps run out of pages
    off = make_decoder(w, B, kv_dtype="float16", num_pages=pages)
    off.begin_synthetic(B, 0, 0, False)
    with pytest.raises(RuntimeError, match="exhausted"):
        for r in range(B):
            off.prefill(r, prompt[r])
        tok = [1, 2]
        for pos in range(600, 700):
            tok = off.step(tok, want_next=True)


# --------------------------------------------------------------------------
# refusals and state
# --------------------------------------------------------------------------
def test_window_refusals_and_state(gpu, oracle):
    import llm_capi
    from llm_capi import LlmBeamOptions
    torch = _torch()
    lib = llm_capi.load()
    w = _int8_model(oracle, L=2, H=4, D=64, V=1000, S=64)
    V = 1000
    toks = [[int(t) for t in np.random.default_rng(2).integers(0, V, 3)] for _ in range(30)]

    def run(dec):
        dec.begin_synthetic(3, 0, 0, False)
        plan = dec.attention_plan()
        lg = torch.empty((3, V), device="cuda")
        out = []
        for tok in toks:
            dec.step(tok, logits_ptr=lg.data_ptr())
            torch.cuda.synchronize()
            out.append(lg.cpu().numpy().copy())
        return plan, np.stack(out)

    fresh_plan, fresh = run(make_decoder(w, 3, kv_dtype="float16"))
    back = make_decoder(w, 3, kv_dtype="float16")
    back.set_window(8)
    with pytest.raises(RuntimeError, match="window must be >= 0"):
        back.set_window(-1)
    assert back.window == 8
    back.set_window(0)  # before any row: today's launches again
    back_plan, back_logits = run(back)
    assert back_plan == fresh_plan
    np.testing.assert_array_equal(back_logits.view(np.uint32), fresh.view(np.uint32))
    # a window wider than the rows ever get computes the window-off bits, and a
    # narrow one the same keys while the contexts are within it (that a window
    # changes the result is test_windowed_prefill_matches_stepping_fp16's and
    # test_windowed_launch_forms_agree's to show: this model's logits barely
    # move with its attention rows)
    wide = _windowed(make_decoder(w, 3, kv_dtype="float16"), 64)
    np.testing.assert_array_equal(run(wide)[1].view(np.uint32), fresh.view(np.uint32))
    narrow = _windowed(make_decoder(w, 3, kv_dtype="float16"), 8)
    _, nl = run(narrow)
    assert rel_err(nl[:8], fresh[:8]) < LOGIT_TOL  # contexts <= W: the same keys
    # rows are active: refused, unchanged
    for d, was in ((narrow, 8), (back, 0)):
        with pytest.raises(RuntimeError, match="rows are active"):
            d.set_window(16)
        assert d.window == was
    # beam entries on a windowed decoder: unsupported, nothing moved, no page taken
    wd = _windowed(make_decoder(w, 4, kv_dtype="float16"), 8)
    kvh = ctypes.c_void_p(wd.kv_handle)
    free = lib.kv_cache_free_pages(kvh)
    with pytest.raises(RuntimeError, match="sliding window"):
        wd.begin_beams(1, 2, 8, 4, 0, False)
    with pytest.raises(RuntimeError, match="sliding window"):
        wd.beam_search([1, 2, 3], beam_width=1, max_new_tokens=3)
    with pytest.raises(RuntimeError, match="sliding window"):
        wd.beam_search_batch([[1, 2, 3], [4, 5]], beam_width=2, max_new_tokens=3)
    assert lib.kv_cache_free_pages(kvh) == free and wd.context_len(0) < 0
    # the status codes, through the C ABI
    cfg = _Cfg(1, 4, 64, 256, 100, 32, 0, 16, llm_capi.LLM_I8, 2, 1.0, 0)
    lib.llm_decoder_create.argtypes = [ctypes.POINTER(_Cfg), ctypes.POINTER(ctypes.c_void_p)]
    h = ctypes.c_void_p()
    llm_capi.check(lib.llm_decoder_create(ctypes.byref(cfg), ctypes.byref(h)))
    try:
        assert lib.llm_decoder_window(h) == 0
        assert lib.llm_decoder_set_window(h, -2) == llm_capi.LLM_ERR_INVALID
        assert lib.llm_decoder_set_window(h, 4) == llm_capi.LLM_OK and lib.llm_decoder_window(h) == 4
        lib.llm_decoder_begin_beams.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [
            ctypes.c_uint64, ctypes.c_int]
        assert lib.llm_decoder_begin_beams(h, 1, 1, 4, 4, 0, 0) == llm_capi.LLM_ERR_UNSUPPORTED
        prompts = (ctypes.c_int32 * 2)(1, 2)
        lens = (ctypes.c_int32 * 1)(2)
        opt = LlmBeamOptions(beam_width=1, max_new_tokens=2, eos_token=-1, length_penalty=0.0)
        ids, n = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 2)()
        lp, sc = (ctypes.c_float * 2)(), (ctypes.c_float * 2)()
        assert lib.llm_decoder_beam_search(h, prompts, lens, 2, 1, ctypes.byref(opt), ids, n, lp,
                                           sc) == llm_capi.LLM_ERR_UNSUPPORTED
        assert lib.llm_decoder_set_window(h, 0) == llm_capi.LLM_OK
        assert lib.llm_decoder_begin_beams(h, 1, 1, 4, 4, 0, 0) == llm_capi.LLM_OK
        assert lib.llm_decoder_set_window(h, 4) == llm_capi.LLM_ERR_INVALID  # rows are active
        assert lib.llm_decoder_window(h) == 0
    finally:
        lib.llm_decoder_destroy(h)
