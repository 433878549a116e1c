"""Rotary position embedding through the decoders (llm_decoder_set_rope): the
qkv projection rotates q and K by each row's position before q is stored and
K is rounded into the pages, in decode steps, prompt chunks and packed prefill
passes alike.

At the dims and bars of tests/test_decoder_gpu.py (imported from it: L 2, H 4,
D 64, V 1000; LOGIT_TOL, TIE_TOL, FREE_RUN_TOL, one int8 LSB, 1e-5 on the row
scales, flips below 1e-3 of the values).  The oracle knows no rotation, so the
teacher-forced test feeds it the GPU's rotated K (forced_kv) and holds stages
0, 2, 3 and the logits as that file does; the oracle's own stage-1 figures
(its q is not rotated) are replaced by tests/_rope.py::stage1_stats, which
restates the path from the stage-0 tap to the o_proj input with rope_ref on q,
and which reproduces the oracle's stage-1 figures on a rope-off decoder (the
anchor, run first)."""
import numpy as np
import pytest

from _fp8 import Pages, boundary_sensitive, f16_model, make_decoder, ref_encode
from _rope import KvHistory, identity_table, rope_ref, stage1_stats
from _util import assert_parity, decoder_kv_at, rel_err
from test_decoder_fp8_gpu import BOUNDARY_CAP
from test_decoder_gpu import (FREE_RUN_TOL, LOGIT_TOL, TIE_TOL, _int8_model, _prefill_vs_stepping,
                              _Taps)

pytestmark = pytest.mark.gpu
THETA = 10000.0


def _torch():
    import torch
    return torch


def _table(w):
    import llm_decoder
    c = w["cfg"]
    return llm_decoder.rope_table(THETA, c["D"], c["max_seq"])


def _same_bits(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8),
                                  np.ascontiguousarray(b).view(np.uint8), err_msg=what)


def _forced_rope_steps(dec, oracle, w, prompts, steps, table):
    """GPU (taps on) and the teacher-forced oracle in lockstep, the oracle's
    cache fed the K / V the GPU appended.  table None: a rope-off decoder, on
    which stage1_stats must give the oracle's own stage-1 figures."""
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
        kv = decoder_kv_at(dec, B, pos, L)  # fp16 [L][B][2][H][D]
        hist.append(kv, pos)
        qkv, st1 = stage1_stats(oracle, w, fq, fs, hist, s, table)
        # the appended K is the rotated K, rounded once; V is not rotated
        for l in range(L):
            k = qkv[l, :, hid:2 * hid]
            if table is not None:
                k = rope_ref(k, pos, table)
            _same_bits(kv[l, :, 0].reshape(B, hid), k.astype(np.float16), f"step {s} layer {l} K")
            _same_bits(kv[l, :, 1].reshape(B, hid), qkv[l, :, 2 * hid:].astype(np.float16),
                       f"step {s} layer {l} V")
        o_logits, o_next, stats, _ = odec.step_attn(np.array(tok, np.int32), pos, fq, fs,
                                                    forced_kv=kv)
        if table is None:  # the anchor: the helper restates the oracle's stage 1
            np.testing.assert_array_equal(st1[:, :2], stats[:, 1, :2])
            assert np.max(np.abs(st1[:, 2] - stats[:, 1, 2])) < 1e-7, (st1, stats[:, 1])
            assert odec.kv_stats[:, 0].max() == 0, odec.kv_stats
        stats[:, 1] = st1  # the oracle's own q is not rotated: its stage 1 is replaced
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


def test_int8_teacher_forced_rope(gpu, oracle):
    w = _int8_model(oracle, L=2, H=4, D=64, V=1000, S=64)
    rng = np.random.default_rng(0)
    prompts = [list(rng.integers(0, 1000, n)) for n in (5, 17, 1)]
    # anchor: the helper on a rope-off decoder
    off = make_decoder(w, 3, kv_dtype="float16")
    assert off.rope is False
    _forced_rope_steps(off, oracle, w, prompts, 8, None)
    dec = make_decoder(w, 3, kv_dtype="float16")
    dec.set_rope(theta=THETA)
    assert dec.rope is True
    worst, n_vals, n_flips = _forced_rope_steps(dec, oracle, w, prompts, 40, _table(w))
    assert n_flips < 1e-3 * n_vals, (n_flips, n_vals)
    print(f"rope forced lockstep: worst logit rel err {worst:.2e}, int8 flips {n_flips}/{n_vals}")


def _step_logits(dec, toks, B, V):
    torch = _torch()
    logits = torch.empty((B, V), device="cuda")
    dec.begin_synthetic(B, 0, 0, False)
    out = []
    for tok in toks:
        dec.step(tok, logits_ptr=logits.data_ptr())
        torch.cuda.synchronize()
        out.append(logits.cpu().numpy().copy())
    return out


def test_identity_table_theta_table_and_off(gpu, oracle):
    """An identity table (cos 1, sin 0) computes the rope-off logits (values:
    y * 1 - y1 * 0 can turn an exact -0 into +0); a theta table does not, from
    the second position on; set_rope(None) after a table leaves a decoder that
    computes the rope-off bits; the table is refused while rows are active."""
    w = _int8_model(oracle, L=2, H=4, D=64, V=1000, S=64)
    c = w["cfg"]
    B, V = 3, c["V"]
    rng = np.random.default_rng(2)
    toks = [[int(t) for t in rng.integers(0, V, B)] for _ in range(12)]
    off = _step_logits(make_decoder(w, B, kv_dtype="float16"), toks, B, V)
    ident = make_decoder(w, B, kv_dtype="float16")
    ident.set_rope(table=identity_table(c["max_seq"], c["D"]))
    assert ident.rope is True
    for s, (a, b) in enumerate(zip(_step_logits(ident, toks, B, V), off)):
        assert np.array_equal(a, b), s  # values, not bits
    rot = make_decoder(w, B, kv_dtype="float16")
    rot.set_rope(theta=THETA)
    on = _step_logits(rot, toks, B, V)
    assert np.array_equal(on[0], off[0])  # position 0 is the identity (values)
    diffs = [rel_err(on[s], off[s]) for s in range(1, 12)]
    print("theta table against rope off, per step:", " ".join(f"{d:.2e}" for d in diffs))
    assert all(not np.array_equal(on[s], off[s]) for s in range(1, 12))
    assert max(diffs) > LOGIT_TOL  # more than the parity bar: no rounding effect
    # the table, then no table, before any row: the rope-off bits
    back = make_decoder(w, B, kv_dtype="float16")
    back.set_rope(theta=THETA)
    back.set_rope(None)
    assert back.rope is False
    for s, (a, b) in enumerate(zip(_step_logits(back, toks, B, V), off)):
        _same_bits(a, b, f"step {s}")
    # rows are active now: refused, and the decoder is unchanged
    for d in (back, rot):
        with pytest.raises(RuntimeError, match="rows are active"):
            d.set_rope(theta=THETA)
        with pytest.raises(RuntimeError, match="rows are active"):
            d.set_rope(None)
    assert back.rope is False and rot.rope is True
    # table checks
    fresh = make_decoder(w, B, kv_dtype="float16")
    bad = identity_table(c["max_seq"], c["D"])
    bad[3, 5] = np.inf
    with pytest.raises(RuntimeError, match="finite"):
        fresh.set_rope(table=bad)
    with pytest.raises(ValueError):
        fresh.set_rope(table=bad[:-1])
    assert fresh.rope is False


def test_set_rope_refuses_odd_head_dim(gpu):
    import ctypes
    import llm_capi
    from _fp8 import DecoderConfig
    lib = llm_capi.load()
    cfg = DecoderConfig(num_layers=1, num_heads=64, head_dim=3, hidden_dim=192, vocab_size=100,
                        max_seq_len=8, weight_dtype=llm_capi.LLM_I8, max_batch=1)
    h = ctypes.c_void_p()
    llm_capi.check(lib.llm_decoder_create(ctypes.byref(cfg), ctypes.byref(h)))
    t = np.zeros((8, 3), np.float32)
    assert lib.llm_decoder_rope(h) == 0
    assert lib.llm_decoder_set_rope(h, t.ctypes.data) == llm_capi.LLM_ERR_INVALID
    assert b"even" in lib.llm_last_error()
    assert lib.llm_decoder_set_rope(h, None) == llm_capi.LLM_OK and lib.llm_decoder_rope(h) == 0
    lib.llm_decoder_destroy(h)


def _f16_maker(w):
    return lambda n: _roped(make_decoder(w, n, kv_dtype="float16", cls="CUDADecoder"))


def _roped(dec):
    dec.set_rope(theta=THETA)
    return dec


@pytest.mark.parametrize("D,kernel,S", [(64, "mfma", 700), (256, "decode", 700)])
def test_f16_prefill_matches_stepping_rope(gpu, D, kernel, S):
    """fp16 CUDADecoder, rope on: prompt chunks (MFMA prefill kernel at D 64,
    the decode-kernel fallback at D 256) against feeding the prompt token by
    token, at the bar test_prefill_decode_kernel_fallback holds the two paths
    to each other."""
    rng = np.random.default_rng(4)
    L, H, V = 2, 2, 400
    w = f16_model(rng, L, H, D, V, S)
    prompts = [rng.integers(0, V, 530).tolist(), rng.integers(0, V, 9).tolist()]
    make = _f16_maker(w)
    assert make(1).prefill_kernel == kernel
    la, lb, nxt = _prefill_vs_stepping(make, prompts, V)
    for r in range(2):
        assert rel_err(lb[r], la[r]) < 2 * LOGIT_TOL, (r, rel_err(lb[r], la[r]))
        assert la[r].max() - la[r][nxt[r]] <= 2 * LOGIT_TOL * np.abs(la[r]).max()
    # rotation is on in both paths: the rope-off decoder computes other logits
    off = make_decoder(w, 1, kv_dtype="float16", cls="CUDADecoder")
    lo = _step_logits(off, [[t] for t in prompts[1]], 1, V)[-1][0]
    print(f"rope on against rope off: {rel_err(la[1], lo):.3e}")
    assert rel_err(la[1], lo) > 2 * LOGIT_TOL  # the bar above tells the two apart


def test_f16_packed_prefill_matches_stepping_rope(gpu):
    """prefill_batch (several rows' chunks in one layer pass, each row at its
    own positions) with rope on, against token-by-token stepping."""
    torch = _torch()
    rng = np.random.default_rng(6)
    L, H, D, V, S = 2, 4, 64, 300, 128
    w = f16_model(rng, L, H, D, V, S)
    prompts = [rng.integers(0, V, n).tolist() for n in (70, 9, 33)]
    make = _f16_maker(w)
    b = make(3)
    b.begin_synthetic(3, 0, 0, False)
    b.prefill_batch([0, 1, 2], [p[:-1] for p in prompts])
    lb = torch.empty((3, V), device="cuda")
    b.step([p[-1] for p in prompts], logits_ptr=lb.data_ptr())
    torch.cuda.synchronize()
    lb = lb.cpu().numpy()
    for r, p in enumerate(prompts):
        la = _step_logits(make(1), [[t] for t in p], 1, V)[-1][0]
        assert rel_err(lb[r], la) < 2 * LOGIT_TOL, (r, rel_err(lb[r], la))


def test_int8_prefill_matches_stepping_rope(gpu, oracle):
    """INT8, rope on: chunked prefill against stepping at the free-running bar
    of test_prefill_matches_token_by_token."""
    w = _int8_model(oracle, L=2, H=4, D=64, V=500, S=1024, seed=12)
    V = w["cfg"]["V"]
    rng = np.random.default_rng(3)
    prompts = [rng.integers(0, V, 600).tolist(), rng.integers(0, V, 37).tolist()]
    la, lb, nxt = _prefill_vs_stepping(
        lambda n: _roped(make_decoder(w, n, kv_dtype="float16")), prompts, V)
    for r in range(2):
        err = rel_err(lb[r], la[r])
        gap = float((la[r].max() - la[r][nxt[r]]) / np.abs(la[r]).max())
        print(f"row {r}: prefill vs stepping {err:.3e}, id gap {gap:.3e}")
        assert err < FREE_RUN_TOL, (r, err)
        assert gap <= FREE_RUN_TOL, (r, gap)


def test_fp8_kv_append_bytes_rope(gpu, oracle):
    """FP8-KV INT8 decoder, rope on, scales that are no powers of two for K:
    the appended K bytes are the reference encoding of rope_ref(k) at k_scale
    (a byte may differ only where the reference byte changes within one fp32
    ulp of the pre-image, and such bytes stay under BOUNDARY_CAP); V bytes
    that of the unrotated v."""
    torch = _torch()
    w = _int8_model(oracle, L=2, H=4, D=64, V=1000, S=64)
    c = w["cfg"]
    B, L, H, D, hid, V = 3, c["L"], c["H"], c["D"], c["hid"], c["V"]
    k_scale, v_scale = [0.3, 1.7], [4.0, 0.0625]
    dec = make_decoder(w, B)  # fp8 pools
    dec.set_kv_scales(k_scale, v_scale)
    dec.set_rope(theta=THETA)
    table = _table(w)
    taps, pages = _Taps(dec, w, B), Pages(dec)
    dec.begin_synthetic(B, 0, 0, False)
    logits = torch.empty((B, V), device="cuda")
    rng = np.random.default_rng(8)
    n_bytes = n_boundary = 0
    for s in range(20):
        dec.step([int(t) for t in rng.integers(0, V, B)], logits_ptr=logits.data_ptr())
        torch.cuda.synchronize()
        fq, fs = taps.read(B)
        pos = np.full(B, s, np.int32)
        got = pages.at(pages.pool(), B, pos, L)  # uint8 [L][B][2][H][D]
        for l in range(L):
            y = oracle.i8_gemm(fq[l, 0, :, :hid], w["wqkv"][l], fs[l, 0], w["sw_qkv"][l])[1]
            pre_k = rope_ref(y[:, hid:2 * hid], pos, table).reshape(B, H, D)
            pre_v = y[:, 2 * hid:].reshape(B, H, D)
            for which, pre, sc in ((0, pre_k, k_scale[l]), (1, pre_v, v_scale[l])):
                want = ref_encode(pre, sc)
                g = got[l, :, which]
                diff = g != want
                assert not (diff & ~boundary_sensitive(pre, sc)).any(), (s, l, which)
                n_bytes += g.size
                n_boundary += int(diff.sum())
    assert n_boundary <= BOUNDARY_CAP * n_bytes, (n_boundary, n_bytes)
    assert np.isfinite(logits.cpu().numpy()).all()


@pytest.mark.parametrize("cls", ["INT8Decoder", "CUDADecoder"])
def test_beam_width_one_is_greedy_generate_rope(gpu, oracle, cls):
    w = (_int8_model(oracle, L=2, H=4, D=64, V=300, S=96, seed=21) if cls == "INT8Decoder"
         else f16_model(np.random.default_rng(21), 2, 4, 64, 300, 96))
    dec = _roped(make_decoder(w, 2, kv_dtype="float16", cls=cls))
    prompt = [int(t) for t in np.random.default_rng(5).integers(0, 300, 37)]
    new = 12
    greedy = dec.generate(prompt, new, 1.0)[len(prompt):]
    (ids, score), = dec.beam_search(prompt, beam_width=1, max_new_tokens=new)
    assert ids == greedy
    assert np.isfinite(score) and score < 0
    assert dec.generate(prompt, new, 1.0)[len(prompt):] == greedy
