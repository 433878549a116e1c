"""The decoder with an FP8 (OCP e4m3fn) KV cache (kv_dtype="fp8"): the qkv
projection appends e4m3 bytes at the layer's scales, the attention reads them
(k_scale folded into the score multiplier, v_scale applied to the normalised
heads), through every launch form the step takes.

The oracle keeps fp16 KV.  decode(byte) * scale is an fp16 value exactly for
power-of-two scales in [2^-4, 2^2] (448 * 4 < 65504, 2^-9 * 2^-4 = 2^-13), so
the teacher-forced steps feed the oracle the very values the GPU attends to and
hold the project's step bar unchanged: logits 1e-3 (assert_parity), tokens
exact up to ties at 1e-5 (tests/test_decoder_gpu.py)."""
import ctypes

import numpy as np
import pytest

from _fp8 import (DecoderConfig, F16Taps, FORM_BEAM, FORM_DIRECT, FORM_SPLIT_MERGE,
                  FORM_SPLIT_MERGE_ROW, FORM_WG_MERGE, NAN_CODES, Pages, boundary_sensitive,
                  f16_model, fp8_kv_to_oracle, make_decoder, ref_decode, ref_encode)
from _util import assert_parity, record, rel_err

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-3
TIE_TOL = 1e-5
FREE_RUN_TOL = 2.5e-2
BOUNDARY_CAP = 1e-4  # share of append bytes that may sit on a rounding boundary


def _torch():
    import torch
    return torch


def _int8_model(oracle, L=2, H=4, D=64, V=1000, S=64, seed=1234):
    from oracle.oracle import synthetic_int8_model
    return synthetic_int8_model(oracle, L=L, H=H, D=D, V=V, max_seq=S, seed=seed)


class _Taps:
    """llm_decoder_set_taps buffers of an INT8 decoder, unpacked into the
    oracle's forced-activation layout [L][4][B][max(hid, inter)]."""

    def __init__(self, dec, c, max_batch):
        torch = _torch()
        self.L, self.hid, self.inter = c["L"], c["hid"], c["inter"]
        self.K = max(self.hid, self.inter)
        self.b16 = (max_batch + 15) // 16 * 16
        self.maxB = max_batch
        self.q = torch.zeros(self.L * 4 * self.b16 * self.K, dtype=torch.int8, device="cuda")
        self.s = torch.zeros(self.L * 4 * max_batch, dtype=torch.float32, device="cuda")
        dec.set_taps(self.q.data_ptr(), self.s.data_ptr())

    def read(self, B):
        from oracle.oracle import unpack_a_i8
        q = self.q.cpu().numpy().reshape(self.L, 4, self.b16 * self.K)
        s = self.s.cpu().numpy().reshape(self.L, 4, self.maxB)
        fq = np.zeros((self.L, 4, B, self.K), np.int8)
        for l in range(self.L):
            for st in range(4):
                Kst = self.inter if st == 3 else self.hid
                fq[l, st, :, :Kst] = unpack_a_i8(q[l, st, :self.b16 * Kst], B, Kst)
        return fq, np.ascontiguousarray(s[:, :, :B])


def _check_append_bytes(oracle, w, fq, fs, got, k_scale, v_scale, tally):
    """The bytes one step appended (got uint8 [L][B][2][H][D]) against the
    reference encoding of the K / V pre-images, recomputed on the CPU from the
    tapped LN1 activations (the qkv GEMM epilogue is bit-exact to
    oracle.i8_gemm, and qkv has no bias).  A byte may differ only where the
    reference byte itself changes within one fp32 ulp of the pre-image."""
    c = w["cfg"]
    hid, H, D = c["hid"], c["H"], c["D"]
    for l in range(c["L"]):
        _, y = oracle.i8_gemm(fq[l, 0, :, :hid], w["wqkv"][l], sa=fs[l, 0], sw=w["sw_qkv"][l])
        B = y.shape[0]
        for which, sc in ((0, k_scale[l]), (1, v_scale[l])):
            pre = y[:, hid * (1 + which): hid * (2 + which)].reshape(B, H, D)
            want = ref_encode(pre, sc)
            g = got[l, :, which]
            diff = g != want
            assert not (diff & ~boundary_sensitive(pre, sc)).any(), (l, which, g[diff], want[diff])
            assert not np.isin(g, NAN_CODES).any()
            tally["bytes"] += g.size
            tally["boundary"] += int(diff.sum())
            tally["saturated"] += int(((want & 0x7F) == 0x7E).sum())


def _forced_steps(dec, odec, oracle, w, taps, pages, tokens_of, steps, k_scale, v_scale, pos0=0):
    """GPU (taps on) and teacher-forced oracle in lockstep: every step the
    bytes the GPU appended are read back, checked against the reference
    encoding, decoded to fp16 and fed to the oracle as its appended K / V."""
    torch = _torch()
    c = w["cfg"]
    B, V, L = odec.B, c["V"], c["L"]
    logits = torch.empty((B, V), device="cuda")
    nxt = [0] * B
    worst = 0.0
    tally = dict(bytes=0, boundary=0, saturated=0)
    for s in range(steps):
        tok = tokens_of(s, nxt)
        g_next = dec.step(tok, logits_ptr=logits.data_ptr())
        torch.cuda.synchronize()
        fq, fs = taps.read(B)
        got = pages.at(pages.pool(), B, [pos0 + s] * B, L)
        _check_append_bytes(oracle, w, fq, fs, got, k_scale, v_scale, tally)
        fkv = np.empty((L, B, 2, c["H"], c["D"]), np.float16)
        for l in range(L):
            for which, sc in ((0, k_scale[l]), (1, v_scale[l])):
                val = ref_decode(got[l, :, which], sc)
                fkv[l, :, which] = val.astype(np.float16)
                assert np.array_equal(fkv[l, :, which].astype(np.float32), val)
        o_logits, o_next, stats, attn = odec.step_attn(
            np.array(tok, np.int32), np.full(B, pos0 + s, np.int32), fq, fs, forced_kv=fkv)
        assert stats[:, :, 1].max() <= 1, (s, stats)    # int8 GEMM inputs within one LSB
        assert stats[:, :, 2].max() < 1e-5, (s, stats)  # row scales agree
        gl = logits.cpu().numpy()
        err = rel_err(gl, o_logits)
        print(f"step {s}: logits rel err {err:.3e}")
        assert_parity(gl, o_logits, LOGIT_TOL, axis=1, what=f"step {s} logits")
        worst = max(worst, err)
        for b in range(B):
            if g_next[b] != o_next[b]:
                gap = o_logits[b][o_next[b]] - o_logits[b][g_next[b]]
                assert gap <= TIE_TOL * np.abs(o_logits[b]).max(), (s, b, gap)
        nxt = list(g_next)
    assert tally["boundary"] <= BOUNDARY_CAP * tally["bytes"], tally
    return worst, tally


@pytest.mark.parametrize("H,D", [(4, 64), (2, 128)])
def test_teacher_forced_steps_and_append_bytes(gpu, oracle, H, D):
    """C1 dims, 3 ragged rows, 30 steps, a different power-of-two scale pair per
    layer: logits at the step bar, and every appended byte is the specified
    encoding of its pre-image."""
    from oracle.oracle import OracleDecoder
    w = _int8_model(oracle, L=2, H=H, D=D, V=1000, S=64)
    k_scale, v_scale = [0.25, 2.0], [4.0, 0.0625]
    dec = make_decoder(w, 3)
    assert dec.kv_dtype == "float8_e4m3fn"
    dec.set_kv_scales(k_scale, v_scale)
    taps = _Taps(dec, w["cfg"], 3)
    rng = np.random.default_rng(0)
    prompts = [list(rng.integers(0, 1000, n)) for n in (5, 17, 1)]
    dec.begin_synthetic(3, 0, 0, False)
    tokens_of = lambda s, nxt: [int(p[s]) if s < len(p) else int(nxt[b])
                                for b, p in enumerate(prompts)]
    worst, tally = _forced_steps(dec, OracleDecoder(oracle, w, 3), oracle, w, taps, Pages(dec),
                                 tokens_of, 30, k_scale, v_scale)
    print(f"fp8 forced lockstep D {D}: worst logit rel err {worst:.2e}, append bytes {tally}")


@pytest.mark.parametrize("log2_scale", [-8, -12])
def test_append_saturates_to_max_finite(gpu, oracle, log2_scale):
    """Scales that put pre-images beyond 448 * scale: those bytes are 0x7E /
    0xFE (the clamped reference), never a NaN code.  This model's K / V have a
    median magnitude of 0.21 and a maximum near 1.0 (the CPU oracle's own
    step), so 2^-8 (limit 1.75) clamps nothing here and 2^-12 (limit 0.109)
    clamps most; the saturated share of each is recorded."""
    w = _int8_model(oracle, L=2, H=4, D=64, V=1000, S=64)
    sc = [2.0 ** log2_scale] * 2
    dec = make_decoder(w, 3)
    dec.set_kv_scales(sc, sc)
    taps = _Taps(dec, w["cfg"], 3)
    pages = Pages(dec)
    dec.begin_synthetic(3, 0, 0, False)
    rng = np.random.default_rng(3)
    tally = dict(bytes=0, boundary=0, saturated=0)
    for s in range(4):
        dec.step([int(t) for t in rng.integers(0, 1000, 3)])
        _torch().cuda.synchronize()
        fq, fs = taps.read(3)
        got = pages.at(pages.pool(), 3, [s] * 3, 2)
        _check_append_bytes(oracle, w, fq, fs, got, sc, sc, tally)
    share = tally["saturated"] / tally["bytes"]
    record("kv_fp8", test="append_saturation", scale=sc[0], saturated_share=share, **tally)
    print(f"saturated share at scale 2^{log2_scale}: {share:.3f} of {tally['bytes']} bytes")
    if log2_scale == -12:
        assert share > 0.5, share
    assert tally["boundary"] <= BOUNDARY_CAP * tally["bytes"], tally


def test_non_power_of_two_scales(gpu, oracle):
    """k_scale 1.7, v_scale 0.3 over 12 steps from an empty context (the direct
    form; test_non_power_of_two_scales_through_the_merge_forms runs the others).
    A forgotten v_scale or a k_scale applied twice moves the attention by far
    more than the bars here.
    INT8 decoder: the oracle is teacher-forced with fp16(decode(byte) * scale),
    which is not exact now (2^-11 relative per element), so only layer 0's
    attention is held: its int8 image within one LSB and its row scales
    (absmax / 127 of the attention row) within 1e-3.
    FP16 decoder (fp16 o_proj input): the tapped fp16 attention rows of layer 0
    against the oracle's attention tensor at 1e-3, tensor-normalised (both
    sides carry fp16 roundings of single K / V elements, so the elementwise
    half of assert_parity does not apply)."""
    torch = _torch()
    from oracle.oracle import OracleDecoder
    k_scale, v_scale = [1.7, 1.7], [0.3, 0.3]
    rng = np.random.default_rng(5)
    # INT8 weights
    w = _int8_model(oracle, L=2, H=4, D=64, V=1000, S=64)
    dec = make_decoder(w, 2)
    dec.set_kv_scales(k_scale, v_scale)
    taps, pages = _Taps(dec, w["cfg"], 2), Pages(dec)
    odec = OracleDecoder(oracle, w, 2)
    dec.begin_synthetic(2, 0, 0, False)
    for s in range(12):
        tok = [int(t) for t in rng.integers(0, 1000, 2)]
        dec.step(tok)
        torch.cuda.synchronize()
        fq, fs = taps.read(2)
        got = pages.at(pages.pool(), 2, [s, s], 2)
        fkv = np.empty((2, 2, 2, 4, 64), np.float16)
        for l in range(2):
            fkv[l, :, 0] = ref_decode(got[l, :, 0], k_scale[l]).astype(np.float16)
            fkv[l, :, 1] = ref_decode(got[l, :, 1], v_scale[l]).astype(np.float16)
        _, _, stats, attn = odec.step_attn(np.array(tok, np.int32), np.full(2, s, np.int32), fq, fs,
                                           forced_kv=fkv)
        assert stats[0, 1, 1] <= 1 and stats[0, 1, 2] < 1e-3, (s, stats[0, 1])
        deq = fq[0, 1, :, :256].astype(np.float32) * fs[0, 1][:, None]
        assert rel_err(deq, attn[0]) < 1.0 / 127, s  # (half an int8 LSB of the row's absmax)
    # FP16 weights: the fp16 o_proj input
    L, H, D, V, S = 2, 2, 64, 300, 40
    wf = f16_model(rng, L, H, D, V, S)
    hid = wf["cfg"]["hid"]
    decf = make_decoder(wf, 2, cls="CUDADecoder")
    decf.set_kv_scales(k_scale, v_scale)
    ftaps, pages = F16Taps(decf, wf["cfg"], 2), Pages(decf)
    odec = OracleDecoder(oracle, wf, 2)
    decf.begin_synthetic(2, 0, 0, False)
    for s in range(12):
        tok = [int(t) for t in rng.integers(0, V, 2)]
        decf.step(tok)
        torch.cuda.synchronize()
        fh = ftaps.read(2)
        got = pages.at(pages.pool(), 2, [s, s], L)
        fkv = np.empty((L, 2, 2, H, D), np.float16)
        for l in range(L):
            fkv[l, :, 0] = ref_decode(got[l, :, 0], k_scale[l]).astype(np.float16)
            fkv[l, :, 1] = ref_decode(got[l, :, 1], v_scale[l]).astype(np.float16)
        _, _, _, attn = odec.step_attn(np.array(tok, np.int32), np.full(2, s, np.int32), fh,
                                       forced_kv=fkv)
        err = rel_err(fh[0, 1, :, :hid].astype(np.float32), attn[0])
        print(f"fp16-weights step {s}: layer-0 attention rel err {err:.3e}")
        assert err < 1e-3, (s, err)


@pytest.mark.parametrize("cls,rows,form", [("INT8Decoder", 16, FORM_WG_MERGE),
                                           ("INT8Decoder", 4, FORM_SPLIT_MERGE),
                                           ("CUDADecoder", 4, FORM_SPLIT_MERGE_ROW)])
def test_non_power_of_two_scales_through_the_merge_forms(gpu, oracle, cls, rows, form):
    """k_scale 1.7, v_scale 0.3 at context 2000 (L 1, H 4, D 128), where the
    step merges splits: in the workgroup, by pa_merge_kernel, and (FP16 weights:
    fp16 o_proj input) by pa_merge_row_kernel.
    FP16 weights: the oracle's fp16 KV holds fp16(decode(byte) * scale) (2^-11
    relative per element); the tapped fp16 attention rows against its attention
    tensor at 1e-3, tensor-normalised (the tap itself is rounded to fp16).
    INT8 weights: the reference is exact -- oracle.paged_attention over fp32
    pools of decode(byte) * scale with the step's own q.  The GPU's attention is
    visible only as its int8 image (one LSB = 1 / 127 of the row's absmax,
    coarser than 1e-3), so the 1e-3 bar is held on what that image keeps at full
    precision -- each row's scale, (absmax + 1e-6) / 127 of the attention row --
    and every int8 value is within one LSB of the quantised reference.  (Against
    the fp16-KV oracle instead, the 16-row case measured 1.14e-3 on the row
    scale: the reference's own fp16 rounding of K, not the kernel.)"""
    torch = _torch()
    from oracle.oracle import OracleDecoder
    T, k_scale, v_scale = 2000, [1.7], [0.3]
    rng = np.random.default_rng(rows)
    int8 = cls == "INT8Decoder"
    w = (_int8_model(oracle, L=1, H=4, D=128, V=512, S=T + 8, seed=51) if int8
         else f16_model(rng, 1, 4, 128, 512, T + 8))
    hid = w["cfg"]["hid"]
    dec = make_decoder(w, rows, cls=cls)
    dec.set_kv_scales(k_scale, v_scale)
    taps = _Taps(dec, w["cfg"], rows) if int8 else F16Taps(dec, w["cfg"], rows)
    dec.begin_synthetic(rows, T, 78, True)
    ns, got = dec.attention_plan()
    assert got == form and ns >= 2, (ns, got)
    odec = OracleDecoder(oracle, w, rows)
    pages = Pages(dec)
    fp8_kv_to_oracle(pages, odec, rows, T, k_scale, v_scale, exact=False)
    tok = [int(t) for t in rng.integers(0, 512, rows)]
    dec.step(tok)
    torch.cuda.synchronize()
    app = pages.at(pages.pool(), rows, [T] * rows, 1)
    fkv = np.empty((1, rows, 2, 4, 128), np.float16)
    fkv[0, :, 0] = ref_decode(app[0, :, 0], k_scale[0]).astype(np.float16)
    fkv[0, :, 1] = ref_decode(app[0, :, 1], v_scale[0]).astype(np.float16)
    pos = np.full(rows, T, np.int32)
    if int8:
        # exact reference: q recomputed from the tapped LN1 activations (the qkv
        # GEMM epilogue is bit-exact to oracle.i8_gemm), fp32 pools holding
        # decode(byte) * scale of every page, the decoder's own page table
        fq, fs = taps.read(rows)
        _, y = oracle.i8_gemm(fq[0, 0, :, :hid], w["wqkv"][0], sa=fs[0, 0], sw=w["sw_qkv"][0])
        pool = pages.pool()
        ref = oracle.paged_attention(
            np.ascontiguousarray(y[:, :hid]).reshape(rows, 4, 128),
            ref_decode(pool[:, 0], k_scale[0]), ref_decode(pool[:, 1], v_scale[0]),
            np.ascontiguousarray(pages.table(0)[:rows]), T=T + 1).reshape(rows, hid)
        amax = np.abs(ref).max(axis=1)
        want_s = (amax + 1e-6) / 127.0
        s_err = float(np.abs(fs[0, 1] - want_s).max() / want_s.max())
        want_q = np.clip(np.rint(ref * (127.0 / (amax + 1e-6))[:, None]), -128, 127)
        q_err = float(np.abs(fq[0, 1, :, :hid].astype(np.float64) - want_q).max())
        print(f"{cls} rows {rows}: {ns} splits form {got}, attention row scale rel err "
              f"{s_err:.3e}, int8 max diff {q_err}")
        assert_parity(fs[0, 1], want_s, 1e-3, what="attention row scales")
        assert q_err <= 1, q_err
    else:
        fh = taps.read(rows)
        _, _, _, attn = odec.step_attn(np.array(tok, np.int32), pos, fh, forced_kv=fkv)
        err = rel_err(fh[0, 1, :, :hid].astype(np.float32), attn[0])
        print(f"{cls} rows {rows}: {ns} splits form {got}, attention rel err {err:.3e}")
        assert err < 1e-3, err


@pytest.mark.parametrize("rows,form", [(16, FORM_WG_MERGE), (4, FORM_SPLIT_MERGE)])
def test_long_context_through_the_steps_launch_forms(gpu, oracle, rows, form):
    """L 1, H 4, D 128 at context 2000 (begin_synthetic on an FP8 decoder fills
    the pages with seeded bytes): the pages are read back, decoded at the
    layer's scales into the oracle's KV, and one step is teacher forced.  16
    rows merge their 8 splits in the workgroup; 4 rows take more splits than a
    workgroup merge holds and run split + merge.  The fp16-KV twin reports the
    same form."""
    from oracle.oracle import OracleDecoder
    T = 2000
    w = _int8_model(oracle, L=1, H=4, D=128, V=512, S=T + 8, seed=51)
    k_scale, v_scale = [2.0], [0.5]
    dec = make_decoder(w, rows)
    dec.set_kv_scales(k_scale, v_scale)
    taps = _Taps(dec, w["cfg"], rows)
    dec.begin_synthetic(rows, T, 77, True)
    ns, got = dec.attention_plan()
    assert got == form and ns >= 2 and (form != FORM_WG_MERGE or ns <= 8), (ns, got)
    twin = make_decoder(w, rows, kv_dtype="float16")
    twin.begin_synthetic(rows, T, 77, True)
    assert twin.attention_plan()[1] == form, twin.attention_plan()
    del twin
    odec = OracleDecoder(oracle, w, rows)
    pages = Pages(dec)
    fp8_kv_to_oracle(pages, odec, rows, T, k_scale, v_scale)
    rng = np.random.default_rng(T + rows)
    first = [int(t) for t in rng.integers(0, 512, rows)]
    worst, tally = _forced_steps(dec, odec, oracle, w, taps, pages,
                                 lambda s, nxt: first if s == 0 else [int(t) for t in nxt], 2,
                                 k_scale, v_scale, pos0=T)
    print(f"fp8 rows {rows} T {T}: {ns} splits form {got}, logits rel err {worst:.2e}")


def test_direct_form_step(gpu, oracle):
    """A short context is one split per (row, head): the direct form, which
    applies v_scale itself."""
    from oracle.oracle import OracleDecoder
    w = _int8_model(oracle, L=1, H=4, D=128, V=512, S=96, seed=52)
    k_scale, v_scale = [0.5], [4.0]
    dec = make_decoder(w, 2)
    dec.set_kv_scales(k_scale, v_scale)
    taps = _Taps(dec, w["cfg"], 2)
    dec.begin_synthetic(2, 40, 5, True)
    assert dec.attention_plan() == (1, FORM_DIRECT)
    odec = OracleDecoder(oracle, w, 2)
    pages = Pages(dec)
    fp8_kv_to_oracle(pages, odec, 2, 40, k_scale, v_scale)
    _forced_steps(dec, odec, oracle, w, taps, pages,
                  lambda s, nxt: [7, 9] if s == 0 else [int(t) for t in nxt], 3, k_scale, v_scale,
                  pos0=40)


def _code_ordinal(b):
    """e4m3 codes in value order (-0 and +0 both 0): adjacent values differ by 1."""
    m = (b & 0x7F).astype(np.int32)
    return np.where(b & 0x80, -m, m)


def test_prefill_equals_token_by_token(gpu, oracle):
    """prefill of a 530-token (two chunks) and a 9-token prompt against the same
    prompts fed one token per step, on the model of
    test_prefill_decode_kernel_fallback (an FP8 decoder prefills through the
    decode kernel: chunk GEMM append, beam_ids = the row, context p0 + i + 1).
    Logits within FREE_RUN_TOL.  Bytes: layer 0's K / V pre-images depend on
    the token alone, so its bytes agree except where an int8 LN1 activation
    flipped between the two paths (below 1e-3 of the activations,
    tests/test_decoder_gpu.py; one flip moves a pre-image by ~1 / (127
    sqrt(hid)) of its size against an e4m3 spacing of 2^-4 .. 2^-3, a few 1e-3
    of the row's bytes) or the pre-image sits on a rounding boundary: at most
    1e-2 of them differ, each by one code.  (Prefill chunks are not tapped, so
    the pre-images themselves are not available for the exact boundary rule;
    deeper layers inherit the int8 flips and are held by the logits.)"""
    torch = _torch()
    w = _int8_model(oracle, L=2, H=2, D=256, V=400, S=700, seed=13)
    V = 400
    rng = np.random.default_rng(4)
    prompts = [rng.integers(0, V, 530).tolist(), rng.integers(0, V, 9).tolist()]
    la, bytes_a = [], []
    for p in prompts:
        a = make_decoder(w, 1)
        a.begin_synthetic(1, 0, 0, False)
        l1 = torch.empty((1, V), device="cuda")
        for t in p:
            a.step([t], logits_ptr=l1.data_ptr())
        torch.cuda.synchronize()
        la.append(l1[0].cpu().numpy().copy())
        pg = Pages(a)
        bytes_a.append(pg.context(pg.pool(), 0, 1, len(p))[:, 0])
    b = make_decoder(w, 2)
    b.begin_synthetic(2, 0, 0, False)
    for r, p in enumerate(prompts):
        b.prefill(r, p[:-1])
    lb = torch.empty((2, V), device="cuda")
    b.step([p[-1] for p in prompts], logits_ptr=lb.data_ptr())
    torch.cuda.synchronize()
    lb = lb.cpu().numpy()
    pg = Pages(b)
    pool = pg.pool()
    for r, p in enumerate(prompts):
        assert b.context_len(r) == len(p)
        got = pg.context(pool, 0, 1, len(p), row0=r)[:, 0]
        assert not np.isin(got, NAN_CODES).any()
        diff = got != bytes_a[r]
        share = float(diff.mean())
        step = np.abs(_code_ordinal(got[diff]) - _code_ordinal(bytes_a[r][diff]))
        err = rel_err(lb[r], la[r])
        record("kv_fp8", test="prefill_vs_stepping", row=r, layer0_byte_diff_share=share,
               max_code_step=int(step.max()) if step.size else 0, logit_err=err)
        print(f"row {r}: layer-0 bytes differing {share:.2e}, logits rel err {err:.2e}")
        assert share <= 1e-2, (r, share)
        assert (step <= 1).all(), (r, step.max())
        assert err < FREE_RUN_TOL, (r, err)


def test_generate_and_beams_run(gpu, oracle):
    """generate (which prefills the prompt: an FP8 decoder prefills through the
    decode kernel, the MFMA prefill reads fp16 pools), generate_batch and a beam
    step run on an FP8 decoder; a fork's
    copy-on-write copies bytes: after the forked rows append, the page they
    shared keeps its bytes and every new page starts with the same prefix."""
    torch = _torch()
    w = _int8_model(oracle, L=1, H=2, D=64, V=300, S=48, seed=3)
    dec = make_decoder(w, 4)
    prompt = [3, 14, 15, 92]
    r1 = dec.generate(prompt, 10, 1.0)
    assert r1[:4] == prompt and len(r1) == 14 and all(0 <= t < 300 for t in r1)
    assert dec.generate(prompt, 10, 1.0) == r1
    rb = dec.generate_batch([prompt, [7], prompt], 10)
    assert rb[0] == r1 and rb[2] == r1 and len(rb[1]) == 11
    # 4 beams sharing 20 tokens: tile 0 full, tile 1 holds 4 tokens of every beam
    dec.begin_beams(1, 4, 20, 0, 9, True)
    ns, form = dec.attention_plan()
    assert form & FORM_BEAM == 0, form  # the LDS beam form is fp16-KV only
    pg = Pages(dec)
    before, pt0 = pg.pool(), pg.table(0)
    assert len({int(x) for x in pt0[:4, 0, 1]}) == 1  # one shared page
    logits = torch.empty((4, 300), device="cuda")
    dec.step([1, 2, 3, 4], logits_ptr=logits.data_ptr())
    torch.cuda.synchronize()
    assert np.isfinite(logits.cpu().numpy()).all()
    after, pt1 = pg.pool(), pg.table(0)
    for h in range(2):
        shared = int(pt0[0, h, 1])
        now = [int(x) for x in pt1[:4, h, 1]]
        assert len(set(now)) == 4, now  # every beam owns its page after the append
        for r in range(4):
            assert np.array_equal(after[now[r], :, :4], before[shared, :, :4]), (h, r)
        assert np.array_equal(after[shared, :, :4], before[shared, :, :4])
        assert np.array_equal(after[shared, :, 5:], before[shared, :, 5:])
        assert np.array_equal(after[int(pt1[0, h, 0])], before[int(pt0[0, h, 0])])  # tile 0 shared


def test_surface(gpu, oracle, tmp_path):
    import llm_capi
    lib = gpu
    w = _int8_model(oracle, L=2, H=2, D=64, V=300, S=48, seed=3)
    d8, d16 = make_decoder(w, 2), make_decoder(w, 2, kv_dtype="float16")
    assert (d8.kv_dtype, d16.kv_dtype) == ("float8_e4m3fn", "float16")
    kv8, kv16 = ctypes.c_void_p(d8.kv_handle), ctypes.c_void_p(d16.kv_handle)
    assert lib.kv_cache_page_stride(kv8) * 2 == lib.kv_cache_page_stride(kv16)
    assert lib.kv_cache_num_pages(kv8) == lib.kv_cache_num_pages(kv16)
    with pytest.raises(RuntimeError):
        d16.set_kv_scales([1.0, 1.0], [1.0, 1.0])  # fp16 KV has no scales
    with pytest.raises(RuntimeError):
        d8.set_kv_scales([1.0, 0.0], None)         # must be > 0
    with pytest.raises(RuntimeError):
        d8.set_kv_scales([1.0, float("inf")], None)
    d8.set_kv_scales([2.0, 0.5], None)
    d8.begin_synthetic(2, 20, 1, True)
    with pytest.raises(RuntimeError):
        d8.set_kv_scales([1.0, 1.0], [1.0, 1.0])  # rows are active
    # the C entries' status codes
    cfg = DecoderConfig(num_layers=1, num_heads=2, head_dim=64, hidden_dim=128, vocab_size=100,
                        max_seq_len=32, weight_dtype=llm_capi.LLM_I8, max_batch=1)
    h = ctypes.c_void_p()
    llm_capi.check(lib.llm_decoder_create_kv(ctypes.byref(cfg), llm_capi.LLM_FP8, ctypes.byref(h)))
    assert lib.llm_decoder_kv_dtype(h) == llm_capi.LLM_FP8
    one = (ctypes.c_float * 1)(1.0)
    assert lib.llm_decoder_set_kv_scales(h, one, one) == llm_capi.LLM_OK
    llm_capi.check(lib.llm_decoder_begin_synthetic(h, 1, 4, 0, 0))
    assert lib.llm_decoder_set_kv_scales(h, one, one) == llm_capi.LLM_ERR_INVALID
    lib.llm_decoder_destroy(h)
    h16 = ctypes.c_void_p()
    llm_capi.check(lib.llm_decoder_create_kv(ctypes.byref(cfg), llm_capi.LLM_F16, ctypes.byref(h16)))
    assert lib.llm_decoder_kv_dtype(h16) == llm_capi.LLM_F16
    assert lib.llm_decoder_set_kv_scales(h16, one, one) == llm_capi.LLM_ERR_INVALID
    lib.llm_decoder_destroy(h16)
    # snapshot round trip restores the bytes (and the table)
    path = str(tmp_path / "dec_fp8.kv").encode()
    llm_capi.check(lib.kv_cache_save(kv8, path))
    pg = Pages(d8)
    want = [pg.context(pg.pool(), l, 2, 20) for l in range(2)]
    other = make_decoder(w, 2)
    other.begin_synthetic(2, 0, 2, False)
    llm_capi.check(lib.kv_cache_load(ctypes.c_void_p(other.kv_handle), path))
    llm_capi.check(lib.kv_cache_sync(ctypes.c_void_p(other.kv_handle), None))
    _torch().cuda.synchronize()
    pg2 = Pages(other)
    for l in range(2):
        assert np.array_equal(pg2.context(pg2.pool(), l, 2, 20), want[l])
    assert lib.kv_cache_load(kv16, path) == llm_capi.LLM_ERR_INVALID  # the file's kv_dtype differs


def test_accuracy_record(gpu, oracle):
    """FP8 is lossy by design: the same model and prompts on the fp16-KV and the
    FP8-KV decoder at scale 1, 32 steps.  The figures are recorded (DESIGN);
    the assertion only catches a scrambled layout."""
    torch = _torch()
    w = _int8_model(oracle, L=2, H=4, D=64, V=1000, S=64)
    rng = np.random.default_rng(6)
    toks = rng.integers(0, 1000, (32, 3))
    out = {}
    for kvd in ("float16", "fp8"):
        dec = make_decoder(w, 3, kv_dtype=kvd)
        dec.begin_synthetic(3, 0, 0, False)
        logits = torch.empty((3, 1000), device="cuda")
        rows = []
        for s in range(32):
            dec.step([int(t) for t in toks[s]], logits_ptr=logits.data_ptr())
            torch.cuda.synchronize()
            rows.append(logits.cpu().numpy().copy())
        out[kvd] = np.stack(rows)
    assert np.isfinite(out["fp8"]).all()
    errs = [rel_err(out["fp8"][s], out["float16"][s]) for s in range(32)]
    top1 = float((out["fp8"].argmax(-1) == out["float16"].argmax(-1)).mean())
    record("kv_fp8", test="accuracy_c1_dims", logit_rel_err_max=max(errs),
           logit_rel_err_mean=float(np.mean(errs)), top1_agreement=top1, steps=32)
    print(f"fp8 vs fp16 KV: logit rel err max {max(errs):.3e} mean {np.mean(errs):.3e}, "
          f"top-1 agreement {top1:.3f}")
    assert max(errs) < 0.5
