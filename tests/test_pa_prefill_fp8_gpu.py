"""Parity of the MFMA prefill attention on FP8 (OCP e4m3fn) pools (pa_prefill
with LLM_FP8 views, read at scale 1 as pa_decode reads them).

Every e4m3 value is an fp16 normal (2^-9 .. 448), so the kernel's decode at
staging is exact and three references hold at the fp16 kernel's own bars:
  1. the CPU oracle on the decoded fp32 values, 1e-3 relative with the
     elementwise floor ATOL_FRAC = 4e-6 (tests/test_pa_prefill_gpu.py);
  2. pa_decode on the same FP8 pools and rows, same bar;
  3. pa_prefill on fp16 pools holding the decoded values: bit-equal, which pins
     every byte's decode and its place in LDS.
In the last page the bytes past the context are NaN codes (0x7F) in K and V: a
masked key stages zeros, so they never reach the output."""
import numpy as np
import pytest

from _fp8 import dev_fp8, fp8_pools, ref_decode
from _util import assert_parity

pytestmark = pytest.mark.gpu
RTOL = 1e-3
ATOL_FRAC = 4e-6
NAN_CODE = 0x7F


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _case(rng, *, rows, H, D, T, ts, missing=0.0, nan_tail=False):
    """(k bytes, v bytes, k fp32, v fp32, page table); the fp32 pools are the
    bytes' exact values, NaN where the bytes are NaN codes."""
    nt = (T + ts - 1) // ts
    num_pages = rows * H * nt + 7
    kb, vb, kf, vf = fp8_pools(rng, (num_pages, ts, D), D ** -0.25)
    perm = rng.permutation(num_pages)[: rows * H * nt].astype(np.int32)
    pt = np.full((rows, H, nt + 2), -1, np.int32)
    pt[:, :, :nt] = perm.reshape(rows, H, nt)
    if missing:
        gone = rng.random(pt[:, :, :nt].shape) < missing
        pt[:, :, :nt][gone] = -1
    if nan_tail and T % ts:
        for p in pt[:, :, nt - 1].ravel():
            if p >= 0:
                kb[p, T % ts:] = NAN_CODE
                vb[p, T % ts:] = NAN_CODE
                kf[p, T % ts:] = np.nan
                vf[p, T % ts:] = np.nan
    return kb, vb, kf, vf, pt


def _oracle(oracle, q, kf, vf, pt, row, p0, sm_scale=1.0):
    m = q.shape[0]
    T = p0 + m
    return oracle.paged_attention(
        q, kf, vf, pt, T=T, beam_ids=np.full(m, row, np.int32),
        context_lens=np.arange(p0 + 1, T + 1, dtype=np.int32), temperature=sm_scale ** -0.5)


def _f16_exact(x):
    h = x.astype(np.float16)
    ok = ~np.isnan(x)
    assert np.array_equal(h.astype(np.float32)[ok], x[ok]) and np.isnan(h[~ok]).all()
    return h


@pytest.mark.parametrize("H,D,ts,p0,m,row", [
    (4, 64, 16, 0, 1, 0),       # one token, one key
    (4, 64, 16, 0, 37, 1),      # ragged query block, first chunk
    (3, 128, 16, 0, 33, 2),
    (2, 128, 16, 1000, 200, 1), # later chunk: long prefix, ragged tail page
    (2, 128, 32, 517, 96, 0),   # page 32
    (2, 64, 32, 31, 1, 1),
])
@pytest.mark.parametrize("split", [True, False])
def test_pa_prefill_fp8(gpu, oracle, H, D, ts, p0, m, row, split):
    import llm_capi
    rng = np.random.default_rng(p0 * 7 + m + D)
    kb, vb, kf, vf, pt = _case(rng, rows=3, H=H, D=D, T=p0 + m, ts=ts, nan_tail=True)
    q = (rng.standard_normal((m, H, D)) * D ** -0.25).astype(np.float32)
    out = llm_capi.pa_prefill(_dev(q), dev_fp8(kb), dev_fp8(vb), _dev(pt), row=row, p0=p0,
                              split=split).cpu().numpy()
    # 1. the oracle on the decoded values
    ref = _oracle(oracle, q, kf, vf, pt, row, p0)
    assert np.isfinite(out).all()
    assert_parity(out, ref, RTOL, ATOL_FRAC)
    # 2. the decode kernel on the same FP8 pools and rows
    dec = llm_capi.pa_decode(_dev(q), dev_fp8(kb), dev_fp8(vb), _dev(pt), T=p0 + m,
                             beam_ids=_dev(np.full(m, row, np.int32)),
                             context_lens=_dev(np.arange(p0 + 1, p0 + m + 1, dtype=np.int32)))
    assert_parity(out, dec.cpu().numpy(), RTOL, ATOL_FRAC)
    # 3. the fp16 kernel on the decoded values (NaN tails included): the same bits
    out16 = llm_capi.pa_prefill(_dev(q), _dev(_f16_exact(kf)), _dev(_f16_exact(vf)), _dev(pt),
                                row=row, p0=p0, split=split).cpu().numpy()
    assert np.array_equal(out, out16)


@pytest.mark.parametrize("split", [True, False])
def test_pa_prefill_fp8_every_code(gpu, split):
    """Every non-NaN byte value, in every position of a lane's 8-byte chunk, in
    K and in V: bit-equal to the fp16 kernel on the decoded values (subnormal
    codes 0x01 .. 0x07, both zeros and +-448 included).  K codes are large here
    (the softmax is near one-hot), which the bit comparison does not mind."""
    import llm_capi
    H, D, ts, m = 2, 64, 16, 40
    nt = 3
    rng = np.random.default_rng(17)
    codes = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)
    n = H * nt * ts * D
    kb = np.resize(codes, n)
    vb = np.resize(codes[::-1], n)
    # shift by one element per row so each code meets each chunk position
    kb = np.stack([np.roll(r, i) for i, r in enumerate(kb.reshape(-1, D))]).reshape(H * nt, ts, D)
    vb = np.stack([np.roll(r, i) for i, r in enumerate(vb.reshape(-1, D))]).reshape(H * nt, ts, D)
    for b in (kb, vb):
        assert set(np.unique(b)) == set(codes.tolist())
    pt = rng.permutation(H * nt).astype(np.int32).reshape(1, H, nt)
    q = (rng.standard_normal((m, H, D)) * 1e-3).astype(np.float32)
    out = llm_capi.pa_prefill(_dev(q), dev_fp8(kb), dev_fp8(vb), _dev(pt), row=0, p0=0,
                              split=split).cpu().numpy()
    out16 = llm_capi.pa_prefill(_dev(q), _dev(_f16_exact(ref_decode(kb))),
                                _dev(_f16_exact(ref_decode(vb))), _dev(pt), row=0, p0=0,
                                split=split).cpu().numpy()
    assert np.isfinite(out).all()
    assert np.array_equal(out, out16)


@pytest.mark.parametrize("code", [0x7F, 0xFF])
def test_pa_prefill_fp8_nan_code_is_nan(gpu, code):
    """A NaN code inside the context decodes to NaN and nothing else.  In V, at
    key 0 (which every query sees), it makes exactly the output dim it sits in
    NaN; in K, at key 21, it makes the whole head of exactly the queries that
    see that key NaN (their score is NaN; earlier queries mask it)."""
    import llm_capi
    H, D, ts, m = 2, 64, 16, 40
    rng = np.random.default_rng(23)
    kb, vb, kf, vf, pt = _case(rng, rows=1, H=H, D=D, T=m, ts=ts)
    q = (rng.standard_normal((m, H, D)) * D ** -0.25).astype(np.float32)
    key, dim, head = 21, 13, 1
    vb2 = vb.copy()
    vb2[pt[0, head, 0], 0, dim] = code
    out = llm_capi.pa_prefill(_dev(q), dev_fp8(kb), dev_fp8(vb2), _dev(pt), row=0, p0=0,
                              split=False).cpu().numpy()
    want = np.zeros((m, H, D), bool)
    want[:, head, dim] = True
    assert np.array_equal(np.isnan(out), want)
    page = pt[0, head, key // ts]
    kb2 = kb.copy()
    kb2[page, key % ts, dim] = code
    out = llm_capi.pa_prefill(_dev(q), dev_fp8(kb2), dev_fp8(vb), _dev(pt), row=0, p0=0,
                              split=False).cpu().numpy()
    want = np.zeros((m, H, D), bool)
    want[key:, head, :] = True
    assert np.array_equal(np.isnan(out), want)


def test_pa_prefill_fp8_missing_pages_and_scale(gpu, oracle):
    import llm_capi
    rng = np.random.default_rng(11)
    H, D, ts, p0, m = 3, 128, 16, 300, 70
    kb, vb, kf, vf, pt = _case(rng, rows=2, H=H, D=D, T=p0 + m, ts=ts, missing=0.15)
    # spiky scores: a large sm_scale stresses the running-max rescale
    q = (rng.standard_normal((m, H, D)) * 2.0).astype(np.float32)
    out = llm_capi.pa_prefill(_dev(q), dev_fp8(kb), dev_fp8(vb), _dev(pt), row=1, p0=p0,
                              sm_scale=0.5).cpu().numpy()
    ref = _oracle(oracle, q, kf, vf, pt, 1, p0, sm_scale=0.5)
    assert_parity(out, ref, RTOL, ATOL_FRAC)


def test_pa_prefill_fp8_all_missing_is_zero(gpu):
    import llm_capi
    rng = np.random.default_rng(3)
    kb, vb, kf, vf, pt = _case(rng, rows=1, H=2, D=64, T=40, ts=16)
    pt[:] = -1
    q = rng.standard_normal((40, 2, 64)).astype(np.float32)
    out = llm_capi.pa_prefill(_dev(q), dev_fp8(kb), dev_fp8(vb), _dev(pt), row=0,
                              p0=0).cpu().numpy()
    np.testing.assert_array_equal(out, np.zeros_like(out))


def test_pa_prefill_fp8_strided_q_interleaved_pools(gpu, oracle):
    """q read in place from a wider row (the decoder's qkv rows) and K/V pages
    interleaved in one [num_pages][2][ts][D] allocation (kv_cache's own layout:
    the page stride is in bytes, 2 * ts * D for one-byte elements)."""
    import torch
    import llm_capi
    rng = np.random.default_rng(5)
    H, D, ts, p0, m = 4, 128, 16, 64, 48
    kb, vb, kf, vf, pt = _case(rng, rows=1, H=H, D=D, T=p0 + m, ts=ts)
    kv = torch.empty((kb.shape[0], 2, ts, D), dtype=torch.float8_e4m3fn, device="cuda")
    kv.view(torch.uint8)[:, 0] = _dev(kb)
    kv.view(torch.uint8)[:, 1] = _dev(vb)
    q = (rng.standard_normal((m, H, D)) * D ** -0.25).astype(np.float32)
    wide = torch.zeros((m, 3 * H * D), dtype=torch.float32, device="cuda")
    wide[:, :H * D] = _dev(q.reshape(m, H * D))
    out = llm_capi.pa_prefill(wide, kv[:, 0], kv[:, 1], _dev(pt), row=0, p0=p0).cpu().numpy()
    ref = _oracle(oracle, q, kf, vf, pt, 0, p0)
    assert_parity(out, ref, RTOL, ATOL_FRAC)


def test_pa_prefill_fp8_rejects_head_dim_32(gpu):
    import llm_capi
    rng = np.random.default_rng(1)
    kb, vb, kf, vf, pt = _case(rng, rows=1, H=2, D=32, T=20, ts=16)
    q = rng.standard_normal((20, 2, 32)).astype(np.float32)
    with pytest.raises(llm_capi.LlmError) as ei:
        llm_capi.pa_prefill(_dev(q), dev_fp8(kb), dev_fp8(vb), _dev(pt), row=0, p0=0)
    assert ei.value.status == llm_capi.LLM_ERR_UNSUPPORTED
