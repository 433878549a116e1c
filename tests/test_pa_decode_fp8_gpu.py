"""pa_decode / pa_decode_grouped / pa_decode_ex over FP8 (OCP e4m3fn) KV pools.

The public entries read FP8 pools as plain numbers (scale 1, as they read
LLM_I8).  The reference is the CPU oracle over fp32 pools holding the decoded
values, so FP8 itself adds no error and the project's attention bar (1e-3,
assert_parity) applies unchanged."""
import ctypes

import numpy as np
import pytest

from _fp8 import (FORM_DIRECT, FORM_SPLIT_MERGE, NAN_CODES, dev_fp8, fp8_pools, ref_decode)
from _util import assert_parity

pytestmark = pytest.mark.gpu
RTOL = 1e-3


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("D,ts", [(128, 16), (64, 32)])
def test_every_code_decodes_right(gpu, D, ts):
    """Context length 1: out = v / (1 + 1e-6) for the one token, so every
    element shows its decoded value.  V pages hold the codes 0..255 (the two
    NaN codes replaced), K is arbitrary."""
    import llm_capi
    B, H = 1, 2
    codes = np.arange(256, dtype=np.uint8)
    codes[list(NAN_CODES)] = (0x3C, 0xBC)
    n_pages = -(-256 // D) + 1
    rng = np.random.default_rng(D)
    kb = rng.integers(0, 0x40, size=(n_pages, ts, D)).astype(np.uint8)
    q = _dev(rng.standard_normal((B, H, D)).astype(np.float32))
    for first in range(0, 256, D):  # D codes per token row
        vb = rng.integers(0, 0x78, size=(n_pages, ts, D)).astype(np.uint8)
        chunk = np.stack([codes[first:first + D], codes[first:first + D][::-1]])
        pt = np.array([[[0], [1]]], np.int32)  # head h reads page h, token 0
        vb[0, 0], vb[1, 0] = chunk[0], chunk[1]
        out = llm_capi.pa_decode(q, dev_fp8(kb), dev_fp8(vb), _dev(pt), T=1).cpu().numpy()
        want = ref_decode(chunk).astype(np.float64) / (1.0 + 1e-6)
        err = np.abs(out[0] - want)
        assert (err <= 1e-6 * np.abs(want)).all(), (first, np.argmax(err))


def _random_case(rng, B, H, D, T, ts, *, num_beams=None, max_tiles=None, missing_frac=0.0):
    num_beams = num_beams or B
    nt = (T + ts - 1) // ts
    max_tiles = max_tiles or nt
    num_pages = num_beams * H * nt + 5
    q = (rng.standard_normal((B, H, D)) * D ** -0.25).astype(np.float32)
    kb, vb, kf, vf = fp8_pools(rng, (num_pages, ts, D), D ** -0.25)
    perm = rng.permutation(num_pages)[: num_beams * H * nt].astype(np.int32)
    pt = np.full((num_beams, H, max_tiles), -1, np.int32)
    pt[:, :, :nt] = perm.reshape(num_beams, H, nt)
    if missing_frac:
        mask = rng.random(pt[:, :, :nt].shape) < missing_frac
        pt[:, :, :nt][mask] = -1
    return q, kb, vb, kf, vf, pt


@pytest.mark.parametrize("B,H,D,T,ts", [
    (3, 4, 128, 1000, 16),
    (5, 3, 64, 257, 32),
    (2, 2, 256, 300, 16),
    (5, 3, 32, 257, 32),  # the 1 KiB minimum page
])
def test_random_pools_vs_oracle(gpu, oracle, B, H, D, T, ts):
    import llm_capi
    rng = np.random.default_rng(B * 1000 + T + D)
    q, kb, vb, kf, vf, pt = _random_case(rng, B, H, D, T, ts, missing_frac=0.02)
    ref = oracle.paged_attention(q, kf, vf, pt, T=T)
    kd, vd = dev_fp8(kb), dev_fp8(vb)
    for pps in (0, 8, 64):
        out = llm_capi.pa_decode(_dev(q), kd, vd, _dev(pt), T=T, pages_per_split=pps).cpu().numpy()
        assert_parity(out, ref, RTOL, what=f"pps {pps}")


def test_ragged_context_and_beams(gpu, oracle):
    """The case of test_pa_decode_ragged_context_and_beams on FP8 pools; the
    row of context 0 gives exact zeros."""
    import llm_capi
    rng = np.random.default_rng(11)
    B, H, D, T, ts = 6, 4, 128, 700, 16
    q, kb, vb, kf, vf, pt = _random_case(rng, B, H, D, T, ts, num_beams=3, max_tiles=50)
    beam_ids = np.array([2, 0, 1, 1, 0, 2], np.int32)
    lens = np.array([700, 1, 0, 17, 512, 333], np.int32)
    ref = oracle.paged_attention(q, kf, vf, pt, T=T, beam_ids=beam_ids, context_lens=lens)
    kd, vd = dev_fp8(kb), dev_fp8(vb)
    for pps in (0, 4, 64):
        out = llm_capi.pa_decode(_dev(q), kd, vd, _dev(pt), T=T, beam_ids=_dev(beam_ids),
                                 context_lens=_dev(lens), pages_per_split=pps).cpu().numpy()
        assert_parity(out, ref, RTOL)
        np.testing.assert_array_equal(out[2], 0.0)


def test_stale_nan_bytes_ignored(gpu, oracle):
    """Bytes past the context and in unmapped pages may be anything, the NaN
    codes included; they must not reach the output."""
    import llm_capi
    rng = np.random.default_rng(17)
    B, H, D, T, ts = 3, 2, 128, 200, 16
    q, kb, vb, kf, vf, pt = _random_case(rng, B, H, D, T, ts)
    ref = oracle.paged_attention(q, kf, vf, pt, T=T)
    last = pt[:, :, T // ts]
    kb[last, T % ts:] = 0x7F
    vb[last, T % ts:] = 0xFF
    unused = np.setdiff1d(np.arange(kb.shape[0]), pt.ravel())
    kb[unused] = 0xFF
    vb[unused] = 0x7F
    for pps in (0, 4):
        out = llm_capi.pa_decode(_dev(q), dev_fp8(kb), dev_fp8(vb), _dev(pt), T=T,
                                 pages_per_split=pps).cpu().numpy()
        assert np.isfinite(out).all()
        assert_parity(out, ref, RTOL)


def test_grouped_entry_equals_pa_decode_bitwise(gpu):
    """row_group 4 on a forked table (4 beams sharing a prefix): FP8 rows take
    the plain grouped schedule (the LDS beam form is fp16 only), the same
    arithmetic as pa_decode."""
    import torch
    import llm_capi
    rng = np.random.default_rng(23)
    B, H, D, T, ts = 8, 3, 128, 600, 16
    q, kb, vb, _, _, pt = _random_case(rng, B, H, D, T, ts)
    shared = 30  # leading tiles the 4 beams of a sequence share
    for g in range(0, B, 4):
        pt[g + 1:g + 4, :, :shared] = pt[g, :, :shared]
    lens = np.array([600, 600, 600, 600, 599, 333, 600, 17], np.int32)
    lib = llm_capi.load()
    view = llm_capi.kv_view(dev_fp8(kb), dev_fp8(vb), _dev(pt))
    ns, form = ctypes.c_int32(), ctypes.c_int32()
    llm_capi.check(lib.pa_decode_plan(ctypes.byref(view), B, H, D, T, 0, 4, ctypes.byref(ns),
                                      ctypes.byref(form)))
    assert form.value & 16 == 0, form.value  # no LLM_PA_FORM_BEAM on FP8 pools
    kd, vd = dev_fp8(kb), dev_fp8(vb)
    for pps in (0, 8):
        a = llm_capi.pa_decode(_dev(q), kd, vd, _dev(pt), T=T, context_lens=_dev(lens),
                               pages_per_split=pps)
        b = llm_capi.pa_decode(_dev(q), kd, vd, _dev(pt), T=T, context_lens=_dev(lens),
                               pages_per_split=pps, row_group=4)
        assert torch.equal(a, b), pps


def test_options_top_k(gpu, oracle):
    import llm_capi
    rng = np.random.default_rng(29)
    B, H, D, T, ts = 2, 2, 64, 200, 16
    nt = (T + ts - 1) // ts
    num_pages = B * H * nt + 2
    q = (rng.standard_normal((B, H, D)) * 0.5).astype(np.float32)
    kb, vb, kf, vf = fp8_pools(rng, (num_pages, ts, D), 0.5)
    pt = rng.permutation(num_pages)[: B * H * nt].astype(np.int32).reshape(B, H, nt)
    pt[1, 0, 3] = -1
    lens = np.array([200, 133], np.int32)
    ref, rp, _ = oracle.paged_attention(q, kf, vf, pt, T=T, context_lens=lens, temperature=0.8,
                                        top_k=7, want_probs=True)
    out, probs, _ = llm_capi.pa_decode_ex(_dev(q), dev_fp8(kb), dev_fp8(vb), _dev(pt), T=T,
                                          context_lens=_dev(lens), temperature=0.8, top_k=7,
                                          want_probs=True)
    assert_parity(out.cpu().numpy(), ref, RTOL)
    assert_parity(probs.cpu().numpy(), rp, RTOL)
    np.testing.assert_array_equal(probs.cpu().numpy() > 0, rp > 0)


@pytest.mark.parametrize("B,H,T,pps,form", [
    (4, 4, 100, 0, FORM_DIRECT),        # 7 pages: one split
    (2, 2, 1000, 8, FORM_SPLIT_MERGE),  # 63 pages in fixed splits of 8
    (16, 12, 2048, 0, FORM_SPLIT_MERGE),  # dynamic splits (the device's occupancy)
])
def test_launch_forms(gpu, oracle, B, H, T, pps, form):
    """The forms pa_decode takes on FP8 views, asserted so the coverage cannot
    vanish.  The public entry never merges in the workgroup (no row outputs):
    that form is the decoder's, asserted through llm_decoder_attention_plan in
    tests/test_decoder_fp8_gpu.py."""
    import llm_capi
    D, ts = 128, 16
    rng = np.random.default_rng(T)
    q, kb, vb, kf, vf, pt = _random_case(rng, B, H, D, T, ts)
    kd, vd = dev_fp8(kb), dev_fp8(vb)
    view = llm_capi.kv_view(kd, vd, _dev(pt))
    ns, got = ctypes.c_int32(), ctypes.c_int32()
    llm_capi.check(gpu.pa_decode_plan(ctypes.byref(view), B, H, D, T, pps, 1, ctypes.byref(ns),
                                      ctypes.byref(got)))
    assert got.value == form and (ns.value == 1) == (form == FORM_DIRECT), (ns.value, got.value)
    out = llm_capi.pa_decode(_dev(q), kd, vd, _dev(pt), T=T, pages_per_split=pps).cpu().numpy()
    assert_parity(out, oracle.paged_attention(q, kf, vf, pt, T=T), RTOL)


def test_kv_tile_cache_fp8(gpu, oracle, tmp_path):
    """KVTileCache.init(dtype="fp8"): raw bytes in, attention over them, and the
    three file formats round trip the bytes (no file holds a scale)."""
    import torch
    import llm_decoder
    import llm_capi
    rng = np.random.default_rng(2)
    H, D, TS, T = 2, 64, 16, 90
    kv = llm_decoder.KVTileCache()
    kv.init(num_pages=32, tile_size=TS, head_dim=D, num_layers=1, num_beams=1, num_heads=H,
            max_tiles=8, dtype="fp8")
    assert kv.view(0)["kv_dtype"] == llm_capi.LLM_FP8
    kb = llm_capi.fp8_encode((rng.standard_normal((T, H, D)) * 0.4).astype(np.float32))
    vb = llm_capi.fp8_encode(rng.standard_normal((T, H, D)).astype(np.float32))
    kv.write_tokens(0, 0, 0, kb, vb)
    kv.sync_page_table_to_gpu()
    q = (rng.standard_normal((1, H, D)) * 0.5).astype(np.float32)

    def run(cache):
        out = torch.empty((1, H, D), device="cuda")
        llm_decoder.paged_attention(cache.handle, 0, _dev(q).data_ptr(), out.data_ptr(), B=1, H=H,
                                    D=D, T=T)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    out = run(kv)
    nt = (T + TS - 1) // TS
    pt = np.arange(H * nt, dtype=np.int32).reshape(1, H, nt)
    kp = np.zeros((H * nt, TS, D), np.float32)
    vp = np.zeros_like(kp)
    kf, vf = ref_decode(kb), ref_decode(vb)
    for h in range(H):
        for t in range(T):
            kp[pt[0, h, t // TS], t % TS] = kf[t, h]
            vp[pt[0, h, t // TS], t % TS] = vf[t, h]
    assert_parity(out, oracle.paged_attention(q, kp, vp, pt, T=T), RTOL)
    snap = str(tmp_path / "fp8.kv")
    kv.save_to_file(snap, "snapshot")
    geo = (ctypes.c_longlong * 9)()
    llm_capi.check(gpu.kv_cache_inspect(snap.encode(), geo))
    assert geo[7] == llm_capi.LLM_FP8
    kv2 = llm_decoder.KVTileCache()
    kv2.init(num_pages=32, tile_size=TS, head_dim=D, num_layers=1, num_beams=1, num_heads=H,
             max_tiles=8, dtype="float8_e4m3fn")
    kv2.load_from_file(snap, "snapshot")
    kv2.sync_page_table_to_gpu()
    assert np.array_equal(run(kv2), out)
    f16 = llm_decoder.KVTileCache()
    f16.init(num_pages=32, tile_size=TS, head_dim=D, num_layers=1, num_beams=1, num_heads=H,
             max_tiles=8)
    with pytest.raises(RuntimeError):
        f16.load_from_file(snap, "snapshot")  # the file's kv_dtype differs
