"""CPU checks of the FP8 (OCP e4m3fn) KV element type: the host codec
(llm_fp8_e4m3_encode / _decode) pins the format against torch byte for byte,
and the host-side refusals happen before any device call.

Format (include/llm_decoder.h): byte = e4m3_rne(clamp(y / scale, -448, 448)),
value = decode(byte) * scale; NaN = 0x7F / 0xFF, no infinities."""
import ctypes

import numpy as np

from _fp8 import DecoderConfig, NAN_CODES, boundary_sensitive, ref_decode, ref_encode

CODES = np.arange(256, dtype=np.uint8)


def test_decode_all_codes_equals_torch():
    import llm_capi
    got = llm_capi.fp8_decode(CODES)
    want = ref_decode(CODES)
    assert np.isnan(got[list(NAN_CODES)]).all()
    assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert got[0x7E] == 448.0 and got[0xFE] == -448.0 and got[0x01] == 2.0 ** -9
    # scale is applied after the decode
    assert np.array_equal(llm_capi.fp8_decode(CODES[:0x7F], 3.0), want[:0x7F] * np.float32(3.0))


def _check(x, scale=1.0):
    import llm_capi
    x = np.asarray(x, np.float32)
    got, want = llm_capi.fp8_encode(x, scale), ref_encode(x, scale)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (scale, x[bad[:5]], got[bad[:5]], want[bad[:5]])
    return got


def test_encode_equals_torch_reference():
    finite = np.array([c for c in range(256) if c not in NAN_CODES], np.uint8)
    vals = ref_decode(finite)
    # every code value encodes to itself (-0 keeps its sign)
    assert np.array_equal(_check(vals), finite)
    # every midpoint between adjacent codes: ties to even
    pos = np.sort(vals[vals >= 0])
    mids = ((pos[:-1].astype(np.float64) + pos[1:]) / 2).astype(np.float32)
    assert np.array_equal(mids.astype(np.float64), (pos[:-1].astype(np.float64) + pos[1:]) / 2)
    even = _check(mids)
    assert ((even & 1) == 0).all()
    assert ((_check(-mids) & 0x7F) == even).all()
    # one fp32 ulp either side of every midpoint rounds to the nearer code
    up, dn = np.nextafter(mids, np.float32(np.inf)), np.nextafter(mids, np.float32(0))
    assert np.array_equal(ref_decode(_check(up)), pos[1:])
    assert np.array_equal(ref_decode(_check(dn)), pos[:-1])
    # +-0
    assert list(_check([0.0, -0.0])) == [0x00, 0x80]
    # beyond +-448: saturates (torch alone would give NaN: the clamp is explicit)
    big = np.array([448.0, 449.0, 464.0, 480.0, 500.0, 1e4, 3.4e38, np.inf], np.float32)
    assert (_check(big) == 0x7E).all() and (_check(-big) == 0xFE).all()
    # subnormals below 2^-9 and around the subnormal steps
    tiny = np.array([2.0 ** -9, 2.0 ** -10, np.nextafter(np.float32(2.0 ** -10), np.float32(1)),
                     2.0 ** -11, 1e-30, 1e-45, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 7.5 * 2.0 ** -9,
                     2.0 ** -6, np.nextafter(np.float32(2.0 ** -6), np.float32(0))], np.float32)
    got = _check(np.concatenate([tiny, -tiny]))
    assert got[1] == 0 and got[2] == 1  # half the smallest subnormal ties to zero
    # NaN stays NaN
    import llm_capi
    assert (llm_capi.fp8_encode(np.array([np.nan], np.float32)) & 0x7F == 0x7F).all()
    # seeded normals over the whole range, three scales
    rng = np.random.default_rng(8)
    x = (rng.standard_normal(100_000) * np.exp(rng.uniform(-12, 7, 100_000))).astype(np.float32)
    for scale in (0.25, 1.0, 3.0):
        _check(x, scale)
        _check(rng.standard_normal(100_000).astype(np.float32), scale)


def test_boundary_rule_leaves_slack_for_the_reference():
    """The append-byte tests allow a byte to differ only where the reference
    byte itself changes within one fp32 ulp of the pre-image, and cap those at
    1e-4 of the bytes.  An fp32 value lies within an ulp of an e4m3 rounding
    boundary about once in 2^20 / 2 values (2 ulps of 2^-23 against a spacing of
    2^-3 .. 2^-4 relative), so the reference alone stays an order of magnitude
    under the cap."""
    rng = np.random.default_rng(9)
    pre = rng.standard_normal(2_000_000).astype(np.float32)
    for scale in (1.0, 0.3, 2.0 ** -4):
        frac = boundary_sensitive(pre, scale).mean()
        assert frac <= 1e-5, (scale, frac)


def test_host_side_refusals():
    """Decided on the host before any device call (fake pointers)."""
    import llm_capi
    lib = llm_capi.load()
    # a page must be 1..16 KiB: D 32 x 16 tokens of one byte is 512 B
    fake = llm_capi.PaKvView(k_pool=1, v_pool=1, page_table=1, num_pages=1, page_size=16,
                             head_dim=32, num_beams=1, num_heads=1, max_tiles=1,
                             kv_dtype=llm_capi.LLM_FP8)
    args = (ctypes.c_void_p(1), ctypes.c_void_p(1), None, None, 1, 1, 32, 16, 1.0, 0, None, 0, None)
    assert lib.pa_decode(ctypes.byref(fake), *args) == llm_capi.LLM_ERR_UNSUPPORTED
    ns, form = ctypes.c_int32(), ctypes.c_int32()
    assert lib.pa_decode_plan(ctypes.byref(fake), 1, 1, 32, 16, 0, 1, ctypes.byref(ns),
                              ctypes.byref(form)) == llm_capi.LLM_ERR_UNSUPPORTED
    # the decoder takes fp16 or fp8 pools only
    cfg = DecoderConfig(num_layers=1, num_heads=2, head_dim=64, hidden_dim=128, vocab_size=100,
                        max_seq_len=32, weight_dtype=llm_capi.LLM_I8, max_batch=1)
    out = ctypes.c_void_p()
    rc = lib.llm_decoder_create_kv(ctypes.byref(cfg), llm_capi.LLM_BF16, ctypes.byref(out))
    assert rc == llm_capi.LLM_ERR_UNSUPPORTED and not out.value
    rc = lib.llm_decoder_create_kv(ctypes.byref(cfg), 9, ctypes.byref(out))
    assert rc == llm_capi.LLM_ERR_INVALID and not out.value
    assert b"kv_dtype" in lib.llm_last_error()
    # the codec refuses a scale that is not finite and positive
    x = np.zeros(1, np.float32)
    b = np.zeros(1, np.uint8)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.llm_fp8_e4m3_encode(x.ctypes.data, 1, bad, b.ctypes.data) == 1
        assert lib.llm_fp8_e4m3_decode(b.ctypes.data, 1, bad, x.ctypes.data) == 1


def test_python_surface():
    import llm_decoder
    import torch
    import llm_capi
    assert llm_capi.LLM_FP8 == 4
    assert llm_capi.kv_dtype_of(torch.empty(0, dtype=torch.float8_e4m3fn)) == llm_capi.LLM_FP8
    for cls in (llm_decoder.CUDADecoder, llm_decoder.INT8Decoder):
        assert hasattr(cls, "set_kv_scales") and hasattr(cls, "kv_dtype")
