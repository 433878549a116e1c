"""RMSNorm on the device against float64 numpy of the header's formula
(include/llm_decoder.h, "RMSNorm"): the row launch, the weight GEMM's and the
gated kernel's prologues, and the decoder under set_norm("rms").

fp32 values: relative error |y - ref| / max(|ref|, 1e-3 max|ref|) within 4x
that of an fp32 numpy restatement on the same inputs (test_gemm_gated_gpu.py's
convention: the device's reduction order is not numpy's).  int8: within 1 LSB
of the float64 quantisation, at most 1 % of the elements off, the restatement
held to the same cap beside the device; row scales to 1e-6.  The prologues'
images and scales equal the launch's bit for bit, and the I8 products equal
i8_gemm / i8_gemm_gated on that image bit for bit.  Rows a prologue does not
take (_ln_fusable / _gated_fusable restate the host predicates) must be refused.
Prefill chunks are not tapped, so the launch form is tapped on INT8 decode rows
of hid 128 (no prologue there) and the prologue at hid 256; a prefilled prompt
is held to the same prompt stepped token by token."""
import numpy as np
import pytest

from _util import rel_err
from test_gemm_gated_gpu import _dev, _formula, _frag_off, _worst

pytestmark = pytest.mark.gpu
F, EPS = np.float32, 1e-5


def _rms(x, g, f):
    """The header's formula in float type f (float64: the reference)."""
    x = x.astype(f)
    ms = (x * x).sum(-1, keepdims=True, dtype=f) / f(x.shape[-1])
    inv = (1.0 / np.sqrt(ms + f(EPS)).astype(np.float64)).astype(f)
    return (x * inv) * g.astype(f)


def _quantise(y):
    y = y.astype(np.float64)
    scale = 127.0 / (np.abs(y).max(-1, keepdims=True) + 1e-6)
    t = y * scale
    return np.clip(np.sign(t) * np.floor(np.abs(t) + 0.5), -128, 127), 1.0 / scale[..., 0]


def _check_q(x, g, q, inv):
    ref, rinv = _quantise(_rms(x, g, np.float64))
    for name, got in (("fp32 numpy", _quantise(_rms(x, g, F))[0]), ("device", q.astype(np.float64))):
        d = np.abs(got - ref)
        print(f"int8 {name}: max LSB {d.max():.0f}, off {np.mean(d > 0):.4%}")
        assert d.max() <= 1 and np.mean(d > 0) <= 0.01, name
    np.testing.assert_allclose(inv, rinv, rtol=1e-6)


def _rows(rng, M, K):
    x = rng.standard_normal((M, K)).astype(F)
    if M >= 3:
        x[1] = 0  # a row of zeros, and one with a single large element
        x[2, K // 3] = 1e4
    return x, (1 + 0.1 * rng.standard_normal(K)).astype(F)


@pytest.mark.parametrize("cols", [64, 1024, 2048, 4096])
@pytest.mark.parametrize("rows", [1, 5])
def test_rmsnorm_rows(gpu, rows, cols):
    import llm_capi
    x, g = _rows(np.random.default_rng(rows * 7 + cols), rows, cols)
    out, q, s = (t.cpu().numpy() for t in llm_capi.rmsnorm_quant(_dev(x), _dev(g), EPS))
    ref = _rms(x, g, np.float64)
    base, err = max(_worst(_rms(x, g, F), ref), 2.0 ** -23), _worst(out, ref)
    print(f"rmsnorm {rows} x {cols}: fp32 numpy {base:.3e} device {err:.3e}")
    assert err <= 4 * base
    _check_q(x, g, q, s)


def _ln_fusable(i8, M, K):  # csrc/gemm.hip ln_fusable
    rows = 16 if M <= 16 else 32 if M <= 32 else 64
    return (K * (1 if i8 else 2)) % 256 == 0 and K <= 2048 and rows * K * 4 <= 64 * 1024


def _gated_fusable(i8, M, K):  # csrc/gemm_gated.hip gated_rms_fusable (N < 8192: one column tile)
    rows = 16 if M <= 16 else 32 if M <= 32 else 64
    return (M <= 64 and K <= 2048 and rows * K * 4 <= 64 * 1024
            and rows * K * (1 if i8 else 2) + rows * 4 <= 160 * 1024)


def _launch_image(x, g, i8):
    """rmsnorm_quant's image (int8, or fp16 bits of out) and scales, on the host."""
    import llm_capi
    out, q, s = (t.cpu().numpy() for t in llm_capi.rmsnorm_quant(_dev(x), _dev(g), EPS))
    return (q, s) if i8 else (out.astype(np.float16), None)


def _same_image(a_out, s_out, img, s, i8):
    M, K = img.shape
    kstep = 64 if i8 else 32
    got = a_out.cpu().numpy()[_frag_off(M, K, K // kstep, kstep)]
    np.testing.assert_array_equal(got.view(np.uint8 if i8 else np.uint16),
                                  img.view(np.uint8 if i8 else np.uint16))
    if i8:
        np.testing.assert_array_equal(s_out.cpu().numpy(), s)


# K 64 / 2048 and M 1 .. 64; K 256 / 1024 are the widths the weight GEMM's
# prologue takes at all; M 16 / 17 (K 1024) and 64 / 65 (K 64) are the two
# sides of the gated predicate's limits
GRID = [(M, K) for K in (64, 256, 1024, 2048) for M in (1, 16, 17, 64)] + [(65, 64)]


@pytest.mark.parametrize("dtype", ["i8", "f16"])
@pytest.mark.parametrize("N", [16, 48])
@pytest.mark.parametrize("M,K", GRID)
def test_gemm_rms_prologue(gpu, M, K, N, dtype):
    import llm_capi
    i8 = dtype == "i8"
    rng = np.random.default_rng(M * 131 + K + N)
    x, g = _rows(rng, M, K)
    bias = rng.standard_normal(N).astype(F)
    if i8:
        W, sw = rng.integers(-128, 128, (K, N), dtype=np.int8), rng.uniform(0.5, 1.5, N).astype(F)
    else:
        W, sw = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float16), None
    Wp = llm_capi.pack_weights(_dev(W), llm_capi.LLM_I8 if i8 else llm_capi.LLM_F16)
    kw = dict(f16=not i8, eps=EPS, bias=_dev(bias), sw=_dev(sw))
    if not _ln_fusable(i8, M, K):
        with pytest.raises(Exception, match="ln_fusable"):
            llm_capi.gemm_rms(_dev(x), _dev(g), Wp, N, **kw)
        return
    C, a_out, s_out = llm_capi.gemm_rms(_dev(x), _dev(g), Wp, N, **kw)
    img, s = _launch_image(x, g, i8)
    _same_image(a_out, s_out, img, s, i8)
    if i8:
        _, C2 = llm_capi.i8_gemm(_dev(img), Wp, N, sa=_dev(s), sw=_dev(sw), bias=_dev(bias))
        np.testing.assert_array_equal(C.cpu().numpy(), C2.cpu().numpy())
    else:
        ref = img.astype(np.float64) @ W.astype(np.float64) + bias
        base = max(_worst(img.astype(F) @ W.astype(F) + bias, ref), 2.0 ** -23)
        assert _worst(C.cpu().numpy(), ref) <= 4 * base


@pytest.mark.parametrize("dtype", ["i8", "f16"])
@pytest.mark.parametrize("N", [16, 48])
@pytest.mark.parametrize("M,K", GRID)
def test_gemm_gated_rms_prologue(gpu, M, K, N, dtype):
    import llm_capi
    i8 = dtype == "i8"
    rng = np.random.default_rng(M * 137 + K + N)
    x, g = _rows(rng, M, K)
    bg, bu = (rng.standard_normal(N).astype(F) for _ in range(2))
    if i8:
        Wg, Wu = (rng.integers(-128, 128, (K, N), dtype=np.int8) for _ in range(2))
        sws = [rng.uniform(0.5, 1.5, N).astype(F) * F(2 / (5400 * np.sqrt(K))) for _ in range(2)]
    else:
        Wg, Wu = ((rng.standard_normal((K, N)) * 1.5 / np.sqrt(K)).astype(np.float16)
                  for _ in range(2))
        sws = [None, None]
    Pg, Pu = (llm_capi.pack_weights(_dev(W), llm_capi.LLM_I8 if i8 else llm_capi.LLM_F16)
              for W in (Wg, Wu))
    kw = dict(sw_gate=_dev(sws[0]), sw_up=_dev(sws[1]), b_gate=_dev(bg), b_up=_dev(bu))
    if not _gated_fusable(i8, M, K):
        with pytest.raises(Exception, match="gated_rms_fusable"):
            llm_capi.gemm_gated_rms(_dev(x), _dev(g), Pg, Pu, N, f16=not i8, eps=EPS, **kw)
        return
    img, s = _launch_image(x, g, i8)
    for mlp in (llm_capi.LLM_MLP_GATED_SILU, llm_capi.LLM_MLP_GATED_GELU):
        ag, au, H, a_out, s_out = llm_capi.gemm_gated_rms(_dev(x), _dev(g), Pg, Pu, N, f16=not i8,
                                                          eps=EPS, mlp=mlp, **kw)
        _same_image(a_out, s_out, img, s, i8)
        if i8:
            rg, ru, rH, _ = llm_capi.gemm_gated(_dev(img), Pg, Pu, N, sa=_dev(s), mlp=mlp, **kw)
            for got, want in ((ag, rg), (au, ru), (H, rH)):
                np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
        else:
            g64, u64 = (img.astype(np.float64) @ W.astype(np.float64) for W in (Wg, Wu))
            g32, u32 = (img.astype(F) @ W.astype(F) for W in (Wg, Wu))
            ref = _formula(g64 + np.float64(bg), u64 + np.float64(bu), mlp, np.float64)
            base = max(_worst(_formula(g32 + bg, u32 + bu, mlp, F), ref), 2.0 ** -23)
            assert _worst(H.cpu().numpy(), ref) <= 4 * base, mlp


def _decoder(kind, H, mlp):
    """One layer, D 64, inter 256, V 512; (decoder, weights without any beta)."""
    import llm_decoder
    hid, inter, V = 64 * H, 256, 512
    rng = np.random.default_rng(11)
    dec = getattr(llm_decoder, "INT8Decoder" if kind == "i8" else "CUDADecoder")(
        1, H, 64, hid, V, 64, max_batch=1, inter_dim=inter)
    dec.set_norm("rms", eps=EPS)
    dec.set_mlp(mlp)
    w = {"emb": rng.standard_normal((V, hid)).astype(np.float16),
         "ln1_g": (1 + 0.1 * rng.standard_normal((1, hid))).astype(F),
         "ln2_g": (1 + 0.1 * rng.standard_normal((1, hid))).astype(F),
         "b1": (0.1 * rng.standard_normal((1, inter))).astype(F),
         "b2": (0.1 * rng.standard_normal((1, hid))).astype(F)}
    for k, (kk, n) in dict(wqkv=(hid, 3 * hid), wo=(hid, hid), w1=(hid, inter), w2=(inter, hid),
                           w_up=(hid, inter)).items():
        if kind == "i8":
            w[k] = rng.integers(-127, 128, (1, kk, n), dtype=np.int8)
            w[{"wqkv": "sw_qkv", "wo": "sw_o", "w1": "sw1", "w2": "sw2", "w_up": "sw_up"}[k]] = (
                rng.uniform(0.5, 1.5, (1, n)) * 0.05 / 127).astype(F)
        else:
            w[k] = (0.05 * rng.standard_normal((1, kk, n))).astype(np.float16)
    d = {k: (v.view(np.uint16) if v.dtype == np.float16 else v) for k, v in w.items()
         if mlp != "plain" or k not in ("w_up", "sw_up")}
    return dec, d, w


@pytest.mark.parametrize("mlp", ["plain", "gated_silu"])
def test_rms_decoder_f16_logits(gpu, mlp):
    """One token at position 0 (attention over a single key is V / (1 + 1e-6),
    the project's softmax), float64 numpy with the project's fp16 GEMM inputs."""
    import torch
    dec, d, w = _decoder("f16", 2, mlp)
    assert dec.norm() == "rms"
    dec.set_weights(d)  # no ln1_b / ln2_b
    with pytest.raises(Exception, match="before the weights"):
        dec.set_norm("layer")
    logits = torch.empty((1, 512), device="cuda")
    dec.begin_synthetic(1, 0, 0, False)
    dec.step([7], logits_ptr=logits.data_ptr())
    torch.cuda.synchronize()
    f16 = lambda a: np.asarray(a, F).astype(np.float16).astype(np.float64)
    m = {k: v[0].astype(np.float64) for k, v in w.items() if k != "emb"}
    x = w["emb"][7].astype(np.float64)[None, :]
    v = f16(f16(_rms(x, m["ln1_g"], np.float64)) @ m["wqkv"])[:, 256:]
    x = f16(v / (1 + 1e-6)) @ m["wo"]
    a = f16(_rms(x, m["ln2_g"], np.float64))
    if mlp == "plain":
        h = np.maximum(a @ m["w1"] + m["b1"], 0)
    else:
        h = _formula(a @ m["w1"] + m["b1"], a @ m["w_up"], 1, np.float64)
    x = f16(h) @ m["w2"] + m["b2"]
    assert rel_err(logits.cpu().numpy(), x @ w["emb"].astype(np.float64).T) < 1e-3


@pytest.mark.parametrize("mlp", ["plain", "gated_silu"])
@pytest.mark.parametrize("H", [2, 4])  # hid 128: the launch reads E[token]; 256: the qkv prologue
def test_rms_decoder_i8_tap(gpu, H, mlp):
    import torch
    from oracle.oracle import unpack_a_i8
    dec, d, w = _decoder("i8", H, mlp)
    dec.set_weights(d)
    hid = 64 * H
    tq = torch.zeros(4 * 16 * max(hid, 256), dtype=torch.int8, device="cuda")
    ts = torch.zeros(4, dtype=torch.float32, device="cuda")
    dec.set_taps(tq.data_ptr(), ts.data_ptr())
    logits, ref = torch.empty((1, 512), device="cuda"), torch.empty((1, 512), device="cuda")
    dec.begin_synthetic(1, 0, 0, False)
    dec.step([7], logits_ptr=logits.data_ptr())
    torch.cuda.synchronize()
    q = unpack_a_i8(tq.cpu().numpy()[:16 * hid], 1, hid)
    _check_q(w["emb"][7].astype(F)[None, :], w["ln1_g"][0], q, ts.cpu().numpy()[:1])
    # the launch form on a prompt chunk against the same prompt stepped
    dec.set_taps(0, 0)
    prompt = [3, 1, 4, 1, 5, 9, 2, 6]
    dec.begin_synthetic(1, 0, 0, False)
    for t in prompt:
        dec.step([t])
    dec.step([7], logits_ptr=ref.data_ptr())
    dec.begin_synthetic(1, 0, 0, False)
    dec.prefill(0, prompt)
    dec.step([7], logits_ptr=logits.data_ptr())
    torch.cuda.synchronize()
    assert rel_err(logits.cpu().numpy(), ref.cpu().numpy()) < 1e-3
