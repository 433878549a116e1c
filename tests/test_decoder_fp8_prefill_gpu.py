"""Prompt chunks of an FP8-KV decoder (kv_dtype="fp8") on the MFMA prefill
kernel: the chunk's K / V are appended as e4m3 bytes at the layer's scales and
pa_prefill reads them back, k_scale folded into the score multiplier and
v_scale applied to the normalised heads, in its split form (long prompts: the
merge applies v_scale) and its one-pass form (short prompts: the kernel does).

Reference: the same prompt fed one token per decode step (the decode kernel),
the comparison of tests/test_decoder_gpu.py (_prefill_vs_stepping) and
tests/test_decoder_fp8_gpu.py (test_prefill_equals_token_by_token), re-stated
here with scales and page readback."""
import numpy as np
import pytest

from _fp8 import NAN_CODES, Pages, f16_model, make_decoder
from _util import record, rel_err

pytestmark = pytest.mark.gpu
FREE_RUN_TOL = 2.5e-2  # the project's bar for prefill against stepping through int8 activations
# CUDADecoder (fp16 weights), FP8 KV, prefill against stepping.  On the parent
# commit, where both paths run the decode kernel, this test's body measured
# rel_err 2.457e-4 (530 tokens) and 5.167e-4 (20 tokens); PARENT_F16W_ERR is
# the worse row.  The bar is twice that (e4m3 boundary flips of the appended
# bytes are independent in the two paths) and not below the fp16-KV figure of
# test_prefill_mfma_fp16_decoder, 1e-3: 1.033e-3.  On the MFMA prefill the
# same rows measure 4.29e-4 and 5.17e-4.
PARENT_F16W_ERR = 5.166e-4
# The same body at F16W_SCALES on the parent commit: 2.818e-4 / 7.112e-4, bar
# 1.422e-3 by the same rule; on the MFMA prefill 3.95e-4 / 4.08e-4.  A prefill
# that drops v_scale measures 1.05e-2 / 3.6e-3 here (and stays under
# FREE_RUN_TOL in the INT8Decoder tests, whose attention output is a small part
# of the residual stream: 2.1e-2 / 1.8e-2), so this is the test that holds the
# V scale of both forms; a dropped k_scale moves the INT8 logits by 0.13 .. 0.44.
PARENT_F16W_SCALED_ERR = 7.112e-4
F16W_FLOOR = 1e-3


def _torch():
    import torch
    return torch


def _int8_model(oracle, L, H, D, V, S, seed):
    from oracle.oracle import synthetic_int8_model
    return synthetic_int8_model(oracle, L=L, H=H, D=D, V=V, max_seq=S, seed=seed)


def _code_ordinal(b):
    """e4m3 codes in value order (-0 and +0 both 0): adjacent values differ by 1."""
    m = (b & 0x7F).astype(np.int32)
    return np.where(b & 0x80, -m, m)


def _prefill_vs_stepping(make, prompts, V, L, want_bytes=True, kernel="mfma"):
    """A: each prompt one token per decode step, in a decoder of its own;
    B: prefill all but the last token of every prompt, then one step.
    Returns (logits A per row, logits B [rows][V], layer-0 context bytes of A
    per row, of B per row); checks context_len and NaN codes of B.  kernel:
    what B's prefill_kernel must report (None: not asked)."""
    torch = _torch()
    la, bytes_a = [], []
    for p in prompts:
        a = make(1)
        a.begin_synthetic(1, 0, 0, False)
        l1 = torch.empty((1, V), device="cuda")
        for t in p:
            a.step([t], logits_ptr=l1.data_ptr())
        torch.cuda.synchronize()
        la.append(l1[0].cpu().numpy().copy())
        if want_bytes:
            pg = Pages(a)
            bytes_a.append(pg.context(pg.pool(), 0, 1, len(p))[:, 0])
    b = make(len(prompts))
    assert kernel is None or b.prefill_kernel == kernel
    b.begin_synthetic(len(prompts), 0, 0, False)
    for r, p in enumerate(prompts):
        b.prefill(r, p[:-1])
    lb = torch.empty((len(prompts), V), device="cuda")
    b.step([p[-1] for p in prompts], logits_ptr=lb.data_ptr())
    torch.cuda.synchronize()
    bytes_b = []
    pg = Pages(b)
    pool = pg.pool()
    for r, p in enumerate(prompts):
        assert b.context_len(r) == len(p)  # tokens now in the row's KV
        for layer in range(L):
            got = pg.context(pool, layer, 1, len(p), row0=r)[:, 0]
            assert not np.isin(got, NAN_CODES).any(), (r, layer)
            if layer == 0:
                bytes_b.append(got)
    return la, lb.cpu().numpy(), bytes_a, bytes_b


def _check_int8(w, prompts, tag, scales=None, **kw):
    V, L = w["cfg"]["V"], w["cfg"]["L"]

    def make(n):
        dec = make_decoder(w, n, **kw)
        if scales:
            dec.set_kv_scales(*scales)
        return dec

    la, lb, bytes_a, bytes_b = _prefill_vs_stepping(make, prompts, V, L)
    for r in range(len(prompts)):
        err = rel_err(lb[r], la[r])
        diff = bytes_b[r] != bytes_a[r]
        share = float(diff.mean())
        step = np.abs(_code_ordinal(bytes_b[r][diff]) - _code_ordinal(bytes_a[r][diff]))
        record("kv_fp8", test=tag, row=r, scales=scales, layer0_byte_diff_share=share,
               max_code_step=int(step.max()) if step.size else 0, logit_err=err)
        print(f"{tag} row {r}: layer-0 bytes differing {share:.2e}, logits rel err {err:.2e}")
        assert np.isfinite(lb[r]).all()
        assert err < FREE_RUN_TOL, (r, err)
        # layer 0's pre-images depend on the token alone (the rule of
        # test_prefill_equals_token_by_token): int8 LN1 flips and rounding
        # boundaries move at most 1e-2 of the bytes, each by one code
        assert share <= 1e-2, (r, share)
        assert (step <= 1).all(), (r, step.max())


def test_prefill_kernel_reports_the_path(gpu, oracle):
    for D, want in ((64, "mfma"), (128, "mfma"), (256, "decode")):
        w = _int8_model(oracle, L=1, H=2, D=D, V=100, S=64, seed=2)
        assert make_decoder(w, 1).prefill_kernel == want, D
    w = _int8_model(oracle, L=1, H=2, D=64, V=100, S=64, seed=2)
    assert make_decoder(w, 1, kv_dtype="float16").prefill_kernel == "mfma"
    # the C entry
    import ctypes
    import llm_capi
    from _fp8 import DecoderConfig
    cfg = DecoderConfig(num_layers=1, num_heads=2, head_dim=128, hidden_dim=256, vocab_size=100,
                        max_seq_len=32, weight_dtype=llm_capi.LLM_I8, max_batch=1)
    h = ctypes.c_void_p()
    llm_capi.check(gpu.llm_decoder_create_kv(ctypes.byref(cfg), llm_capi.LLM_FP8, ctypes.byref(h)))
    assert gpu.llm_decoder_prefill_kernel(h) == 1  # LLM_PREFILL_MFMA
    gpu.llm_decoder_destroy(h)


@pytest.mark.parametrize("scales", [None, ([0.25, 0.5], [2.0, 4.0])], ids=["scale1", "scaled"])
def test_prefill_vs_stepping_int8(gpu, oracle, scales):
    """600 tokens: two chunks (512 + 87 prefilled), both in the split form (8
    and 10 splits); 9 tokens: the one-pass form.  The scales are powers of two in the
    exact range of tests/_fp8.py.  A dropped k_scale moves these logits by 0.13
    .. 0.44, far past the bar; a dropped v_scale by only ~2e-2 (measured on
    such builds), which test_prefill_vs_stepping_f16_weights_scaled holds."""
    w = _int8_model(oracle, L=2, H=4, D=64, V=500, S=1024, seed=12)
    rng = np.random.default_rng(3)
    prompts = [rng.integers(0, 500, 600).tolist(), rng.integers(0, 500, 9).tolist()]
    _check_int8(w, prompts, "prefill_mfma_int8_d64", scales)


def test_prefill_vs_stepping_int8_d128(gpu, oracle):
    w = _int8_model(oracle, L=1, H=2, D=128, V=300, S=256, seed=14)
    rng = np.random.default_rng(6)
    prompts = [rng.integers(0, 300, 100).tolist()]
    _check_int8(w, prompts, "prefill_mfma_int8_d128", page_size=16)


F16W_SCALES = ([0.25, 0.5], [2.0, 4.0])


def f16_weights_errs(kernel="mfma", scales=None):
    """The body of test_prefill_vs_stepping_f16_weights (scales: of its scaled
    twin): (logits B, rel_err per row of prefill + step against stepping)."""
    rng = np.random.default_rng(4)
    L, H, D, V, S = 2, 4, 64, 300, 700
    w = f16_model(rng, L, H, D, V, S)
    prompts = [rng.integers(0, V, 530).tolist(), rng.integers(0, V, 20).tolist()]

    def make(n):
        dec = make_decoder(w, n, cls="CUDADecoder")
        if scales:
            dec.set_kv_scales(*scales)
        return dec

    la, lb, _, _ = _prefill_vs_stepping(make, prompts, V, L, want_bytes=False, kernel=kernel)
    return lb, [rel_err(lb[r], la[r]) for r in range(2)]


def test_prefill_vs_stepping_f16_weights(gpu, oracle):
    """CUDADecoder with FP8 KV, D 64, L 2, prompts of 530 and 20 tokens: no int8
    activation amplifies a difference, so the two paths differ by the attention
    kernels' own error (~1e-6) and by e4m3 bytes of deeper layers that flip on
    a rounding boundary.  Parent commit (both paths on the decode kernel):
    2.457e-4 / 5.167e-4 for the two rows; bar max(2 x 5.166e-4, 1e-3) =
    1.033e-3, see PARENT_F16W_ERR above."""
    lb, errs = f16_weights_errs()
    record("kv_fp8", test="prefill_mfma_f16w", rel_err=errs)
    print(f"prefill_mfma_f16w rel_err {errs}")
    assert np.isfinite(lb).all()
    bar = max(2 * PARENT_F16W_ERR, F16W_FLOOR)
    for r in range(2):
        assert errs[r] < bar, (r, errs[r], bar)


def test_prefill_vs_stepping_f16_weights_scaled(gpu, oracle):
    """The same comparison at F16W_SCALES (k 0.25 / 0.5, v 2 / 4): the 530-token
    prompt takes the split form (the merge applies v_scale), the 20-token one
    the one-pass form (the kernel does).  Parent commit: 2.818e-4 / 7.112e-4;
    bar max(2 x 7.112e-4, 1e-3) = 1.422e-3, see PARENT_F16W_SCALED_ERR above."""
    lb, errs = f16_weights_errs(scales=F16W_SCALES)
    record("kv_fp8", test="prefill_mfma_f16w_scaled", rel_err=errs)
    print(f"prefill_mfma_f16w_scaled rel_err {errs}")
    assert np.isfinite(lb).all()
    bar = max(2 * PARENT_F16W_SCALED_ERR, F16W_FLOOR)
    for r in range(2):
        assert errs[r] < bar, (r, errs[r], bar)
