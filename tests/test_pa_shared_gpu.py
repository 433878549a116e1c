"""Parity of the shared-prefix decode attention (pa_decode_shared, via the C
ABI): groups of rows whose leading tiles map the same pages read them once, on
MFMA, and each row's other tiles go through the split kernel; one merge joins
the two.

Oracle: the CPU restatement (oracle.paged_attention) on the same rows, each
with its own page-table row and context.  The group kernel keeps pa_prefill's
arithmetic (q and p as fp16 hi + lo halves into v_mfma_f32_16x16x32_f16, log2
softmax), so the bars are tests/test_pa_prefill_gpu.py's, derived in its
docstring: 1e-3 relative, tensor-normalised and elementwise, with the
elementwise floor ATOL_FRAC = 4e-6 of the largest |output|; FP8 pools decode
exactly to fp16, so tests/test_pa_prefill_fp8_gpu.py holds them to the same.
Plain pa_decode on the same rows is held to the same bars."""
import numpy as np
import pytest

from _fp8 import dev_fp8
from _util import assert_parity
from test_pa_prefill_fp8_gpu import _case as _case_fp8
from test_pa_prefill_gpu import ATOL_FRAC, RTOL, _case, _dev

pytestmark = pytest.mark.gpu


def _shared_case(rng, *, fp8, H, D, ts, ctx, groups, missing=0.0):
    """Pools and table as _case builds them, then each group's page ids copied
    into its members' leading tiles, and NaN behind every row's context in its
    last (private) page.  Returns (device k, device v, k fp32, v fp32, table)."""
    B, T = len(ctx), max(ctx)
    if fp8:
        kp, vp, kf, vf, pt = _case_fp8(rng, rows=B, H=H, D=D, T=T, ts=ts, missing=missing)
    else:
        kp, vp, pt = _case(rng, rows=B, H=H, D=D, T=T, ts=ts, missing=missing)
        kf, vf = kp.astype(np.float32), vp.astype(np.float32)
    for rows, P in groups:
        pt[rows, :, :P] = pt[rows[0], :, :P]
    shared = {r: P for rows, P in groups for r in rows}
    for b, c in enumerate(ctx):
        if c % ts and c > shared.get(b, 0) * ts:
            for p in pt[b, :, c // ts]:
                if p >= 0:
                    for pool, bad in ((kp, 0x7F if fp8 else np.nan), (vp, 0x7F if fp8 else np.nan),
                                      (kf, np.nan), (vf, np.nan)):
                        pool[p, c % ts:] = bad
    up = dev_fp8 if fp8 else _dev
    return up(kp), up(vp), kf, vf, pt


_CTX64 = [256 + 1 + (7 * i) % 40 for i in range(64)]
CASES = {
    # G 2, P 1: the suffix ends mid-page, NaN behind it
    "g2_p1": dict(H=2, D=64, ts=16, ctx=[21, 25], groups=[([0, 1], 1)]),
    # ragged second / third query tiles; row 0 of the first is in no group
    "g17": dict(H=2, D=64, ts=16, ctx=[50 + i for i in range(18)],
                groups=[([17, 3, 9] + [i for i in range(1, 17) if i not in (3, 9)], 3)]),
    "g33": dict(H=1, D=128, ts=16, ctx=[33 + (5 * i) % 23 for i in range(33)],
                groups=[(list(range(33)), 2)]),
    # C3 heads, 64 rows: 4 query tiles x 16 heads, 8 key blocks = 2 key splits
    "g64_c3": dict(H=16, D=128, ts=16, ctx=_CTX64, groups=[(list(range(64)), 16)]),
    # two groups of different P, members neither adjacent nor ordered, rows 1 and
    # 4 ungrouped; row 5's context ends with its prefix (empty suffix), row 8's
    # suffix is several splits long
    "two_groups": dict(H=2, D=64, ts=16, ctx=[70, 40, 45, 90, 33, 32, 64, 37, 3300],
                       groups=[([7, 2, 5], 2), ([0, 8, 3, 6], 4)]),
    "page32": dict(H=2, D=128, ts=32, ctx=[100, 97, 130], groups=[([2, 0, 1], 3)]),
    "missing": dict(H=3, D=128, ts=16, ctx=[200, 230, 215, 222, 207], missing=0.15,
                    groups=[([0, 1, 2, 3, 4], 12)]),
    # spiky scores: a large sm_scale stresses the running-max rescale and the merges
    "scale": dict(H=3, D=128, ts=16, ctx=[300, 340, 321], groups=[([0, 1, 2], 18)],
                  q_std=2.0, sm_scale=0.5),
}


@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("name", list(CASES))
def test_pa_decode_shared_vs_oracle(gpu, oracle, name, fp8):
    import llm_capi
    c = dict(CASES[name])
    q_std, sm = c.pop("q_std", c["D"] ** -0.25), c.pop("sm_scale", 1.0)
    rng = np.random.default_rng(len(name) + 31 * c["D"])
    k, v, kf, vf, pt = _shared_case(rng, fp8=fp8, **c)
    ctx = np.array(c["ctx"], np.int32)
    B, T = len(ctx), int(ctx.max())
    q = (rng.standard_normal((B, c["H"], c["D"])) * q_std).astype(np.float32)
    out = llm_capi.pa_decode_shared(_dev(q), k, v, _dev(pt), T=T, groups=c["groups"],
                                    context_lens=_dev(ctx), sm_scale=sm).cpu().numpy()
    ref = oracle.paged_attention(q, kf, vf, pt, T=T, beam_ids=np.arange(B, dtype=np.int32),
                                 context_lens=ctx, temperature=sm ** -0.5)
    assert np.isfinite(out).all()
    assert_parity(out, ref, RTOL, ATOL_FRAC)
    dec = llm_capi.pa_decode(_dev(q), k, v, _dev(pt), T=T, context_lens=_dev(ctx), sm_scale=sm)
    assert_parity(out, dec.cpu().numpy(), RTOL, ATOL_FRAC)


@pytest.mark.parametrize("what", ["overlap", "pages_differ", "past_context", "one_row"])
def test_pa_decode_shared_refuses(gpu, what):
    import llm_capi
    rng = np.random.default_rng(2)
    ctx = [40, 40, 40, 20]
    k, v, _, _, pt = _shared_case(rng, fp8=False, H=2, D=64, ts=16, ctx=ctx, groups=[([0, 1, 3], 1)])
    groups = {"overlap": [([0, 1], 1), ([1, 3], 1)],
              "pages_differ": [([0, 1, 2], 1)],       # row 2 kept its own pages
              "past_context": [([0, 1, 3], 2)],       # row 3 holds 20 tokens: tile 1 is past them
              "one_row": [([0], 1)]}[what]
    q = rng.standard_normal((4, 2, 64)).astype(np.float32)
    with pytest.raises(llm_capi.LlmError) as ei:
        llm_capi.pa_decode_shared(_dev(q), k, v, _dev(pt), T=40, groups=groups,
                                  context_lens=_dev(np.array(ctx, np.int32)))
    assert ei.value.status == llm_capi.LLM_ERR_INVALID
