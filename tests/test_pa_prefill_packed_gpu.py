"""Parity of the packed MFMA prefill attention (pa_prefill_packed, via the C
ABI): prompt chunks of several sequences, dense in q / out, in one launch
driven by a tile table.

Oracle: the CPU restatement run as a decode batch of the m packed rows, with
beam_ids = each row's page-table row and context_lens = its position + 1; the
tolerance is the single-sequence kernel's (tests/test_pa_prefill_gpu.py:
RTOL = 1e-3 relative, elementwise floor ATOL_FRAC = 4e-6 of the largest
|output|), for the split and the one-pass form.

Bit-equality: in the one-pass form a query's result does not depend on which
other queries share its tile (a key block past its own position leaves its
running max, sum and output bit-unchanged: corr = exp2(0), every p = 0), so
the packed one-pass output equals single-sequence pa_prefill(split=False) of
each segment bit for bit; on FP8 pools it equals the same call on fp16 pools
holding the decoded values, as the single-sequence kernel's does."""
import numpy as np
import pytest

from _fp8 import dev_fp8, fp8_pools
from _util import assert_parity

pytestmark = pytest.mark.gpu
RTOL = 1e-3
ATOL_FRAC = 4e-6
NAN_CODE = 0x7F

_D_ROWS = np.random.default_rng(64).permutation(64).tolist()
CASES = {
    "A": dict(H=4, D=64, ts=16, segs=[(2, 0, 5), (0, 0, 64), (1, 0, 17)]),
    # a long prefix beside short segments: some tiles skip splits
    "B": dict(H=3, D=128, ts=16, segs=[(1, 1000, 70), (3, 0, 1), (0, 37, 65), (2, 16, 16)]),
    "C": dict(H=2, D=128, ts=32, segs=[(0, 517, 96), (2, 31, 1), (1, 0, 33)]),
    # 64 short segments at one depth, rows in a shuffled order
    "D": dict(H=16, D=128, ts=16, segs=[(r, 120, 8) for r in _D_ROWS]),
}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tables(rng, segs, H, ts, num_rows, missing=0.0):
    """Page table [num_rows][H][max_tiles] with every row's own context mapped
    (rows not in segs map nothing) and the permutation of pages used."""
    ends = {r: p0 + n for r, p0, n in segs}
    mt = (max(ends.values()) + ts - 1) // ts + 2
    need = sum(H * ((e + ts - 1) // ts) for e in ends.values())
    num_pages = need + 7
    perm = rng.permutation(num_pages).astype(np.int32)
    pt = np.full((num_rows, H, mt), -1, np.int32)
    at = 0
    for r, e in ends.items():
        nt = (e + ts - 1) // ts
        pt[r, :, :nt] = perm[at:at + H * nt].reshape(H, nt)
        at += H * nt
    if missing:
        gone = (rng.random(pt.shape) < missing) & (pt >= 0)
        pt[gone] = -1
    return pt, num_pages, ends


def _case(rng, segs, H, D, ts, missing=0.0):
    """fp16 pools and a table as test_pa_prefill_gpu.py::_case builds them; the
    tokens past a row's context in its last page were never written: NaN."""
    num_rows = max(r for r, _, _ in segs) + 2
    pt, num_pages, ends = _tables(rng, segs, H, ts, num_rows, missing)
    kp = (rng.standard_normal((num_pages, ts, D)) * D ** -0.25).astype(np.float16)
    vp = rng.standard_normal((num_pages, ts, D)).astype(np.float16)
    for r, e in ends.items():
        if e % ts:
            for p in pt[r, :, (e - 1) // ts]:
                if p >= 0:
                    kp[p, e % ts:] = np.nan
                    vp[p, e % ts:] = np.nan
    return kp, vp, pt


def _rows_of(segs):
    beam = np.concatenate([np.full(n, r, np.int32) for r, _, n in segs])
    ctx = np.concatenate([np.arange(p0 + 1, p0 + n + 1, dtype=np.int32) for _, p0, n in segs])
    return beam, ctx


def _oracle(oracle, q, kf, vf, pt, segs, sm_scale=1.0):
    beam, ctx = _rows_of(segs)
    return oracle.paged_attention(q, kf, vf, pt, T=int(ctx.max()), beam_ids=beam,
                                  context_lens=ctx, temperature=sm_scale ** -0.5)


def _per_segment(llm_capi, q, kp, vp, pt, segs, **kw):
    """Single-sequence pa_prefill, one pass, segment by segment."""
    import torch
    outs, at = [], 0
    for r, p0, n in segs:
        outs.append(llm_capi.pa_prefill(q[at:at + n], kp, vp, pt, row=r, p0=p0, split=False, **kw))
        at += n
    return torch.cat(outs).cpu().numpy()


@pytest.fixture(scope="module")
def cases(gpu, oracle):
    """Inputs, the oracle's rows and the per-segment one-pass rows, once per case."""
    import llm_capi
    made = {}
    for name, c in CASES.items():
        rng = np.random.default_rng(ord(name))
        segs, H, D, ts = c["segs"], c["H"], c["D"], c["ts"]
        kp, vp, pt = _case(rng, segs, H, D, ts)
        m = sum(n for _, _, n in segs)
        q = (rng.standard_normal((m, H, D)) * D ** -0.25).astype(np.float32)
        dev = (_dev(q), _dev(kp), _dev(vp), _dev(pt))
        made[name] = dict(segs=segs, q=q, kp=kp, vp=vp, pt=pt, dev=dev,
                          ref=_oracle(oracle, q, kp.astype(np.float32), vp.astype(np.float32), pt,
                                      segs),
                          single=_per_segment(llm_capi, *dev, segs))
    return made


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", list(CASES))
def test_packed_vs_oracle(cases, name, split):
    import llm_capi
    c = cases[name]
    out = llm_capi.pa_prefill_packed(*c["dev"], segs=c["segs"], split=split).cpu().numpy()
    assert np.isfinite(out).all()
    assert_parity(out, c["ref"], RTOL, ATOL_FRAC)


@pytest.mark.parametrize("name", list(CASES))
def test_packed_one_pass_bit_equals_single_sequence(cases, name):
    import llm_capi
    c = cases[name]
    out = llm_capi.pa_prefill_packed(*c["dev"], segs=c["segs"], split=False).cpu().numpy()
    np.testing.assert_array_equal(out, c["single"])


def test_split_form_is_taken_and_skips(cases):
    """Case B plans several splits: its split = 1 workspace holds partials beyond
    the one-pass size, so test_packed_vs_oracle[B-True] ran the split form, with
    the short segments' tiles returning early from the splits past them."""
    import ctypes
    import llm_capi
    lib = llm_capi.load()
    c = cases["B"]
    view = llm_capi.kv_view(*c["dev"][1:])
    arr = llm_capi.prefill_segs(c["segs"])
    s0 = lib.pa_prefill_packed_workspace_bytes(ctypes.byref(view), arr, len(c["segs"]), 0)
    s1 = lib.pa_prefill_packed_workspace_bytes(ctypes.byref(view), arr, len(c["segs"]), 1)
    assert s1 > s0 > 0


@pytest.mark.parametrize("name", ["B", "D"])
def test_packed_fp8_pools(gpu, oracle, name):
    """FP8 pools (NaN codes past each context): the oracle on the decoded
    values, and bit-equal to the same call on fp16 pools holding them."""
    import llm_capi
    c = CASES[name]
    segs, H, D, ts = c["segs"], c["H"], c["D"], c["ts"]
    rng = np.random.default_rng(100 + ord(name))
    pt, num_pages, ends = _tables(rng, segs, H, ts, max(r for r, _, _ in segs) + 2)
    kb, vb, kf, vf = fp8_pools(rng, (num_pages, ts, D), D ** -0.25)
    for r, e in ends.items():
        if e % ts:
            for p in pt[r, :, (e - 1) // ts]:
                kb[p, e % ts:] = NAN_CODE
                vb[p, e % ts:] = NAN_CODE
                kf[p, e % ts:] = np.nan
                vf[p, e % ts:] = np.nan
    m = sum(n for _, _, n in segs)
    q = (rng.standard_normal((m, H, D)) * D ** -0.25).astype(np.float32)
    ref = _oracle(oracle, q, kf, vf, pt, segs)
    for split in (True, False):
        out = llm_capi.pa_prefill_packed(_dev(q), dev_fp8(kb), dev_fp8(vb), _dev(pt), segs=segs,
                                         split=split).cpu().numpy()
        assert np.isfinite(out).all()
        assert_parity(out, ref, RTOL, ATOL_FRAC)
        out16 = llm_capi.pa_prefill_packed(_dev(q), _dev(kf.astype(np.float16)),
                                           _dev(vf.astype(np.float16)), _dev(pt), segs=segs,
                                           split=split).cpu().numpy()
        np.testing.assert_array_equal(out, out16)


def test_packed_missing_pages_and_scale(gpu, oracle):
    """15 % of the pages missing under a spiky sm_scale, on case B's mix; then an
    all-missing segment beside a live one: zeros for its rows only."""
    import llm_capi
    c = CASES["B"]
    segs, H, D, ts = c["segs"], c["H"], c["D"], c["ts"]
    rng = np.random.default_rng(11)
    num_rows = max(r for r, _, _ in segs) + 2
    pt, num_pages, _ = _tables(rng, segs, H, ts, num_rows, missing=0.15)
    kp = (rng.standard_normal((num_pages, ts, D)) * D ** -0.25).astype(np.float16)
    vp = rng.standard_normal((num_pages, ts, D)).astype(np.float16)
    m = sum(n for _, _, n in segs)
    q = (rng.standard_normal((m, H, D)) * 2.0).astype(np.float32)
    ref = _oracle(oracle, q, kp.astype(np.float32), vp.astype(np.float32), pt, segs, sm_scale=0.5)
    for split in (True, False):
        out = llm_capi.pa_prefill_packed(_dev(q), _dev(kp), _dev(vp), _dev(pt), segs=segs,
                                         sm_scale=0.5, split=split).cpu().numpy()
        assert_parity(out, ref, RTOL, ATOL_FRAC)
    # segment (0, 37, 65) loses every page: rows 71 .. 135 of the packed output
    gone = pt.copy()
    gone[0] = -1
    ref = _oracle(oracle, q, kp.astype(np.float32), vp.astype(np.float32), gone, segs, sm_scale=0.5)
    for split in (True, False):
        out = llm_capi.pa_prefill_packed(_dev(q), _dev(kp), _dev(vp), _dev(gone), segs=segs,
                                         sm_scale=0.5, split=split).cpu().numpy()
        np.testing.assert_array_equal(out[71:136], np.zeros_like(out[71:136]))
        assert np.abs(out[:71]).max() > 0 and np.abs(out[136:]).max() > 0
        assert_parity(out, ref, RTOL, ATOL_FRAC)


def test_packed_strided_q(cases):
    """q read in place from [m][3 H D] rows (the decoder's qkv rows)."""
    import torch
    import llm_capi
    c = cases["A"]
    m, H, D = c["q"].shape
    wide = torch.full((m, 3 * H * D), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :H * D] = c["dev"][0].reshape(m, H * D)
    for split in (True, False):
        out = llm_capi.pa_prefill_packed(wide, *c["dev"][1:], segs=c["segs"],
                                         split=split).cpu().numpy()
        assert_parity(out, c["ref"], RTOL, ATOL_FRAC)
    np.testing.assert_array_equal(out, c["single"])


def test_packed_rejects_on_device_call(gpu):
    import llm_capi
    rng = np.random.default_rng(1)
    segs = [(0, 0, 20), (1, 0, 4)]
    kp, vp, pt = _case(rng, segs, 2, 32, 16)
    q = rng.standard_normal((24, 2, 32)).astype(np.float32)
    with pytest.raises(llm_capi.LlmError) as ei:   # head_dim 32
        llm_capi.pa_prefill_packed(_dev(q), _dev(kp), _dev(vp), _dev(pt), segs=segs)
    assert ei.value.status == llm_capi.LLM_ERR_UNSUPPORTED
    kp, vp, pt = _case(rng, segs, 2, 64, 16)
    q = rng.standard_normal((24, 2, 64)).astype(np.float32)
    with pytest.raises(llm_capi.LlmError) as ei:   # a repeated row
        llm_capi.pa_prefill_packed(_dev(q), _dev(kp), _dev(vp), _dev(pt),
                                   segs=[(0, 0, 20), (0, 20, 4)])
    assert ei.value.status == llm_capi.LLM_ERR_INVALID
