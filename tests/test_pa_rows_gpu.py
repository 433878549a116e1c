"""The attention launches' row outputs (the o_proj input) against the oracle.

Every decoder layer runs one attention launch that returns, not the fp32
[B][H][D] of pa_decode / pa_prefill, but per-row int8 + inv_scale or fp16 rows,
usually in packed-A order (PaRowOutputs, PaOut::{ROW_Q, ROW_F16, F32_ROWS} of
pa_decode_internal, pa_prefill_internal and the packed prefill).  Through
pa_rows_tune of the tuning build (csrc/tune/pa_decode_tune.hip), which calls
those entries unchanged, each form is run on the smallest shape that keeps its
path live and checked in two stages:

 1. the fp32 rows (keep_out = 1, or F32_ROWS) against oracle.paged_attention
    over the pool's exact values (times out_scale in float64; windows through
    tests/_window.py), at the public entries' bars: RTOL 1e-3, elementwise
    floor 1e-6 (decode) / 4e-6 (prefill, test_pa_prefill_gpu.py derives it);
 2. no tolerance: q8 / inv_scale equal oracle.quantize_rows of those fp32
    rows and out16 equals their fp16 rounding, bit for bit; the padding rows
    of a packed buffer keep their pre-fill; a keep_out = 0 run (out = NULL
    where the entry allows: the decoder's setting, and the dword-store
    quantiser's) gives the same bits; the workgroup merge and split + merge at
    the same split count give the same bits (LLM_WG_MERGE, per launch).

Every decode case asserts the form and split count the launch reported.

Measured stage-1 rel_err (profiles/pa_rows.jsonl, 152 launches): decode
5e-8 .. 1.2e-6 (the largest at 70 splits), prefill 1e-7 .. 1.8e-6; the worst
element stands at 0.07 (decode) and 0.11 (prefill) of its elementwise bound."""
import contextlib
import functools
import os
import types

import numpy as np
import pytest

import _pa_rows as pr
from _fp8 import (FORM_BEAM, FORM_DIRECT, FORM_SPLIT_MERGE, FORM_SPLIT_MERGE_ROW, FORM_WG_MERGE,
                  dev_fp8)
from _util import assert_parity, elem_err, record, rel_err
from _window import window_reference

pytestmark = pytest.mark.gpu
RTOL = 1e-3
ATOL_DECODE = 1e-6   # test_pa_decode_gpu.py, test_pa_decode_fp8_gpu.py
ATOL_PREFILL = 4e-6  # test_pa_prefill_gpu.py
ROW_Q, ROW_F16, F32_ROWS = 1, 2, 3  # llm_capi.PA_OUT_*
KIND = {ROW_Q: "row_q", ROW_F16: "row_f16", F32_ROWS: "f32_rows"}
# FP8 pools: the layer's V scale, and K's folded into the score multiplier
# (0.25 = temperature 2 exactly, for the oracle)
FP8_OUT_SCALE, FP8_SM_SCALE = 0.37, 0.25


@pytest.fixture(scope="module")
def tune(gpu):
    import llm_capi
    return llm_capi.load_tune()


def _dev(a):
    import torch
    if isinstance(a, torch.Tensor):
        return a.cuda()
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@contextlib.contextmanager
def _env(**kv):
    """The tuning build's per-launch switches, set and restored."""
    for k, v in kv.items():
        if v is not None:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k in kv:
            os.environ.pop(k, None)


@functools.lru_cache(maxsize=None)
def _case(rows, H, D, T, ts, kv="f16", groups=False):
    """Pools of element type kv behind a shuffled page table of `rows` rows
    (garbage in the unused pages), on the device and as the fp32 values the
    kernels read; q for a decode launch of `rows` rows."""
    rng = np.random.default_rng([rows, H, D, T, ts, len(kv), ord(kv[0])])
    pt, num_pages, unused = pr.page_table(rng, rows, H, T, ts, shared_groups=groups)
    kh, kf = pr.pool_values(rng, kv, (num_pages, ts, D), D ** -0.25, unused)
    vh, vf = pr.pool_values(rng, kv, (num_pages, ts, D), 1.0, unused)
    up = dev_fp8 if kv == "fp8" else _dev
    qs = 0.1 if kv == "i8" else 2 * D ** -0.25 if kv == "fp8" else D ** -0.25
    q = (rng.standard_normal((rows, H, D)) * qs).astype(np.float32)
    return types.SimpleNamespace(rows=rows, H=H, D=D, T=T, ts=ts, kv=kv, hid=H * D, pt=pt, kf=kf,
                                 vf=vf, q=q, kd=up(kh), vd=up(vh), ptd=_dev(pt), qd=_dev(q))


def _scales(c):
    return (FP8_SM_SCALE, FP8_OUT_SCALE) if c.kv == "fp8" else (1.0, 1.0)


def _lens(c, B=None):
    """Ragged contexts: the whole table, none, one token, one below a page
    boundary, fewer tokens than a page, and some in between."""
    B = B or c.rows
    base = [c.T, 0, 1, 2 * c.ts - 1, 5, c.T // 2 + 3, c.T - c.ts, c.ts]
    return np.array(base[:B], np.int32)


def _bits_equal(a, b, keys, what):
    import torch
    for k in keys:
        x, y = a[k], b[k]
        assert (x is None) == (y is None), (what, k)
        if x is not None:
            if x.dtype == torch.float32:
                x, y = x.view(torch.int32), y.view(torch.int32)
            assert torch.equal(x, y), f"{what}: {k} differs ({int((x != y).sum())} elements)"


def _np(t):
    return None if t is None else t.cpu().numpy()


def _stage1(res, ref, atol, what):
    assert res["status"] == 0, (what, res["error"])
    out = _np(res["out"])
    assert np.isfinite(out).all(), f"{what}: fp32 rows not all written"
    err, eerr = rel_err(out, ref), elem_err(out, ref, RTOL, atol)
    print(f"{what}: rel_err {err:.3e} elem {eerr:.3f}")
    record("pa_rows", case=what, rel_err=err, elem_err=eerr)
    assert_parity(out, ref, RTOL, atol, what=what)
    return out


def _stage2(oracle, res, out, pack, what):
    pr.check_conversions(oracle.quantize_rows, out, q8=_np(res["q8"]),
                         inv_scale=_np(res["inv_scale"]), out16=_np(res["out16"]), pack=pack,
                         what=what)


# ---------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------
_refs = {}


def _decode_ref(oracle, c, lens, beam_ids, window):
    key = (id(c), lens.tobytes(), beam_ids.tobytes(), window)
    if key not in _refs:
        sm, osc = _scales(c)
        q = c.q[:len(lens)]
        if window:
            r = window_reference(oracle, q, c.kf, c.vf, c.pt, lens, window, beam_ids,
                                 temperature=sm ** -0.5)
        else:
            r = oracle.paged_attention(q, c.kf, c.vf, c.pt, T=c.T, beam_ids=beam_ids,
                                       context_lens=lens, temperature=sm ** -0.5)
        _refs[key] = pr.rows_ref(r, osc)
    return _refs[key]


def _decode(c, lens, beam_ids, kind, pps, *, pack=1, keep_out=1, want_out=True, window=0,
            row_group=1, wg_merge=None):
    import llm_capi
    sm, osc = _scales(c)
    with _env(LLM_WG_MERGE=wg_merge, LLM_WGM_SPLITS=None if wg_merge is None else 0):
        return llm_capi.pa_rows(c.qd[:len(lens)], c.kd, c.vd, c.ptd, launch="decode",
                                out_kind=kind, T=c.T, beam_ids=_dev(beam_ids),
                                context_lens=_dev(lens), pages_per_split=pps, row_group=row_group,
                                sm_scale=sm, window=window, pack=pack, keep_out=keep_out,
                                out_scale=osc, want_out=want_out)


def _decode_check(oracle, c, kind, pps, ns, form, *, pack=1, window=0, row_group=1,
                  wg_merge=None, lens=None, beam_ids=None, what=""):
    """Both stages of one decode request in the form it must report; returns
    the keep_out = 1 result."""
    lens = _lens(c) if lens is None else lens
    B = len(lens)
    if beam_ids is None:  # rows permuted: launch row b reads page-table row B - 1 - b
        beam_ids = np.arange(B - 1, -1, -1, dtype=np.int32)
    what = (f"decode {what} {c.kv} H{c.H} D{c.D} ts{c.ts} T{c.T} pps{pps} {KIND[kind]}"
            f" pack{pack} w{window} ns{ns} form{form}")
    ref = _decode_ref(oracle, c, lens, beam_ids, window)
    kw = dict(pack=pack, window=window, row_group=row_group, wg_merge=wg_merge)
    r1 = _decode(c, lens, beam_ids, kind, pps, **kw)
    assert (r1["nsplit"], r1["form"]) == (ns, form), (what, r1["nsplit"], r1["form"])
    out = _stage1(r1, ref, ATOL_DECODE, what)
    np.testing.assert_array_equal(out[lens == 0], 0.0)  # empty context -> zeros
    _stage2(oracle, r1, out, pack, what)
    if kind != F32_ROWS:
        # the decoder's setting; a single split converts `out`, so it stays
        r0 = _decode(c, lens, beam_ids, kind, pps, keep_out=0, want_out=form == FORM_DIRECT, **kw)
        assert (r0["status"], r0["nsplit"], r0["form"]) == (0, ns, form), (what, r0["error"])
        _bits_equal(r1, r0, ("q8", "inv_scale", "out16"), what + " keep_out 0")
    return r1


def _wgm_and_split(oracle, c, kind, pps, ns, *, pack=1, window=0, what=""):
    """The same request as workgroup merge and as split + merge(-row) at the
    same split count: both stages on each, and the same bits between them."""
    off_form = FORM_SPLIT_MERGE if kind == F32_ROWS else FORM_SPLIT_MERGE_ROW
    on = _decode_check(oracle, c, kind, pps, ns, FORM_WG_MERGE, pack=pack, window=window,
                       wg_merge=1, what=what)
    off = _decode_check(oracle, c, kind, pps, ns, off_form, pack=pack, window=window,
                        wg_merge=0, what=what)
    _bits_equal(on, off, ("out", "out16"), f"{what} {KIND[kind]} pps{pps} wgm vs split")


@pytest.mark.parametrize("pack", [0, 1])
@pytest.mark.parametrize("kind", [ROW_Q, ROW_F16])
def test_merge_row_past_the_first_batch(gpu, tune, oracle, kind, pack):
    """19 splits: the 8-split first round of pa_merge_row_kernel and two rounds
    of its long-split tail; the ragged rows hold 0, 1, 2, 10 and 19 of them."""
    _decode_check(oracle, _case(6, 4, 64, 300, 16), kind, 1, 19, FORM_SPLIT_MERGE_ROW, pack=pack)


def test_merge_row_second_weight_register(gpu, tune, oracle):
    """70 splits: the weights of splits 64 .. 69 come from the merge lanes'
    second register; the 1039-token row ends in split 64.  (Three rows, so the
    contexts 1 and 5 are left to the other cases.)"""
    c = _case(3, 2, 128, 1120, 16)
    _decode_check(oracle, c, ROW_Q, 1, 70, FORM_SPLIT_MERGE_ROW,
                  lens=np.array([1120, 0, 16 * 65 - 1], np.int32))


@pytest.mark.parametrize("kind", [ROW_Q, ROW_F16])
def test_merge_row_heads_loop(gpu, tune, oracle, kind):
    """20 heads on the merge's 16 waves: waves 0 .. 3 take a second head."""
    _decode_check(oracle, _case(6, 20, 32, 257, 32), kind, 2, 5, FORM_SPLIT_MERGE_ROW,
                  wg_merge=0)


def test_merge_row_scalar_quantiser_unpacked(gpu, tune, oracle):
    """hid = 96: no packed order, no dword stores, row-major int8."""
    _decode_check(oracle, _case(6, 3, 32, 300, 16), ROW_Q, 4, 5, FORM_SPLIT_MERGE_ROW, pack=0)


def test_d256_rows(gpu, tune, oracle):
    """D = 256 (four output dims per merge lane), packed fp16 rows, 4 splits:
    the workgroup merge by default, split + merge-row with it switched off."""
    _wgm_and_split(oracle, _case(6, 2, 256, 200, 16), ROW_F16, 4, 4, what="d256")


@pytest.mark.parametrize("kind", [ROW_Q, ROW_F16])
def test_direct_and_conversion_launches(gpu, tune, oracle, kind):
    """One split: the split kernel writes the final fp32 rows and
    launch_quantize_rows / launch_to_f16 convert them."""
    _decode_check(oracle, _case(6, 4, 64, 40, 16), kind, 128, 1, FORM_DIRECT)


@pytest.mark.parametrize("pps", [8, 3])
@pytest.mark.parametrize("H,D,ts", [(4, 64, 16), (2, 128, 16), (2, 256, 16), (2, 128, 32)],
                         ids=["d64", "d128", "d256", "d128_page32"])
def test_workgroup_merge(gpu, tune, oracle, H, D, ts, pps):
    """pa_split_kernel's C.wgm epilogue: fp16 rows unpacked and packed and
    fp32 rows, 3 and 7 splits (page 32: 2 and 4); the rows of context 0, 1 and
    5 have fewer live splits than the workgroup has waves."""
    c = _case(6, H, D, 300, ts)
    ns = -(-(-(-300 // ts)) // pps)
    assert ns == {(16, 8): 3, (16, 3): 7, (32, 8): 2, (32, 3): 4}[ts, pps]
    for kind, pack in ((ROW_F16, 0), (ROW_F16, 1), (F32_ROWS, 0)):
        _wgm_and_split(oracle, c, kind, pps, ns, pack=pack, what="wgm")


@pytest.mark.parametrize("kind", [ROW_Q, ROW_F16])
def test_beam_groups(gpu, tune, oracle, kind):
    """row_group 4: two groups of 4 rows over forked page-table rows (a shared
    prefix of 9 tiles), the first with equal contexts (the shared LDS path),
    the second ragged; fixed splits and the form's own dynamic (interleaved)
    splits -- 19 tiles give 3 whatever the chip's occupancy (choose_nsplit:
    at least kMinPps = 8 pages per split)."""
    c = _case(8, 4, 64, 300, 16, groups=True)
    lens = np.array([300, 300, 300, 300, 0, 1, 31, 300], np.int32)
    beam_ids = np.array([5, 4, 7, 6, 1, 0, 3, 2], np.int32)
    for pps, ns in ((4, 5), (0, 3)):
        _decode_check(oracle, c, kind, pps, ns, FORM_SPLIT_MERGE_ROW | FORM_BEAM, row_group=4,
                      lens=lens, beam_ids=beam_ids, what="beam")


@pytest.mark.parametrize("window", [5, 40])
def test_window(gpu, tune, oracle, window):
    """A window touches (W - 1) / 16 + 2 tiles: 2 and 4 splits of one page,
    counted from each row's own first live tile, in the merge-row launch and
    in the workgroup merge."""
    c = _case(6, 4, 64, 300, 16)
    ns = (window - 1) // 16 + 2
    _decode_check(oracle, c, ROW_Q, 1, ns, FORM_SPLIT_MERGE_ROW, window=window, what="window")
    _wgm_and_split(oracle, c, ROW_F16, 1, ns, window=window, what="window")


@pytest.mark.parametrize("kv", ["bf16", "i8"])
def test_other_kv_types(gpu, tune, oracle, kv):
    _decode_check(oracle, _case(6, 4, 64, 300, 16, kv), ROW_Q, 1, 19, FORM_SPLIT_MERGE_ROW)


# --- FP8 pools: out_scale reaches every form --------------------------------
@pytest.mark.parametrize("H,D,ts", [(4, 64, 16), (2, 128, 16), (4, 64, 32)],
                         ids=["d64", "d128", "d64_page32"])
def test_fp8_workgroup_merge(gpu, tune, oracle, H, D, ts):
    c = _case(6, H, D, 300, ts, "fp8")
    _wgm_and_split(oracle, c, F32_ROWS, 8, 3 if ts == 16 else 2, pack=0, what="fp8 wgm")


def test_fp8_workgroup_merge_window(gpu, tune, oracle):
    _wgm_and_split(oracle, _case(6, 2, 128, 300, 16, "fp8"), F32_ROWS, 1, 4, pack=0, window=40,
                   what="fp8 wgm")


@pytest.mark.parametrize("H,D,ts", [(2, 128, 32), (2, 256, 16)], ids=["d128_page32", "d256"])
@pytest.mark.parametrize("window", [0, 40])
def test_fp8_split_merge_where_the_workgroup_form_is_not_built(gpu, tune, oracle, H, D, ts,
                                                               window):
    """fp8_wgm_shape_ok is false: fp32 rows keep split + pa_merge_kernel."""
    c = _case(6, H, D, 300, ts, "fp8")
    pps, ns = (1, (window - 1) // ts + 2) if window else (8, -(-(-(-300 // ts)) // 8))
    _decode_check(oracle, c, F32_ROWS, pps, ns, FORM_SPLIT_MERGE, pack=0, window=window,
                  what="fp8")


@pytest.mark.parametrize("window", [0, 40])
def test_fp8_merge_row_f16(gpu, tune, oracle, window):
    """fp16 rows from FP8 pages never merge in the workgroup."""
    c = _case(6, 2, 128, 300, 16, "fp8")
    pps, ns = (1, 4) if window else (8, 3)
    _decode_check(oracle, c, ROW_F16, pps, ns, FORM_SPLIT_MERGE_ROW, window=window, what="fp8")


@pytest.mark.parametrize("window", [0, 5])
def test_fp8_direct_row_q(gpu, tune, oracle, window):
    _decode_check(oracle, _case(6, 4, 64, 40, 16, "fp8"), ROW_Q, 128, 1, FORM_DIRECT,
                  window=window, what="fp8")


# ---------------------------------------------------------------------------
# prefill
# ---------------------------------------------------------------------------
def _prefill_ref(oracle, c, q, beam, ctx, window):
    sm, osc = _scales(c)
    if window:
        r = window_reference(oracle, q, c.kf, c.vf, c.pt, ctx, window, beam,
                             temperature=sm ** -0.5)
    else:
        r = oracle.paged_attention(q, c.kf, c.vf, c.pt, T=int(ctx.max()), beam_ids=beam,
                                   context_lens=ctx, temperature=sm ** -0.5)
    return pr.rows_ref(r, osc)


def _queries(c, m, seed):
    rng = np.random.default_rng([seed, m, c.D])
    qs = 2 * c.D ** -0.25 if c.kv == "fp8" else c.D ** -0.25
    return (rng.standard_normal((m, c.H, c.D)) * qs).astype(np.float32)


def _prefill(c, qd, kind, *, launch="prefill", keep_out=1, want_out=True, split=True, window=0,
             **where):
    import llm_capi
    sm, osc = _scales(c)
    return llm_capi.pa_rows(qd, c.kd, c.vd, c.ptd, launch=launch, out_kind=kind, sm_scale=sm,
                            window=window, pack=1, keep_out=keep_out, out_scale=osc,
                            want_out=want_out, split=split, **where)


def _prefill_check(oracle, c, q, ref, kind, splits, what, **kw):
    """Both stages of one prefill request and its keep_out = 0 twin (out = NULL
    in the split form, which never reads it)."""
    qd = _dev(q)
    what = f"{what} {c.kv} D{c.D} ts{c.ts} {KIND[kind]} split{int(splits)}"
    r1 = _prefill(c, qd, kind, split=splits, **kw)
    out = _stage1(r1, ref, ATOL_PREFILL, what)
    _stage2(oracle, r1, out, 1, what)
    r0 = _prefill(c, qd, kind, split=splits, keep_out=0, want_out=not splits, **kw)
    assert r0["status"] == 0, (what, r0["error"])
    _bits_equal(r1, r0, ("q8", "inv_scale", "out16"), what + " keep_out 0")
    return r1


@pytest.mark.parametrize("p0,m,splits", [(100, 37, True), (0, 20, False), (517, 130, True)],
                         ids=["ctx_p0_ragged_tile", "one_pass", "case_size"])
@pytest.mark.parametrize("kv", ["f16", "fp8"])
@pytest.mark.parametrize("D,ts", [(64, 16), (64, 32), (128, 16), (128, 32)])
def test_prefill_rows(gpu, tune, oracle, D, ts, kv, p0, m, splits):
    """Split + pa_merge_row_kernel with contexts p0 + i + 1 (3 splits at
    p0 100, 11 at p0 517: past the merge's first batch) and the one-pass form
    with its conversion launches (no workspace)."""
    import ctypes
    import llm_capi
    c = _case(3, 3, D, 647, ts, kv)
    row = 1
    view = llm_capi.kv_view(c.kd, c.vd, c.ptd)
    assert (tune.pa_prefill_workspace_bytes(ctypes.byref(view), p0, m) > 0) == splits
    q = _queries(c, m, p0)
    ctx = np.arange(p0 + 1, p0 + m + 1, dtype=np.int32)
    ref = _prefill_ref(oracle, c, q, np.full(m, row, np.int32), ctx, 0)
    for kind in (ROW_Q, ROW_F16):
        _prefill_check(oracle, c, q, ref, kind, splits, f"prefill p0 {p0} m {m}", row=row, p0=p0)


@pytest.mark.parametrize("kv", ["f16", "fp8"])
def test_prefill_rows_window(gpu, tune, oracle, kv):
    """window 24 in the split form: the splits below a query's window hold
    empty partials and the merge counts from tile 0."""
    c = _case(3, 3, 128, 647, 16, kv)
    p0, m, row, W = 100, 37, 2, 24
    q = _queries(c, m, 7)
    ctx = np.arange(p0 + 1, p0 + m + 1, dtype=np.int32)
    ref = _prefill_ref(oracle, c, q, np.full(m, row, np.int32), ctx, W)
    for kind in (ROW_Q, ROW_F16):
        _prefill_check(oracle, c, q, ref, kind, True, "prefill window 24", row=row, p0=p0,
                       window=W)


SEGS = [(2, 0, 37), (0, 100, 70), (1, 31, 1)]


def _seg_rows(segs):
    beam = np.concatenate([np.full(n, r, np.int32) for r, _, n in segs])
    ctx = np.concatenate([np.arange(p0 + 1, p0 + n + 1, dtype=np.int32) for _, p0, n in segs])
    return beam, ctx


@pytest.mark.parametrize("kv,splits,window", [
    ("f16", True, 0), ("f16", False, 0), ("fp8", True, 0), ("fp8", False, 0),
    ("fp8", True, 24), ("f16", False, 24)])
def test_packed_prefill_rows(gpu, tune, oracle, kv, splits, window):
    """Three segments of different page-table rows in one launch, with and
    without the split workspace (and each form once with a window).  One pass:
    every segment's rows equal the single-sequence one-pass prefill of that
    segment bit for bit, in every output."""
    import ctypes
    import llm_capi
    c = _case(3, 2, 128, 170, 16, kv)
    view = llm_capi.kv_view(c.kd, c.vd, c.ptd)
    arr = llm_capi.prefill_segs(SEGS)
    ws = [tune.pa_prefill_packed_workspace_bytes(ctypes.byref(view), arr, len(SEGS), s)
          for s in (0, 1)]
    assert ws[1] > ws[0] > 0  # the split form exists for these segments
    m = sum(n for _, _, n in SEGS)
    q = _queries(c, m, 11)
    beam, ctx = _seg_rows(SEGS)
    ref = _prefill_ref(oracle, c, q, beam, ctx, window)
    from oracle.oracle import unpack_a_f16, unpack_a_i8
    for kind in (ROW_Q, ROW_F16):
        r = _prefill_check(oracle, c, q, ref, kind, splits, f"packed window {window}",
                           launch="packed", segs=SEGS, window=window)
        if splits:
            continue
        out = _np(r["out"])
        at = 0
        for row, p0, n in SEGS:
            s = _prefill(c, _dev(q[at:at + n]), kind, split=False, row=row, p0=p0, window=window)
            assert s["status"] == 0, s["error"]
            sl = slice(at, at + n)
            np.testing.assert_array_equal(out[sl].view(np.uint32), _np(s["out"]).view(np.uint32))
            if kind == ROW_Q:
                np.testing.assert_array_equal(
                    unpack_a_i8(_np(r["q8"]), pr.pad16(m), c.hid)[sl],
                    unpack_a_i8(_np(s["q8"]), pr.pad16(n), c.hid)[:n])
                np.testing.assert_array_equal(_np(r["inv_scale"])[sl].view(np.uint32),
                                              _np(s["inv_scale"]).view(np.uint32))
            else:
                np.testing.assert_array_equal(
                    unpack_a_f16(_np(r["out16"]), pr.pad16(m), c.hid)[sl].view(np.uint16),
                    unpack_a_f16(_np(s["out16"]), pr.pad16(n), c.hid)[:n].view(np.uint16))
            at += n


# ---------------------------------------------------------------------------
# refusals: status and message, nothing written
# ---------------------------------------------------------------------------
def _untouched(res):
    import torch
    for k, fill in (("q8", pr.SENTINEL), ("out16", pr.SENTINEL * 0x0101)):
        if res[k] is not None:
            assert bool((res[k] == fill).all()), f"{k} written by a refused call"
    for k in ("out", "inv_scale"):
        if res[k] is not None:
            assert bool(torch.isnan(res[k]).all()), f"{k} written by a refused call"


def _refused(res, status, text):
    assert res["status"] == status and text in res["error"], (res["status"], res["error"])
    _untouched(res)


def _decode_call(c, kind, **kw):
    import llm_capi
    return llm_capi.pa_rows(c.qd, c.kd, c.vd, c.ptd, launch="decode", out_kind=kind, T=c.T,
                            context_lens=_dev(_lens(c)), **kw)


def test_decode_refusals(gpu, tune):
    import llm_capi
    INVALID, UNSUPPORTED = llm_capi.LLM_ERR_INVALID, llm_capi.LLM_ERR_UNSUPPORTED
    c = _case(6, 4, 64, 300, 16)
    _refused(_decode_call(_case(6, 3, 32, 300, 16), ROW_Q, pages_per_split=4, pack=1), INVALID,
             "packed row outputs need H*D % 64 == 0")
    for gone in ("q", "inv_scale"):
        _refused(_decode_call(c, ROW_Q, pages_per_split=1, omit=(gone,)), INVALID,
                 "row quantisation needs q and inv_scale")
    _refused(_decode_call(c, ROW_F16, pages_per_split=1, omit=("out16",)), INVALID,
             "fp16 rows need out16")
    _refused(_decode_call(c, ROW_Q, pages_per_split=1, has_rows=False), INVALID,
             "row outputs need PaRowOutputs")
    _refused(_decode_call(c, ROW_Q, pages_per_split=1, row_group=4, window=40), UNSUPPORTED,
             "a sliding window needs ungrouped rows")
    # a single split converts the fp32 rows it wrote: out is required
    _refused(_decode_call(_case(6, 4, 64, 40, 16), ROW_Q, pages_per_split=128, want_out=False,
                          keep_out=0), INVALID, "single-split launch needs the fp32 out")
    # 129 heads of 128: a row of 66,048 bytes does not fit the merge's LDS
    wide = _case(1, 129, 128, 32, 16)
    for kind in (ROW_Q, ROW_F16):
        _refused(llm_capi.pa_rows(wide.qd, wide.kd, wide.vd, wide.ptd, launch="decode",
                                  out_kind=kind, T=wide.T, pages_per_split=1), INVALID,
                 "row outputs need H*D <= 16384")


def test_prefill_refusals(gpu, tune):
    """out = NULL needs the split form with row outputs; and the split form's
    merge holds a row of H*D floats in LDS, so it is refused past 64 KiB (as
    pa_decode's row outputs are) before anything is launched -- through the
    internal entries and through the public pa_prefill / pa_prefill_packed."""
    import ctypes
    import llm_capi
    INVALID = llm_capi.LLM_ERR_INVALID
    c = _case(3, 2, 128, 170, 16)
    q = _dev(_queries(c, 20, 1))
    _refused(_prefill(c, q, ROW_Q, split=False, want_out=False, keep_out=0, row=0, p0=0), INVALID,
             "pa_prefill: out is NULL")
    qp = _dev(_queries(c, sum(n for _, _, n in SEGS), 2))
    _refused(_prefill(c, qp, ROW_F16, launch="packed", segs=SEGS, split=False, want_out=False,
                      keep_out=0), INVALID, "pa_prefill_packed: out is NULL")
    wide = _case(1, 129, 128, 200, 16)
    p0, m = 184, 16
    view = llm_capi.kv_view(wide.kd, wide.vd, wide.ptd)
    assert tune.pa_prefill_workspace_bytes(ctypes.byref(view), p0, m) > 0  # it would split
    qw = _dev(_queries(wide, m, 3))
    for kind in (ROW_Q, ROW_F16, F32_ROWS):
        _refused(_prefill(wide, qw, kind, row=0, p0=p0), INVALID,
                 "pa_prefill: the split form needs H*D <= 16384")
        _refused(_prefill(wide, qw, kind, launch="packed", segs=[(0, p0, m)]), INVALID,
                 "pa_prefill_packed: the split form needs H*D <= 16384")
    with pytest.raises(llm_capi.LlmError, match="split form needs H.D <= 16384"):
        llm_capi.pa_prefill(qw, wide.kd, wide.vd, wide.ptd, row=0, p0=p0)
    with pytest.raises(llm_capi.LlmError, match="split form needs H.D <= 16384"):
        llm_capi.pa_prefill_packed(qw, wide.kd, wide.vd, wide.ptd, segs=[(0, p0, m)])
