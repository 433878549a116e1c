"""The attention's fused o_proj (PaOut::OPROJ: pa_split_kernel's workgroup merge
multiplying each merged head by its slice of W_o and adding the products into
counted fixed-point columns, csrc/pa_split.hpp / common.hpp oacc_*) on its own,
through pa_rows_tune of the tuning build, which passes the request to
pa_decode_internal unchanged.

Every launch must report LLM_PA_FORM_WG_MERGE | LLM_PA_FORM_OPROJ at the split
count the case fixes, return status 0, leave o_acc all zero (every column
completed once and cleared itself), leave the row after the last of o_x alone
and write every x[b][n] of the launch.

 a. exact cases, no tolerance: every token of a (page-table row, head) holds one
    V vector of small integers, so the merged head rounds to it in fp16 (asserted
    on the launch's own out16), and W_o holds multiples of 2^-6: every partial
    sum is exact in fp32 whatever the dot instruction rounds (tests/_oproj.py
    assert_fp32_exact), so x equals the integer-exact product bit for bit, with
    heads that cancel to 0 and a negative total among the columns;
 b. random values: the launch's fp32 rows against oracle.paged_attention at the
    decode bars, out16 their fp16 rounding bit for bit, then x against the
    float64 product of the launch's own out16 within the derived elementwise
    bound of _oproj.x_bound; the same bits with and without out16 / the fp32
    rows, on a repeat, and for the same row at another launch row;
 c. the range guard: a head term past (2^23 - 1) / H, and a NaN head, clamp as
    common.hpp oacc_term says, set the flag, still complete and clear;
 d. refusals: status and text, nothing written.

Measured (profiles/oproj_rows.jsonl, 39 launches): the worst |x - ref64| of a
launch stands at 0.0019 .. 0.037 of its elementwise bound (the bound allows
every rounding its worst case; the largest ratios at H = 1, the smallest at
D = 128); stage 1 rel_err 2.6e-7 .. 5.0e-7."""
import contextlib
import functools
import os
import types

import numpy as np
import pytest

import _oproj as op
import _pa_rows as pr
from _fp8 import FORM_WG_MERGE, dev_fp8
from _util import assert_parity, rel_err, record
from _window import window_reference

pytestmark = pytest.mark.gpu
RTOL = 1e-3
ATOL_DECODE = 1e-6  # test_pa_decode_gpu.py, test_pa_rows_gpu.py
FORM_OPROJ = 32     # LLM_PA_FORM_OPROJ
OPROJ = 4           # llm_capi.PA_OUT_OPROJ
B = 6
X_FILL = np.uint32(pr.SENTINEL * 0x01010101)


@pytest.fixture(scope="module")
def tune(gpu):
    import llm_capi
    return llm_capi.load_tune()


def _dev(a):
    import torch
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


# H, D, page, context, and how the split count is fixed: pages_per_split, or
# LLM_WGM_SPLITS over dynamic splits (8 splits of a 9-tile context: the rows'
# own split length is 2 pages, so splits 5 .. 7 hold no tile)
SHAPES = {
    "h1_d64_s8": dict(H=1, D=64, ts=16, T=130, force=8, ns=8),
    "h3_d32_s3": dict(H=3, D=32, ts=16, T=290, pps=7, ns=3),
    "h12_d64_s3": dict(H=12, D=64, ts=16, T=290, pps=7, ns=3),
    "h12_d64_s2": dict(H=12, D=64, ts=16, T=290, pps=10, ns=2),
    "h12_d64_s8": dict(H=12, D=64, ts=16, T=130, force=8, ns=8),
    "h64_d32_s2": dict(H=64, D=32, ts=16, T=130, pps=5, ns=2),
    "h8_d128_s8": dict(H=8, D=128, ts=16, T=130, force=8, ns=8),
    "h8_d128_page32_s2": dict(H=8, D=128, ts=32, T=290, pps=5, ns=2),
}
FULL = [k for k in SHAPES if k not in ("h12_d64_s2", "h12_d64_s8")]


def _round_cols(D, ns):
    """Columns one round of the workgroup covers: 64 lanes x ns waves x CF."""
    kg = D // 8
    return 64 * ns * (1 if kg >= 32 else 32 // kg)


def _o_ns(name):
    s = SHAPES[name]
    if name not in FULL:  # the other split counts of C2's heads: a tail in a wave, a second round
        return [200, _round_cols(s["D"], s["ns"]) + 1]
    r = _round_cols(s["D"], s["ns"])
    return sorted({8, 200, r, r + 1, r + 64 * s["ns"] - 1, s["H"] * s["D"]})


@functools.lru_cache(maxsize=None)
def _geom(H, D, ts, T, kv="f16", rows=B):
    """A shuffled page table of `rows` rows, random K pages and q, and one
    random V pool (1 + 0.25 N(0,1), clipped to >= 0.25; garbage in the unused
    pages) with the fp32 values the kernels read."""
    rng = np.random.default_rng([rows, H, D, T, ts, len(kv)])
    pt, num_pages, unused = pr.page_table(rng, rows, H, T, ts)
    shape = (num_pages, ts, D)
    kh, kf = pr.pool_values(rng, kv, shape, D ** -0.25, unused)
    q = (rng.standard_normal((rows, H, D)) * D ** -0.25).astype(np.float32)
    g = types.SimpleNamespace(rows=rows, H=H, D=D, T=T, ts=ts, hid=H * D, pt=pt, unused=unused,
                              num_pages=num_pages, kf=kf, q=q, ptd=_dev(pt), qd=_dev(q), kv=kv)
    if kv == "f16":
        vr = np.clip(1 + 0.25 * rng.standard_normal(shape), 0.25, None).astype(np.float32)
        vr[unused] *= 50
        vh = vr.astype(np.float16)
        g.kd, g.vd, g.vf = _dev(kh), _dev(vh), vh.astype(np.float32)
    else:  # (the refusals' pools)
        vh, g.vf = pr.pool_values(rng, kv, shape, 1.0, unused)
        up = dev_fp8 if kv == "fp8" else (lambda t: t.cuda())
        g.kd, g.vd = up(kh), up(vh)
    return g


def _shape_geom(name):
    s = SHAPES[name]
    return _geom(s["H"], s["D"], s["ts"], s["T"])


def _const_v(g, v):
    """A V pool whose every token of page-table row r, head h holds v[r][h]
    (fp16 values [rows][H][D]); 1000 in the unused pages."""
    vh = np.full((g.num_pages, g.ts, g.D), 1000.0, np.float16)
    nt = g.pt.shape[2] - 2
    vh[g.pt[:, :, :nt]] = np.asarray(v, np.float16)[:, :, None, None, :]
    return _dev(vh)


def _lens(g, n=B):
    base = [g.T, 0, 1, 2 * g.ts - 1, 5, g.T // 2 + 3, g.T - g.ts, g.ts]
    return np.array(base[:n], np.int32)


def _reversed(n=B):  # launch row b reads page-table row n - 1 - b
    return np.arange(n - 1, -1, -1, dtype=np.int32)


def _launch(g, vd, wo, lens, beam_ids, *, pps=0, force=None, ns=None, qd=None, **kw):
    import llm_capi
    kw.setdefault("pack", 0)
    kw.setdefault("rows16", 1)
    with _env(LLM_WGM_SPLITS=force):
        return llm_capi.pa_rows(g.qd if qd is None else qd, g.kd, vd, g.ptd, launch="decode",
                                out_kind=OPROJ, T=g.T, beam_ids=_dev(beam_ids),
                                context_lens=_dev(lens), pages_per_split=pps, wo=wo, **kw)


def _how(name):
    s = SHAPES[name]
    return dict(pps=s.get("pps", 0), force=s.get("force"))


def _common(res, n_rows, o_n, ns, what, flag=0):
    """What every launch must leave; returns x [rows][o_n] and the fp16 rows."""
    assert res["status"] == 0, (what, res["error"])
    assert (res["nsplit"], res["form"]) == (ns, FORM_WG_MERGE | FORM_OPROJ), \
        (what, res["nsplit"], res["form"])
    xall = res["x"].cpu().numpy()
    assert xall.shape == (n_rows + 1, o_n)
    assert (xall[n_rows].view(np.uint32) == X_FILL).all(), f"{what}: the row past the launch written"
    nz = int((res["o_acc"] != 0).sum())
    assert nz == 0, f"{what}: {nz} accumulator columns not back at zero"
    x = xall[:n_rows]
    left = np.argwhere(x.view(np.uint32) == X_FILL)
    assert left.size == 0, f"{what}: {len(left)} x never written, first (b, n) {tuple(left[0])}"
    assert int(res["o_flag"].item()) == flag, (what, int(res["o_flag"].item()))
    o16 = None
    if res["out16"] is not None:
        o16 = res["out16"].cpu().numpy().view(np.float16).reshape(n_rows, -1)
    return x, o16


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (f"{what}: {len(bad)} of {got.size} x differ, first (b, n) "
                           f"{tuple(bad[0])}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")


def _live(g, lens, beam_ids):
    ids = np.asarray(beam_ids)
    return (np.asarray(lens) > 0) & (ids >= 0) & (ids < g.rows)


def _rows_of(per_row, g, lens, beam_ids):
    """Launch rows from page-table rows: row b holds per_row[beam_ids[b]] where
    it has a context and routes into the table, else zeros."""
    live = _live(g, lens, beam_ids)
    out = np.zeros((len(lens),) + per_row.shape[1:], per_row.dtype)
    out[live] = per_row[np.asarray(beam_ids)[live]]
    return out


# ---------------------------------------------------------------------------
# a. exact cases
# ---------------------------------------------------------------------------
def _exact_check(g, o_n, ns, what, *, lens=None, beam_ids=None, seed=0, **how):
    lens = _lens(g) if lens is None else lens
    beam_ids = _reversed() if beam_ids is None else beam_ids
    rng = np.random.default_rng([g.H, g.D, o_n, ns, seed])
    c = op.exact_case(rng, g.rows, g.H, g.D, o_n, r0=int(beam_ids[0]))
    op.assert_fp32_exact(c.v, c.wo, g.H, g.D)
    res = _launch(g, _const_v(g, c.v), c.wo, lens, beam_ids, **how)
    x, o16 = _common(res, len(lens), o_n, ns, what)
    want16 = _rows_of(c.v.reshape(g.rows, g.hid).astype(np.float16), g, lens, beam_ids)
    assert np.array_equal(o16, want16), f"{what}: the merged heads are not the V vectors"
    _same_bits(x, _rows_of(c.x, g, lens, beam_ids), what)
    return res


@pytest.mark.parametrize("name", list(SHAPES))
def test_exact(gpu, tune, name):
    s, g = SHAPES[name], _shape_geom(name)
    for o_n in _o_ns(name):
        _exact_check(g, o_n, s["ns"], f"exact {name} o_n{o_n}", **_how(name))


@pytest.mark.parametrize("route", [-1, B, 1 << 20])
def test_exact_row_outside_the_page_table(gpu, tune, route):
    """A launch row routed outside the page table reads nothing: its x is
    exactly 0, its columns complete and clear, the other rows do not notice."""
    name = "h12_d64_s3"
    g = _shape_geom(name)
    beam_ids = _reversed()
    beam_ids[3] = route
    res = _exact_check(g, 200, 3, f"exact route {route}", beam_ids=beam_ids, **_how(name))
    assert not res["x"][3].cpu().numpy().any()


def test_exact_window(gpu, tune):
    """window 40 at one page per split: 4 splits counted from each row's own
    first live tile; the merged heads are still the V vectors."""
    g = _shape_geom("h12_d64_s3")
    _exact_check(g, 200, 4, "exact window 40", pps=1, window=40)


def test_exact_layers_back_to_back(gpu, tune):
    """Three launches on one stream into the same o_acc and flag, three W_o (and
    V sets), nothing cleared in between: the "cleared for the next layer"
    contract without a decoder."""
    import torch
    name = "h12_d64_s3"
    s, g = SHAPES[name], _shape_geom(name)
    o_n, lens, beam_ids = 769, _lens(g), _reversed()
    cases = [op.exact_case(np.random.default_rng([77, i]), g.rows, g.H, g.D, o_n,
                           r0=int(beam_ids[0])) for i in range(3)]
    vds = [_const_v(g, c.v) for c in cases]
    o_acc = torch.zeros(((B + 1) * o_n,), dtype=torch.int64, device="cuda")
    o_flag = torch.zeros((1,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    runs = [_launch(g, vd, c.wo, lens, beam_ids, o_acc=o_acc, o_flag=o_flag, sync=False,
                    **_how(name)) for c, vd in zip(cases, vds)]
    torch.cuda.synchronize()
    for i, (c, res) in enumerate(zip(cases, runs)):
        x, _ = _common(res, B, o_n, s["ns"], f"layer {i}")
        _same_bits(x, _rows_of(c.x, g, lens, beam_ids), f"layer {i}")


# ---------------------------------------------------------------------------
# b. random values against float64
# ---------------------------------------------------------------------------
_refs = {}


def _attn_ref(oracle, g, lens, beam_ids, window):
    key = (id(g), lens.tobytes(), beam_ids.tobytes(), window)
    if key not in _refs:
        q = g.q[:len(lens)]
        if window:
            r = window_reference(oracle, q, g.kf, g.vf, g.pt, lens, window, beam_ids)
        else:
            r = oracle.paged_attention(q, g.kf, g.vf, g.pt, T=g.T, beam_ids=beam_ids,
                                       context_lens=lens)
        _refs[key] = pr.rows_ref(r)
    return _refs[key]


def _random_wo(g, o_n, seed=0):
    rng = np.random.default_rng([g.H, g.D, o_n, seed, 5])
    w = (0.02 * rng.standard_normal((g.hid, o_n))).astype(np.float16)
    small = np.abs(w) < np.float16(2.0 ** -13)
    w[small] = np.where(np.signbit(w[small]), -1, 1) * np.float16(2.0 ** -13)
    return w


def _random_check(oracle, g, o_n, ns, what, *, window=0, **how):
    lens, beam_ids = _lens(g), _reversed()
    wo = _random_wo(g, o_n)
    res = _launch(g, g.vd, wo, lens, beam_ids, window=window, **how)
    x, o16 = _common(res, B, o_n, ns, what)
    # stage 1: the attention itself
    out = res["out"].cpu().numpy()
    assert np.isfinite(out).all(), f"{what}: fp32 rows not all written"
    ref = _attn_ref(oracle, g, lens, beam_ids, window)
    assert_parity(out, ref, RTOL, ATOL_DECODE, what=what)
    np.testing.assert_array_equal(out[lens == 0], 0.0)
    pr.check_conversions(None, out, out16=res["out16"].cpu().numpy(), pack=0, what=what)
    a16 = np.abs(o16.astype(np.float64))
    assert ((a16 == 0) | (a16 >= 2.0 ** -14)).all(), f"{what}: a subnormal o_proj input"
    # stage 2: the o_proj of those fp16 rows
    x64 = op.x_ref64(o16, wo)
    ratio = float((np.abs(x.astype(np.float64) - x64) / op.x_bound(o16, wo, g.H, g.D)).max())
    print(f"{what}: stage 1 rel_err {rel_err(out, ref):.3e}, stage 2 worst ratio {ratio:.4f}")
    record("oproj_rows", case=what, rel_err=rel_err(out, ref), bound_ratio=ratio)
    assert ratio <= 1.0, f"{what}: |x - ref64| at {ratio:.3f} of its elementwise bound"
    assert not x[lens == 0].any()
    return res, wo


@pytest.mark.parametrize("name", list(SHAPES))
def test_random_against_float64(gpu, tune, oracle, name):
    s, g = SHAPES[name], _shape_geom(name)
    for o_n in _o_ns(name):
        _random_check(oracle, g, o_n, s["ns"], f"random {name} o_n{o_n}", **_how(name))


def test_random_window(gpu, tune, oracle):
    g = _shape_geom("h12_d64_s3")
    _random_check(oracle, g, 200, 4, "random window 40 h12_d64 o_n200", pps=1, window=40)


@pytest.mark.parametrize("name", FULL)
def test_same_bits_between_runs(gpu, tune, name):
    """x does not depend on which other outputs are asked for, on the run, or
    on the launch row a request sits in (heads arrive in any order: the integer
    columns make the sum order-free)."""
    s, g = SHAPES[name], _shape_geom(name)
    o_n, lens, beam_ids = 200, _lens(g), _reversed()
    wo = _random_wo(g, o_n)
    how = _how(name)
    what = f"bits {name}"
    base = _launch(g, g.vd, wo, lens, beam_ids, **how)
    x, o16 = _common(base, B, o_n, s["ns"], what)
    for label, kw in (("rows16 0", dict(rows16=0)),
                      ("keep_out 0", dict(keep_out=0, want_out=False)),
                      ("rows16 0 keep_out 0", dict(rows16=0, keep_out=0, want_out=False)),
                      ("repeat", {})):
        r = _launch(g, g.vd, wo, lens, beam_ids, **how, **kw)
        xr, o16r = _common(r, B, o_n, s["ns"], f"{what} {label}")
        _same_bits(xr, x, f"{what} {label}")
        assert (o16r is None) == (kw.get("rows16", 1) == 0)
        if o16r is not None:
            assert np.array_equal(o16r.view(np.uint16), o16.view(np.uint16)), label
    perm = np.array([4, 0, 5, 1, 3, 2])
    r = _launch(g, g.vd, wo, lens[perm], beam_ids[perm], qd=g.qd[_dev(perm)].contiguous(), **how)
    xp, o16p = _common(r, B, o_n, s["ns"], f"{what} permuted")
    _same_bits(xp, x[perm], f"{what} permuted")
    assert np.array_equal(o16p.view(np.uint16), o16[perm].view(np.uint16))


# ---------------------------------------------------------------------------
# c. the range guard
# ---------------------------------------------------------------------------
GUARD = "h3_d32_s3"
G_ROW, G_HEAD, G_COL, G_ON = 3, 2, 7, 200  # launch row, head, W_o column


def _guard_base():
    g = _shape_geom(GUARD)
    lens, beam_ids = _lens(g), _reversed()
    c = op.exact_case(np.random.default_rng(31), g.rows, g.H, g.D, G_ON, r0=int(beam_ids[0]))
    return g, lens, beam_ids, c


def _guard_launch_and_ref(g, lens, beam_ids, v16, wo, what):
    s = SHAPES[GUARD]
    res = _launch(g, _const_v(g, v16), wo, lens, beam_ids, **_how(GUARD))
    x, o16 = _common(res, B, G_ON, s["ns"], what, flag=1)
    want16 = _rows_of(v16.reshape(g.rows, g.hid), g, lens, beam_ids)
    assert np.array_equal(o16, want16, equal_nan=True), what
    xr, clamped = op.x_fixed_ref(op.head_terms(want16, wo, g.H, g.D), g.H)
    _same_bits(x, xr, what)
    return res, x, xr, clamped


def test_range_guard_large_term(gpu, tune):
    """One head's V vector and its W_o column at 60000: that head's term
    (32 * 3.6e9) is clamped to +(2^23 - 1) / 3; the column holds the clamped
    sum, the flag is set, everything completes and clears; every other column
    is the exact product; a benign launch into the same buffers is exact."""
    g, lens, beam_ids, c = _guard_base()
    v16 = c.v.astype(np.float16)
    v16[beam_ids[G_ROW], G_HEAD] = 60000
    wo = c.wo.copy()
    wo[G_HEAD * g.D:(G_HEAD + 1) * g.D, G_COL] = 60000
    res, x, xr, clamped = _guard_launch_and_ref(g, lens, beam_ids, v16, wo, "guard 60000")
    assert clamped[G_ROW, G_COL] and not np.delete(clamped, G_COL, axis=1).any()
    lim = float(op.oacc_limit(g.H))
    t = op.head_terms(_rows_of(v16.reshape(g.rows, -1), g, lens, beam_ids), wo, g.H, g.D)
    assert x[G_ROW, G_COL] == np.float32(lim + t[G_ROW, :G_HEAD, G_COL].sum())
    # the other columns: no term near the limit, so the exact product -- every
    # term is exact (the 60000 head's are multiples of 1/2 below 2^22), the
    # integer sum is, and x is that sum (float64 holds it) rounded once to fp32
    x64 = op.x_ref64(_rows_of(v16.reshape(g.rows, -1), g, lens, beam_ids), wo)
    others = np.delete(np.arange(G_ON), G_COL)
    assert np.abs(np.delete(t[:, G_HEAD], G_COL, axis=1)).max() < 2.0 ** 22
    _same_bits(x[:, others], x64[:, others].astype(np.float32), "guard 60000, other columns")
    # benign launch, same accumulator and flag (reset)
    res["o_flag"].zero_()
    again = _launch(g, _const_v(g, c.v), c.wo, lens, beam_ids, o_acc=res["o_acc"],
                    o_flag=res["o_flag"], **_how(GUARD))
    xa, _ = _common(again, B, G_ON, SHAPES[GUARD]["ns"], "guard 60000, then benign")
    _same_bits(xa, _rows_of(c.x, g, lens, beam_ids), "guard 60000, then benign")


def test_range_guard_nan_head(gpu, tune):
    """A NaN in one dim of one head's V: every column's term of that (row,
    head) is NaN and clamps to the positive limit; the other rows are exact."""
    g, lens, beam_ids, c = _guard_base()
    v16 = c.v.astype(np.float16)
    v16[beam_ids[G_ROW], G_HEAD, 5] = np.nan
    res, x, xr, clamped = _guard_launch_and_ref(g, lens, beam_ids, v16, c.wo, "guard nan")
    assert clamped[G_ROW].all() and not np.delete(clamped, G_ROW, axis=0).any()
    rest = np.delete(np.arange(B), G_ROW)
    _same_bits(x[rest], _rows_of(c.x, g, lens, beam_ids)[rest], "guard nan, other rows")
    lim = float(op.oacc_limit(g.H))
    others = np.delete(np.arange(g.H), G_HEAD)
    t = op.head_terms(_rows_of(c.v.reshape(g.rows, -1).astype(np.float16), g, lens, beam_ids),
                      c.wo, g.H, g.D)
    np.testing.assert_array_equal(x[G_ROW], (lim + t[G_ROW, others].sum(axis=0)).astype(np.float32))


# ---------------------------------------------------------------------------
# d. refusals: status and message, nothing written
# ---------------------------------------------------------------------------
def _refused(res, status, text):
    import torch
    assert res["status"] == status and text in res["error"], (res["status"], res["error"])
    assert (res["x"].cpu().numpy().view(np.uint32) == X_FILL).all(), "x written by a refused call"
    assert not bool(res["o_acc"].any()) and int(res["o_flag"].item()) == 0
    assert res["out"] is None or bool(torch.isnan(res["out"]).all())
    assert res["out16"] is None or bool((res["out16"] == pr.SENTINEL * 0x0101).all())


def test_refusals(gpu, tune):
    import llm_capi
    INVALID, UNSUPPORTED = llm_capi.LLM_ERR_INVALID, llm_capi.LLM_ERR_UNSUPPORTED
    no_wgm = "the fused o_proj needs the workgroup-merge form over fp16 pools"
    no_args = "fused o_proj needs W_o head slices, an output, a range flag, o_n > 0"

    def call(g, **kw):
        return _launch(g, g.vd, _random_wo(g, 64), _lens(g), _reversed(), **kw)

    g = _geom(4, 64, 16, 290)
    _refused(call(_geom(4, 64, 16, 40), pps=128), UNSUPPORTED, no_wgm)  # a single split
    _refused(call(g, pps=1), UNSUPPORTED, no_wgm)                      # 19 splits
    for kv in ("bf16", "fp8"):
        _refused(call(_geom(4, 64, 16, 290, kv), pps=7), UNSUPPORTED, no_wgm)
    _refused(call(g, pps=7, row_group=4), UNSUPPORTED, no_wgm)
    _refused(call(_geom(2, 256, 16, 290), pps=7), INVALID, no_args)
    _refused(call(_geom(65, 32, 16, 130), pps=5), INVALID, no_args)
    _refused(call(g, pps=7, o_n=0), INVALID, no_args)
    _refused(call(g, pps=7, omit=("o_flag",)), INVALID, no_args)
    # (and the same request, complete, runs)
    _common(call(g, pps=7), B, 64, 3, "refusals: the complete request")
