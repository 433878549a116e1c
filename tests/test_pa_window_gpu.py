"""Sliding-window paged attention through the C ABI: pa_decode_window,
pa_prefill_window, pa_prefill_packed_window and kv_cache_release_before.

Reference: the oracle knows no window.  Row b's reference is
Oracle.paged_attention over a shifted copy (tests/_window.py): tokens
[t_lo, T_b) of the row in a fresh pool at positions [0, T_b - t_lo).  Bars: the
project's attention bar, assert_parity(.., 1e-3) tensor-wide and elementwise
(the prefill kernel with its elementwise floor of test_pa_prefill_gpu.py,
4e-6 of the output scale, for the reason given there)."""
import ctypes

import numpy as np
import pytest

from _fp8 import FORM_DIRECT, FORM_SPLIT_MERGE, dev_fp8, fp8_pools
from _util import assert_parity
from _window import t_lo_of, t_prime, window_reference

pytestmark = pytest.mark.gpu
RTOL = 1e-3
PREFILL_ATOL_FRAC = 4e-6  # test_pa_prefill_gpu.py ATOL_FRAC


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _case(rng, rows, H, D, T, ts, kind="f16", extra_tiles=0):
    """Pools of `kind` with every tile of `rows` rows present: (q scale, device
    K, device V, fp32 K, fp32 V, page table [rows][H][nt + extra_tiles])."""
    nt = (T + ts - 1) // ts
    num_pages = rows * H * nt + 5
    shape = (num_pages, ts, D)
    if kind == "fp8":
        kb, vb, kf, vf = fp8_pools(rng, shape, D ** -0.25)
        kd, vd = dev_fp8(kb), dev_fp8(vb)
    elif kind == "i8":  # raw values, no scale
        ki = rng.integers(-4, 5, size=shape).astype(np.int8)
        vi = rng.integers(-100, 101, size=shape).astype(np.int8)
        kf, vf, kd, vd = ki.astype(np.float32), vi.astype(np.float32), _dev(ki), _dev(vi)
    else:
        k16 = (rng.standard_normal(shape) * D ** -0.25).astype(np.float16)
        v16 = rng.standard_normal(shape).astype(np.float16)
        kf, vf, kd, vd = k16.astype(np.float32), v16.astype(np.float32), _dev(k16), _dev(v16)
    perm = rng.permutation(num_pages)[: rows * H * nt].astype(np.int32)
    pt = np.full((rows, H, nt + extra_tiles), -1, np.int32)
    pt[:, :, :nt] = perm.reshape(rows, H, nt)
    return kd, vd, kf, vf, pt


def _q(rng, n, H, D, kind="f16"):
    s = D ** -0.25 if kind != "i8" else 0.25 * D ** -0.5
    return (rng.standard_normal((n, H, D)) * s).astype(np.float32)


def _window(q, kd, vd, pt, lens, W, T, pps=0, beam_ids=None):
    import llm_capi
    return llm_capi.pa_decode(_dev(q), kd, vd, _dev(pt), T=T, context_lens=_dev(lens),
                              beam_ids=None if beam_ids is None else _dev(beam_ids),
                              pages_per_split=pps, window=W).cpu().numpy()


LENS = np.array([1, 3, 16, 17, 40, 41, 700, 1500], np.int32)


@pytest.fixture(scope="module")
def base_case(gpu):
    """H 4, D 64, page 16, eight ragged rows: shared by the tests below, unchanged."""
    rng = np.random.default_rng(2024)
    B, H, D, ts, T = len(LENS), 4, 64, 16, 1500
    kd, vd, kf, vf, pt = _case(rng, B, H, D, T, ts)
    return dict(q=_q(rng, B, H, D), kd=kd, vd=vd, kf=kf, vf=vf, pt=pt, T=T, ts=ts, H=H, D=D)


@pytest.mark.parametrize("W", [1, 5, 16, 17, 40, 700])
def test_decode_window_vs_oracle(gpu, oracle, base_case, W):
    """T_b < W, == W and == W + 1 all occur (16 / 17, 40 / 41 against W 16, 17,
    40), and windows inside one page, ending on a page edge and starting
    mid-page.  pages_per_split 8 pins the split count, ceil(tiles / 8) over the
    window's tiles; over the W set both the direct and the split + merge form run."""
    import llm_capi
    c = base_case
    ref = window_reference(oracle, c["q"], c["kf"], c["vf"], c["pt"], LENS, W)
    for pps in (0, 8):
        ns, form = llm_capi.pa_decode_plan(c["kd"], c["vd"], _dev(c["pt"]), B=len(LENS), T=c["T"],
                                           pages_per_split=pps, window=W)
        tiles = min((c["T"] + 15) // 16, (W + 15) // 16 + 1)
        if pps:
            assert ns == (tiles + pps - 1) // pps
        assert form == (FORM_DIRECT if ns == 1 else FORM_SPLIT_MERGE)
        if pps and W <= 40:
            assert form == FORM_DIRECT
        if pps and W == 700:
            assert form == FORM_SPLIT_MERGE and ns == 6
        out = _window(c["q"], c["kd"], c["vd"], c["pt"], LENS, W, c["T"], pps)
        assert_parity(out, ref, RTOL, what=f"W {W} pps {pps}")


@pytest.mark.parametrize("kind,D,ts", [("f16", 128, 32), ("fp8", 64, 16), ("fp8", 128, 16),
                                       ("i8", 64, 16), ("f16", 256, 16)])
def test_decode_window_other_pools(gpu, oracle, kind, D, ts):
    rng = np.random.default_rng(D + ts)
    lens = np.array([1, 33, 100, 101, 500, 777], np.int32)
    B, H, T, W = len(lens), 3, 777, 100
    kd, vd, kf, vf, pt = _case(rng, B, H, D, T, ts, kind)
    q = _q(rng, B, H, D, kind)
    ref = window_reference(oracle, q, kf, vf, pt, lens, W)
    for pps in (0, 2):
        out = _window(q, kd, vd, pt, lens, W, T, pps)
        assert_parity(out, ref, RTOL, what=f"{kind} D {D} ts {ts} pps {pps}")


def test_decode_window_missing_pages(gpu, oracle):
    """A page inside the window gone changes the result as the oracle says; a
    page below the window gone changes nothing, bit for bit."""
    rng = np.random.default_rng(5)
    lens = np.array([80, 160, 400], np.int32)  # t_lo 16, 96, 336: page edges
    B, H, D, ts, T, W = 3, 4, 64, 16, 400, 64
    kd, vd, kf, vf, pt = _case(rng, B, H, D, T, ts)
    q = _q(rng, B, H, D)
    for pps in (0, 2):
        full = _window(q, kd, vd, pt, lens, W, T, pps)
        inside, below = pt.copy(), pt.copy()
        for b in range(B):
            lo_tile = t_lo_of(int(lens[b]), W) // ts
            inside[b, b % H, lo_tile + 1 + b % 2] = -1
            below[b, :, lo_tile - 1] = -1
            below[b, :, 0] = -1
        out_in = _window(q, kd, vd, inside, lens, W, T, pps)
        assert_parity(out_in, window_reference(oracle, q, kf, vf, inside, lens, W), RTOL)
        assert not np.array_equal(out_in, full)
        np.testing.assert_array_equal(_window(q, kd, vd, below, lens, W, T, pps), full)


def test_decode_window_ignores_stale_data_below_it(gpu):
    """NaN in every token below t_lo, the masked head of the first live page
    included: the output is finite and the same bits (0 * NaN would be NaN: the
    kernel selects masked V rows away, it does not multiply them by zero)."""
    import torch
    rng = np.random.default_rng(9)
    lens = np.array([17, 41, 700, 1500], np.int32)
    B, H, D, ts, T, W = 4, 4, 64, 16, 1500, 20
    kd, vd, kf, vf, pt = _case(rng, B, H, D, T, ts)
    q = _q(rng, B, H, D)
    k_nan, v_nan = kd.clone(), vd.clone()
    for b in range(B):
        lo = t_lo_of(int(lens[b]), W)
        for h in range(H):
            for t in range(lo // ts + 1):
                n = min(ts, lo - t * ts)  # tokens of tile t below t_lo
                if n > 0:
                    k_nan[int(pt[b, h, t]), :n] = float("nan")
                    v_nan[int(pt[b, h, t]), :n] = float("nan")
    assert torch.isnan(k_nan).sum() > 0
    for pps in (0, 8):
        clean = _window(q, kd, vd, pt, lens, W, T, pps)
        dirty = _window(q, k_nan, v_nan, pt, lens, W, T, pps)
        assert np.isfinite(dirty).all()
        np.testing.assert_array_equal(dirty, clean)


def test_decode_window_splits_are_relative(gpu):
    """T_b - W on a page edge, pages_per_split 8: the windowed launch cuts tiles
    lo_tile .. into the splits pa_decode cuts tiles 0 .. of the same pages into
    (the page-table rows shifted left by lo_tile, context W), so the bits agree."""
    import llm_capi
    rng = np.random.default_rng(13)
    W, ts = 320, 16
    lens = np.array([W + 16 * 5, W + 16 * 37, W + 16 * 60, W], np.int32)
    B, H, D, T = len(lens), 4, 64, int(lens.max())
    kd, vd, kf, vf, pt = _case(rng, B, H, D, T, ts)
    q = _q(rng, B, H, D)
    shifted = np.full_like(pt, -1)
    for b in range(B):
        lo = (int(lens[b]) - W) // ts
        shifted[b, :, : pt.shape[2] - lo] = pt[b, :, lo:]
    ns_w, form_w = llm_capi.pa_decode_plan(kd, vd, _dev(pt), B=B, T=T, pages_per_split=8, window=W)
    ns_s, form_s = llm_capi.pa_decode_plan(kd, vd, _dev(shifted), B=B, T=W, pages_per_split=8)
    assert (ns_w, form_w) == (ns_s, form_s) == (3, FORM_SPLIT_MERGE)
    out = _window(q, kd, vd, pt, lens, W, T, 8)
    want = llm_capi.pa_decode(_dev(q), kd, vd, _dev(shifted), T=W,
                              context_lens=_dev(np.full(B, W, np.int32)),
                              pages_per_split=8).cpu().numpy()
    np.testing.assert_array_equal(out, want)


def test_decode_window_plan_equivalence(gpu, base_case):
    """W >= T: the launch, its plan and its bits are pa_decode's.  W < T: the
    planned split count is that of T' = min(T, (ceil(W / TS) + 1) * TS)."""
    import llm_capi
    c = base_case
    ptd = _dev(c["pt"])
    B, T = len(LENS), c["T"]
    for pps in (0, 8):
        off = llm_capi.pa_decode_plan(c["kd"], c["vd"], ptd, B=B, T=T, pages_per_split=pps)
        plain = llm_capi.pa_decode(_dev(c["q"]), c["kd"], c["vd"], ptd, T=T,
                                   context_lens=_dev(LENS), pages_per_split=pps).cpu().numpy()
        for W in (T, T + 1, 1 << 30):
            assert llm_capi.pa_decode_plan(c["kd"], c["vd"], ptd, B=B, T=T, pages_per_split=pps,
                                           window=W) == off
            np.testing.assert_array_equal(
                _window(c["q"], c["kd"], c["vd"], c["pt"], LENS, W, T, pps), plain)
        # W = 0 is off
        np.testing.assert_array_equal(_window(c["q"], c["kd"], c["vd"], c["pt"], LENS, 0, T, pps),
                                      plain)
        for W in (1, 17, 100, 700):
            got = llm_capi.pa_decode_plan(c["kd"], c["vd"], ptd, B=B, T=T, pages_per_split=pps,
                                          window=W)
            want = llm_capi.pa_decode_plan(c["kd"], c["vd"], ptd, B=B, T=t_prime(T, W, c["ts"]),
                                           pages_per_split=pps)
            assert got == want, (pps, W, got, want)


# --------------------------------------------------------------------------
# prefill
# --------------------------------------------------------------------------
def _split_plan(H, ts, end, nq):
    """pa_prefill's key split (csrc/pa_prefill.hip split_plan): (nsplit, pps)."""
    step = 32 // ts
    ntiles = (end + ts - 1) // ts
    want = min(max(1024 // max(nq * H, 1), 1), 128)
    pps = (ntiles + want - 1) // want
    pps = max((pps + step - 1) // step * step, 2 * step)
    return max(1, min((ntiles + pps - 1) // pps, 128)), pps


def _prefill_window(q, kd, vd, ptd, *, row, p0, W, split):
    """pa_prefill_window with a workspace full of NaN, so a partial the merge
    reads and no workgroup wrote cannot pass."""
    import llm_capi
    import torch
    lib = llm_capi.load()
    m, H, D = q.shape
    view = llm_capi.kv_view(kd, vd, ptd)
    qd = _dev(q)
    out = torch.empty((m, H, D), dtype=torch.float32, device="cuda")
    nbytes = lib.pa_prefill_workspace_bytes(ctypes.byref(view), p0, m) if split else 0
    ws = torch.full((max(nbytes, 16) // 4,), float("nan"), dtype=torch.float32, device="cuda")
    llm_capi.check(lib.pa_prefill_window(ctypes.byref(view), llm_capi.ptr(qd), H * D,
                                         llm_capi.ptr(out), H * D, row, p0, m, 1.0, W,
                                         llm_capi.ptr(ws) if nbytes else None, nbytes,
                                         llm_capi.stream_ptr()))
    return out.cpu().numpy(), nbytes


@pytest.mark.parametrize("p0,m,W", [(0, 100, 24), (37, 64, 16), (512, 130, 100), (1000, 512, 100)])
@pytest.mark.parametrize("kind,D,ts", [("f16", 64, 16), ("f16", 128, 32), ("fp8", 64, 16),
                                       ("fp8", 128, 32)])
def test_prefill_window_equals_decode_and_oracle(gpu, oracle, p0, m, W, kind, D, ts):
    rng = np.random.default_rng(p0 + 3 * m + D)
    H, row, T = 4, 1, p0 + m
    kd, vd, kf, vf, pt = _case(rng, 2, H, D, T, ts, kind, extra_tiles=2)
    q = _q(rng, m, H, D)
    lens = np.arange(p0 + 1, T + 1, dtype=np.int32)
    rows = np.full(m, row, np.int32)
    ref = window_reference(oracle, q, kf, vf, pt, lens, W, beam_ids=rows)
    dec = _window(q, kd, vd, pt, lens, W, T, 0, beam_ids=rows)
    assert_parity(dec, ref, RTOL, what="decode rows")
    ptd = _dev(pt)
    for split in (False, True):
        out, nbytes = _prefill_window(q, kd, vd, ptd, row=row, p0=p0, W=W, split=split)
        assert np.isfinite(out).all()
        assert_parity(out, ref, RTOL, PREFILL_ATOL_FRAC, what=f"oracle, split {split}")
        assert_parity(out, dec, RTOL, PREFILL_ATOL_FRAC, what=f"decode, split {split}")
        if split and p0 >= 512:
            # the split form ran, and split 0 lies wholly below the first query
            # tile's window: that workgroup wrote empty partials over the NaN
            nsplit, pps = _split_plan(H, ts, T, (m + 63) // 64)
            assert nbytes == m * H * nsplit * (D + 2) * 4 and nsplit > 1
            assert pps * ts <= p0 - W + 1


def test_prefill_packed_window(gpu, oracle):
    """Four segments of mixed p0 and length, W = 50: each packed row equals
    pa_prefill_window of its segment, bit for bit in the one-pass form."""
    import llm_capi
    rng = np.random.default_rng(77)
    H, D, ts, W = 4, 64, 16, 50
    segs = [(0, 0, 1), (1, 5, 70), (2, 300, 64), (3, 900, 130)]
    T = max(p0 + n for _, p0, n in segs)
    kd, vd, kf, vf, pt = _case(rng, 4, H, D, T, ts, extra_tiles=1)
    ptd = _dev(pt)
    m = sum(n for _, _, n in segs)
    q = _q(rng, m, H, D)
    for split in (False, True):
        out = llm_capi.pa_prefill_packed(_dev(q), kd, vd, ptd, segs=segs, split=split,
                                         window=W).cpu().numpy()
        q0 = 0
        for row, p0, n in segs:
            one, _ = _prefill_window(q[q0:q0 + n], kd, vd, ptd, row=row, p0=p0, W=W, split=split)
            if split:
                assert_parity(out[q0:q0 + n], one, RTOL, PREFILL_ATOL_FRAC, what=f"row {row}")
            else:
                np.testing.assert_array_equal(out[q0:q0 + n], one)
            lens = np.arange(p0 + 1, p0 + n + 1, dtype=np.int32)
            ref = window_reference(oracle, q[q0:q0 + n], kf, vf, pt, lens, W,
                                   beam_ids=np.full(n, row, np.int32))
            assert_parity(out[q0:q0 + n], ref, RTOL, PREFILL_ATOL_FRAC, what=f"oracle row {row}")
            q0 += n
    # window 0 through the window entries is the unwindowed entry
    np.testing.assert_array_equal(
        llm_capi.pa_prefill_packed(_dev(q), kd, vd, ptd, segs=segs, split=False, window=0).cpu().numpy(),
        llm_capi.pa_prefill_packed(_dev(q), kd, vd, ptd, segs=segs, split=False).cpu().numpy())


# --------------------------------------------------------------------------
# kv_cache_release_before
# --------------------------------------------------------------------------
def test_kv_cache_release_before(gpu):
    import llm_capi
    from _util import hip_copy_to_host
    lib = llm_capi.load()
    L, beams, H, D, ts, mt, pages = 2, 3, 2, 64, 16, 8, 60
    per_tile = L * H
    h = ctypes.c_void_p()
    llm_capi.check(lib.kv_cache_create(L, beams, H, D, ts, mt, pages, ctypes.byref(h)))

    def entries(beam):
        return [[lib.kv_cache_lookup(h, l, beam, hh, t) for t in range(mt)]
                for l in range(L) for hh in range(H)]

    try:
        llm_capi.check(lib.kv_cache_reserve(h, 0, 100))  # 7 tiles
        assert lib.kv_cache_free_pages(h) == pages - 7 * per_tile
        before = entries(0)
        # no-ops and refusals
        for n in (0, -5, 15):  # tile 0 still holds token 15
            llm_capi.check(lib.kv_cache_release_before(h, 0, n))
        assert entries(0) == before
        for bad in (-1, beams):
            assert lib.kv_cache_release_before(h, bad, 64) == llm_capi.LLM_ERR_INVALID
        assert b"beam" in lib.llm_last_error()
        # tiles wholly below token 50: 0, 1, 2
        llm_capi.check(lib.kv_cache_release_before(h, 0, 50))
        assert lib.kv_cache_free_pages(h) == pages - 4 * per_tile
        now = entries(0)
        for r, b4 in zip(now, before):
            assert r[:3] == [-1, -1, -1] and r[3:] == b4[3:]
        llm_capi.check(lib.kv_cache_release_before(h, 0, 50))  # idempotent
        llm_capi.check(lib.kv_cache_release_before(h, 0, 20))  # a lower mark frees nothing more
        assert entries(0) == now and lib.kv_cache_free_pages(h) == pages - 4 * per_tile
        # the device table reads -1 there after a sync
        llm_capi.check(lib.kv_cache_sync(h, None))
        import torch
        torch.cuda.synchronize()
        for l in range(L):
            dt = np.empty((beams, H, mt), np.int32)
            hip_copy_to_host(dt, lib.kv_cache_page_table(h, l))
            assert (dt[0, :, :3] == -1).all() and (dt[0, :, 3:7] >= 0).all()
        # a later reserve takes pages again (the freed ones among them) and
        # lowers the mark: releasing again frees them again
        freed = {p for r in before for p in r[:3]}
        llm_capi.check(lib.kv_cache_reserve(h, 0, 100))
        assert lib.kv_cache_free_pages(h) == pages - 7 * per_tile
        assert {p for r in entries(0) for p in r[:3]} & freed
        llm_capi.check(lib.kv_cache_release_before(h, 0, 48))
        assert lib.kv_cache_free_pages(h) == pages - 4 * per_tile
        # shared (forked) pages stay until the last owner lets go
        llm_capi.check(lib.kv_cache_clear(h))
        llm_capi.check(lib.kv_cache_reserve(h, 0, 64))  # 4 tiles
        llm_capi.check(lib.kv_cache_fork(h, 0, 1))
        assert lib.kv_cache_free_pages(h) == pages - 4 * per_tile
        llm_capi.check(lib.kv_cache_release_before(h, 0, 32))
        assert lib.kv_cache_free_pages(h) == pages - 4 * per_tile  # beam 1 still holds them
        assert all(r[:2] == [-1, -1] for r in entries(0))
        assert all(min(r[:4]) >= 0 for r in entries(1))
        llm_capi.check(lib.kv_cache_release_before(h, 1, 32))
        assert lib.kv_cache_free_pages(h) == pages - 2 * per_tile
        # pages put back below a beam's release mark lower it again
        llm_capi.check(lib.kv_cache_fork(h, 1, 0))  # beam 0 := beam 1 (tiles 2, 3: no change)
        llm_capi.check(lib.kv_cache_reserve(h, 0, 32))  # tiles 0, 1 again
        assert lib.kv_cache_free_pages(h) == pages - 4 * per_tile
        llm_capi.check(lib.kv_cache_release_before(h, 0, 16))
        assert lib.kv_cache_free_pages(h) == pages - 3 * per_tile
        # kv_cache_release resets the mark as well
        llm_capi.check(lib.kv_cache_release(h, 0))
        llm_capi.check(lib.kv_cache_reserve(h, 0, 48))
        free = lib.kv_cache_free_pages(h)
        llm_capi.check(lib.kv_cache_release_before(h, 0, 48))
        assert lib.kv_cache_free_pages(h) == free + 3 * per_tile
        # the LRU list forgets released entries: with the pool full, the next
        # register_tile evicts a tile that is still mapped, not a released one
        llm_capi.check(lib.kv_cache_clear(h))
        llm_capi.check(lib.kv_cache_set_eviction(h, llm_capi.LLM_EVICT_LRU))
        page = ctypes.c_int32()
        for t in range(4):
            llm_capi.check(lib.kv_cache_register_tile(h, 0, 2, 0, t, ctypes.byref(page)))
        llm_capi.check(lib.kv_cache_release_before(h, 2, 32))  # tiles 0, 1 (the oldest entries)
        llm_capi.check(lib.kv_cache_reserve(h, 1, 16 * 7))  # 28 pages
        llm_capi.check(lib.kv_cache_reserve(h, 0, 16 * 7))  # 28 pages: 58 of 60 taken
        for t in range(2):
            llm_capi.check(lib.kv_cache_register_tile(h, 1, 2, 0, t, ctypes.byref(page)))
        assert lib.kv_cache_free_pages(h) == 0
        llm_capi.check(lib.kv_cache_register_tile(h, 1, 2, 1, 0, ctypes.byref(page)))
        assert lib.kv_cache_lookup(h, 0, 2, 0, 2) == -1  # the oldest entry still listed
        assert lib.kv_cache_lookup(h, 0, 2, 0, 3) >= 0
    finally:
        lib.kv_cache_destroy(h)
    # the pybind faces
    import llm_decoder
    c = llm_decoder.KVTileCache()
    c.init(8, 16, 64, 1, 1, 1, 8, "float16")
    for t in range(4):
        c.register_tile(0, 0, t, 0)
    assert c.free_pages() == 4
    c.release_before(0, 40)
    assert c.free_pages() == 6 and c.lookup(0, 0, 1, 0) == -1 and c.lookup(0, 0, 2, 0) >= 0
    p = llm_decoder.PageTable()
    p.init(1, 2, 6)
    for t in range(5):
        p.assign(0, 1, t, t)
    p.release_before(0, 3)
    assert [p.lookup(0, 1, t) for t in range(5)] == [-1, -1, -1, 3, 4]
