"""Host side of the packed prefill attention (pa_prefill_packed, llm_decoder.h):
the tile table, the status codes and the workspace sizes.  Everything here is
decided on the host before any launch, so a fake view (pointers that are never
dereferenced) is enough and no GPU is needed."""
import ctypes

import numpy as np


def _view(llm_capi, *, kv_dtype=None, num_beams=8, H=2, D=64, ts=16, max_tiles=64):
    return llm_capi.PaKvView(k_pool=16, v_pool=16, page_table=16, num_pages=4, page_size=ts,
                             head_dim=D, num_beams=num_beams, num_heads=H, max_tiles=max_tiles,
                             kv_dtype=llm_capi.LLM_F16 if kv_dtype is None else kv_dtype)


def _tiles(llm_capi, view, segs, cap=None):
    lib = llm_capi.load()
    arr = llm_capi.prefill_segs(segs)
    n = lib.pa_prefill_packed_tiles(ctypes.byref(view), arr, len(segs), None, 0)
    if n < 0:
        return n, None
    cap = n if cap is None else cap
    t = np.full((max(cap, 1), 4), -7, np.int32)
    got = lib.pa_prefill_packed_tiles(ctypes.byref(view), arr, len(segs),
                                      t.ctypes.data_as(llm_capi.c_i32p), cap)
    assert got == n
    return n, t


def test_tile_table_covers_every_row_once():
    import llm_capi
    lens = [5, 64, 17, 1, 65, 130]
    rows = [3, 0, 5, 1, 7, 2]
    p0s = [0, 100, 37, 900, 16, 1]
    segs = list(zip(rows, p0s, lens))
    view = _view(llm_capi)
    n, t = _tiles(llm_capi, view, segs)
    assert n == sum((l + 63) // 64 for l in lens) == len(t)
    start = np.concatenate([[0], np.cumsum(lens)])
    seen = np.zeros(start[-1], np.int32)
    for q0, nq, row, p0 in t:
        assert 1 <= nq <= 64
        seen[q0:q0 + nq] += 1
        j = int(np.searchsorted(start, q0, side="right") - 1)   # the tile's segment
        assert q0 + nq <= start[j + 1], "a tile straddles two segments"
        assert row == rows[j]
        assert p0 == p0s[j] + (q0 - start[j])
    assert (seen == 1).all()
    # tiles in packed order; only a segment's last tile is short
    assert (np.diff(t[:, 0]) > 0).all()
    for j, l in enumerate(lens):
        mine = t[(t[:, 0] >= start[j]) & (t[:, 0] < start[j + 1])]
        assert len(mine) == (l + 63) // 64 and (mine[:-1, 1] == 64).all()
    # a table that is too small (or NULL) still returns the count and writes nothing
    n2, t2 = _tiles(llm_capi, view, segs, cap=n - 1)
    assert n2 == n and (t2 == -7).all()


def _call(llm_capi, view, segs, *, nseg=None, q=16, out=16, q_stride=0, out_stride=0, ws=16,
          ws_bytes=1 << 40):
    lib = llm_capi.load()
    arr = llm_capi.prefill_segs(segs)
    return lib.pa_prefill_packed(ctypes.byref(view), ctypes.c_void_p(q), q_stride,
                                 ctypes.c_void_p(out), out_stride, arr,
                                 len(segs) if nseg is None else nseg, 1.0,
                                 ctypes.c_void_p(ws), ws_bytes, None)


def test_status_codes():
    import llm_capi
    lib = llm_capi.load()
    INV, UNS = llm_capi.LLM_ERR_INVALID, llm_capi.LLM_ERR_UNSUPPORTED
    view = _view(llm_capi)   # 8 rows, 64 tiles of 16: positions < 1024
    ok = [(0, 0, 5), (1, 10, 70)]
    bad = {
        "nseg < 1": dict(segs=ok, nseg=0),
        "len < 1": dict(segs=[(0, 0, 5), (1, 10, 0)]),
        "p0 < 0": dict(segs=[(0, -1, 5)]),
        "row < 0": dict(segs=[(-1, 0, 5)]),
        "row outside the table": dict(segs=[(0, 0, 5), (8, 0, 5)]),
        "repeated row": dict(segs=[(2, 0, 5), (1, 0, 5), (2, 64, 5)]),
        "past max_tiles": dict(segs=[(0, 1020, 5)]),
        "misaligned q stride": dict(segs=ok, q_stride=2 * 64 + 2),
        "short q stride": dict(segs=ok, q_stride=64),
        "short out stride": dict(segs=ok, out_stride=64),
        "misaligned q": dict(segs=ok, q=20),
        "misaligned out": dict(segs=ok, out=24),
        "no workspace": dict(segs=ok, ws=0, ws_bytes=0),
    }
    for name, kw in bad.items():
        assert _call(llm_capi, view, **kw) == INV, name
        assert lib.llm_last_error(), name
    # the same lists are refused by the helpers: no tile count, no size
    for name in ("len < 1", "p0 < 0", "row outside the table", "repeated row", "past max_tiles"):
        segs = bad[name]["segs"]
        assert _tiles(llm_capi, view, segs)[0] < 0, name
        arr = llm_capi.prefill_segs(segs)
        assert lib.pa_prefill_packed_workspace_bytes(ctypes.byref(view), arr, len(segs), 1) == 0
    # a workspace below the one-pass size
    arr = llm_capi.prefill_segs(ok)
    need0 = lib.pa_prefill_packed_workspace_bytes(ctypes.byref(view), arr, len(ok), 0)
    assert _call(llm_capi, view, ok, ws_bytes=need0 - 1) == INV
    assert b"workspace" in lib.llm_last_error()
    # int8 pools, and a head_dim the MFMA kernel is not built for
    assert _call(llm_capi, _view(llm_capi, kv_dtype=llm_capi.LLM_I8), ok) == UNS
    assert _call(llm_capi, _view(llm_capi, D=256), ok) == UNS
    assert lib.pa_prefill_packed(None, None, 0, None, 0, None, 0, 1.0, None, 0, None) == INV


def test_workspace_sizes_monotone():
    import llm_capi
    lib = llm_capi.load()
    for H, D, ts in ((2, 64, 16), (16, 128, 16), (3, 128, 32)):
        view = _view(llm_capi, H=H, D=D, ts=ts, max_tiles=1024, num_beams=64)
        for segs in ([(0, 0, 1)], [(0, 0, 5), (1, 0, 64), (2, 0, 17)],
                     [(1, 1000, 70), (3, 0, 1), (0, 37, 65), (2, 16, 16)],
                     [(r, 120, 8) for r in range(64)], [(0, 7680, 512)]):
            arr = llm_capi.prefill_segs(segs)
            s0 = lib.pa_prefill_packed_workspace_bytes(ctypes.byref(view), arr, len(segs), 0)
            s1 = lib.pa_prefill_packed_workspace_bytes(ctypes.byref(view), arr, len(segs), 1)
            m = sum(s[2] for s in segs)
            ntile = sum((s[2] + 63) // 64 for s in segs)
            assert s1 >= s0 > 0
            assert s0 >= 4 * (4 * ntile + m)   # the tile table and the context lengths
            end = max(s[1] + s[2] for s in segs)
            if end <= 64:   # the longest segment ends within 64 positions: one split
                assert s1 == s0
            else:           # no partials, or those of 2 .. 128 splits: (D + 2) floats
                per = m * H * (D + 2) * 4                       # per (row, head, split)
                assert (s1 - s0) % per == 0
                assert (s1 - s0) // per == 0 or 2 <= (s1 - s0) // per <= 128


def test_new_symbols_exported():
    import llm_capi
    lib = llm_capi.load()
    declared = llm_capi.declared_symbols()
    for name in ("pa_prefill_packed", "pa_prefill_packed_tiles", "pa_prefill_packed_workspace_bytes",
                 "llm_decoder_prefill_rows", "llm_decoder_set_packed_prefill",
                 "llm_decoder_packed_prefill"):
        assert name in declared, name
        assert hasattr(lib, name), name
    assert lib.llm_abi_version() == 3
    assert lib.llm_decoder_packed_prefill(None) == -1
