"""Blocks that outlive a row: kv_cache_hold_tile / _attach_tile / _drop_pages.

Cache: L = 2, H = 2, D = 64, page 16, 3 rows, 48 pages.  Row 0 holds 40 tokens
(two full tiles and a partial one).  Its two full tiles are held, attached to
other rows and read there by pa_decode bit for bit, survive every row's
release, and return to the pool when they are dropped."""
import ctypes

import numpy as np
import pytest

import llm_capi

pytestmark = pytest.mark.gpu

L, H, D, TS, ROWS, MT, NP, T0 = 2, 2, 64, 16, 3, 4, 48, 40
PPT = L * H
INV = llm_capi.LLM_ERR_INVALID


def _lookup(lib, h, row):
    return [[[lib.kv_cache_lookup(h, l, row, hd, t) for t in range(MT)] for hd in range(H)]
            for l in range(L)]


def _tile(lib, h, row, t):
    return [lib.kv_cache_lookup(h, l, row, hd, t) for l in range(L) for hd in range(H)]


def _decode(lib, h, q, row, ctx):
    """pa_decode of q [1][H][D] over `row`'s first ctx tokens, per layer."""
    import torch
    llm_capi.check(lib.kv_cache_sync(h, None))
    outs = []
    for l in range(L):
        view = llm_capi.PaKvView()
        llm_capi.check(lib.kv_cache_view(h, l, ctypes.byref(view)))
        out = torch.zeros((1, H, D), dtype=torch.float32, device="cuda")
        beam = torch.tensor([row], dtype=torch.int32, device="cuda")
        lens = torch.tensor([ctx], dtype=torch.int32, device="cuda")
        nbytes = lib.pa_decode_workspace_bytes(1, H, D, MT, 0)
        ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device="cuda")
        llm_capi.check(lib.pa_decode(ctypes.byref(view), llm_capi.ptr(q), llm_capi.ptr(out),
                                     llm_capi.ptr(beam), llm_capi.ptr(lens), 1, H, D, ctx,
                                     D ** -0.5, 0, llm_capi.ptr(ws), nbytes, None))
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    return np.stack(outs)


@pytest.fixture()
def cache(gpu):
    assert hasattr(gpu, "kv_cache_hold_tile"), "the library has no block entries"
    h = ctypes.c_void_p()
    llm_capi.check(gpu.kv_cache_create_typed(L, ROWS, H, D, TS, MT, NP, llm_capi.LLM_F16,
                                             ctypes.byref(h)))
    rng = np.random.default_rng(3)
    for l in range(L):
        k = rng.standard_normal((T0, H, D)).astype(np.float16)
        v = rng.standard_normal((T0, H, D)).astype(np.float16)
        llm_capi.check(gpu.kv_cache_write_tokens(h, l, 0, 0, T0, k.ctypes.data, v.ctypes.data))
    assert gpu.kv_cache_free_pages(h) == NP - 3 * PPT
    yield h
    gpu.kv_cache_destroy(h)


def test_hold_attach_drop(gpu, cache):
    import torch
    lib, h = gpu, cache
    q = torch.from_numpy(np.random.default_rng(4).standard_normal((1, H, D)).astype(np.float32)).cuda()
    want = _decode(lib, h, q, 0, 2 * TS)
    assert np.abs(want).max() > 0
    held = [llm_capi.kv_hold_tile(h, 0, t, PPT) for t in (0, 1)]
    assert held == [_tile(lib, h, 0, 0), _tile(lib, h, 0, 1)], "layer-major, head-minor"
    assert len({p for b in held for p in b}) == 2 * PPT
    assert lib.kv_cache_free_pages(h) == NP - 3 * PPT
    # attached to row 1: the same ids everywhere, and the same attention output
    for t in (0, 1):
        llm_capi.kv_attach_tile(h, 1, t, held[t])
    tab0, tab1 = _lookup(lib, h, 0), _lookup(lib, h, 1)
    for l in range(L):
        for hd in range(H):
            assert tab1[l][hd][:2] == tab0[l][hd][:2] and tab1[l][hd][2:] == [-1, -1]
    assert np.array_equal(_decode(lib, h, q, 1, 2 * TS), want)
    # the writer's row goes: only its partial tile's pages come back
    llm_capi.check(lib.kv_cache_release(h, 0))
    assert lib.kv_cache_free_pages(h) == NP - 2 * PPT
    assert np.array_equal(_decode(lib, h, q, 1, 2 * TS), want)
    # ... and with no row left the held pages stay allocated, with their contents
    llm_capi.check(lib.kv_cache_release(h, 1))
    assert lib.kv_cache_free_pages(h) == NP - 2 * PPT
    for t in (0, 1):
        llm_capi.kv_attach_tile(h, 2, t, held[t])
    assert np.array_equal(_decode(lib, h, q, 2, 2 * TS), want)
    llm_capi.check(lib.kv_cache_release(h, 2))
    assert lib.kv_cache_free_pages(h) == NP - 2 * PPT
    for b in held:
        llm_capi.kv_drop_pages(h, b)
    assert lib.kv_cache_free_pages(h) == NP, "the pool is whole again"
    assert lib.kv_cache_drop_pages(h, (ctypes.c_int32 * PPT)(*held[0])) == INV  # free pages
    assert lib.kv_cache_free_pages(h) == NP
    assert lib.kv_cache_cow_copies(h) == 0


def test_refusals_change_nothing(gpu, cache):
    lib, h = gpu, cache
    buf = (ctypes.c_int32 * PPT)(*([-7] * PPT))
    # row 1, tile 0: one entry of four mapped
    page = ctypes.c_int32(-1)
    llm_capi.check(lib.kv_cache_register_tile(h, 0, 1, 0, 0, ctypes.byref(page)))
    free = lib.kv_cache_free_pages(h)
    assert free == NP - 3 * PPT - 1
    assert lib.kv_cache_hold_tile(h, 1, 0, buf) == INV
    assert b"not mapped" in lib.llm_last_error()
    assert list(buf) == [-7] * PPT
    assert lib.kv_cache_hold_tile(h, 0, 3, buf) == INV      # nothing mapped at all
    assert lib.kv_cache_hold_tile(h, ROWS, 0, buf) == INV   # no such row
    assert lib.kv_cache_hold_tile(h, 0, MT, buf) == INV     # no such tile
    # the partly mapped tile takes no attach, and neither does a full one
    good = llm_capi.kv_hold_tile(h, 0, 0, PPT)
    before = _lookup(lib, h, 1)
    pages = (ctypes.c_int32 * PPT)(*good)
    assert lib.kv_cache_attach_tile(h, 1, 0, pages) == INV
    assert b"mapped entry" in lib.llm_last_error()
    assert lib.kv_cache_attach_tile(h, 0, 1, pages) == INV
    assert _lookup(lib, h, 1) == before
    # pages that are not allocated (free, or no page at all) are not attached
    unallocated = (ctypes.c_int32 * PPT)(*([good[0]] * (PPT - 1) + [NP - 1]))
    assert lib.kv_cache_attach_tile(h, 2, 0, unallocated) == INV
    assert lib.kv_cache_attach_tile(h, 2, 0, (ctypes.c_int32 * PPT)(*([NP] * PPT))) == INV
    assert _lookup(lib, h, 2) == [[[-1] * MT] * H] * L
    assert lib.kv_cache_free_pages(h) == free
    # the references are what they were: one drop of the hold, one release per row
    llm_capi.kv_drop_pages(h, good)
    for row in range(ROWS):
        llm_capi.check(lib.kv_cache_release(h, row))
    assert lib.kv_cache_free_pages(h) == NP
    assert lib.kv_cache_cow_copies(h) == 0
