"""kv_cache_reorder and the batched copy-on-write of kv_cache_sync.

Cache: L = 2, H = 2, D = 64, page 16; 4 beams of 40 tokens (2.5 tiles) with
distinct bytes per beam.  After a reorder every (beam, head, tile) entry is the
expected parent's old page and the free-page count is the one counted by hand;
after one more token per beam each tail page holds its parent's 8 old tokens
byte for byte plus the beam's own, and nothing else moved."""
import ctypes

import numpy as np
import pytest

from _util import hip_copy_to_host

pytestmark = pytest.mark.gpu

L, H, D, TS, BEAMS, T0, MT, NP = 2, 2, 64, 16, 4, 40, 4, 96
NT = 3  # tiles covering 40 tokens


class _Cache:
    def __init__(self, lib):
        import llm_capi
        self.lib, self.capi = lib, llm_capi
        h = ctypes.c_void_p()
        llm_capi.check(lib.kv_cache_create_typed(L, BEAMS, H, D, TS, MT, NP, llm_capi.LLM_F16,
                                                 ctypes.byref(h)))
        self.h = h

    def close(self):
        self.lib.kv_cache_destroy(self.h)

    def write(self, layer, beam, pos, k, v):
        k, v = np.ascontiguousarray(k), np.ascontiguousarray(v)
        self.capi.check(self.lib.kv_cache_write_tokens(self.h, layer, beam, pos, k.shape[0],
                                                       k.ctypes.data, v.ctypes.data))

    def table(self):
        return np.array([[[[self.lib.kv_cache_lookup(self.h, l, b, h, t) for t in range(MT)]
                           for h in range(H)] for b in range(BEAMS)] for l in range(L)])

    def pool(self):
        assert self.lib.kv_cache_page_stride(self.h) == 2 * TS * D * 2
        p = np.empty((NP, 2, TS, D), np.uint16)
        hip_copy_to_host(p, self.lib.kv_cache_k_pool(self.h))
        return p

    def free(self):
        return self.lib.kv_cache_free_pages(self.h)

    def cow(self):
        return self.lib.kv_cache_cow_copies(self.h)


@pytest.fixture(scope="module")
def tokens():
    """The K / V every test writes: uint16 [2 (K, V)][beam][layer][41][H][D]."""
    rng = np.random.default_rng(11)
    return rng.integers(0, 1 << 16, (2, BEAMS, L, T0 + 1, H, D), dtype=np.uint16)


def _filled(lib, tokens):
    c = _Cache(lib)
    for b in range(BEAMS):
        for l in range(L):
            c.write(l, b, 0, tokens[0, b, l, :T0], tokens[1, b, l, :T0])
    assert c.free() == NP - BEAMS * L * H * NT
    return c


@pytest.mark.parametrize("parent", [[0, 0, 1, 3], [2, 2, 2, 2], [0, 1, 2, 3], [1, 0, 3, 2]])
def test_reorder_then_append(gpu, tokens, parent):
    import llm_capi
    c = _filled(gpu, tokens)
    try:
        old = c.table()
        assert len(np.unique(old[:, :, :, :NT])) == BEAMS * L * H * NT  # nothing shared yet
        llm_capi.kv_cache_reorder(c.h.value, 0, parent, T0)
        new = c.table()
        for b in range(BEAMS):
            assert np.array_equal(new[:, b, :, :NT], old[:, parent[b], :, :NT]), b
        assert (new[:, :, :, NT:] == -1).all()
        # by hand: the pages of the distinct parents stay, every other row's are freed
        assert c.free() == NP - len(set(parent)) * L * H * NT
        assert c.cow() == 0
        llm_capi.check(gpu.kv_cache_sync(c.h, None))
        before = c.pool()
        # one more token per beam; a write syncs, so each (beam, layer) is one sync
        # whose pending copies are the heads whose tail page is still shared
        pending = []
        for b in range(BEAMS):
            for l in range(L):
                n0 = c.cow()
                c.write(l, b, T0, tokens[0, b, l, T0:], tokens[1, b, l, T0:])
                pending.append(c.cow() - n0)
        assert set(pending) <= {0, H}
        children = {p: parent.count(p) for p in set(parent)}
        # a page shared by n children is copied n - 1 times (the last owner writes in place)
        assert sum(pending) == sum(n - 1 for n in children.values()) * L * H
        if len(set(parent)) < BEAMS:
            assert H in pending  # a sync with more than one pending copy ran
        after, tab = c.pool(), c.table()
        assert c.free() == NP - L * H * (len(set(parent)) * (NT - 1) + BEAMS)
        for l in range(L):
            for h in range(H):
                tails = [int(tab[l, b, h, NT - 1]) for b in range(BEAMS)]
                assert len(set(tails)) == BEAMS, tails  # every beam owns its tail page
                for b in range(BEAMS):
                    src = parent[b]
                    for kv in (0, 1):
                        for t in range(NT):
                            pg = after[int(tab[l, b, h, t]), kv]
                            n = min(TS, T0 - t * TS)
                            want = tokens[kv, src, l, t * TS:t * TS + n, h]
                            assert np.array_equal(pg[:n], want), (l, h, b, kv, t)
                        assert np.array_equal(after[tails[b], kv, T0 % TS], tokens[kv, b, l, T0, h])
        # pages nobody wrote kept their bytes: everything but the beams' tail pages
        tails_all = {int(x) for x in tab[:, :, :, NT - 1].ravel()}
        for pg in range(NP):
            if pg not in tails_all:
                assert np.array_equal(after[pg], before[pg]), pg
    finally:
        c.close()


def test_sync_with_exactly_one_pending_copy(gpu, tokens):
    """A fork whose second head already has a private tail page: the append of
    one layer copies exactly one page (the single-copy path), byte for byte."""
    import llm_capi
    c = _filled(gpu, tokens)
    try:
        llm_capi.kv_cache_reorder(c.h.value, 0, [0, 0, 2, 3], T0)
        llm_capi.check(gpu.kv_cache_remove(c.h, 0, 1, 1, NT - 1))  # layer 0, beam 1, head 1
        pg = ctypes.c_int32(-1)
        llm_capi.check(gpu.kv_cache_register_tile(c.h, 0, 1, 1, NT - 1, ctypes.byref(pg)))
        shared = gpu.kv_cache_lookup(c.h, 0, 0, 0, NT - 1)
        assert gpu.kv_cache_lookup(c.h, 0, 1, 0, NT - 1) == shared and pg.value != shared
        n0 = c.cow()
        c.write(0, 1, T0, tokens[0, 1, 0, T0:], tokens[1, 1, 0, T0:])
        assert c.cow() - n0 == 1
        after = c.pool()
        mine = gpu.kv_cache_lookup(c.h, 0, 1, 0, NT - 1)
        assert mine != shared
        for kv in (0, 1):
            assert np.array_equal(after[mine, kv, :T0 % TS], tokens[kv, 0, 0, 2 * TS:T0, 0])
            assert np.array_equal(after[mine, kv, T0 % TS], tokens[kv, 1, 0, T0, 0])
            assert np.array_equal(after[shared, kv, :T0 % TS], tokens[kv, 0, 0, 2 * TS:T0, 0])
    finally:
        c.close()


def test_reorder_rejections(gpu, tokens):
    import llm_capi
    c = _filled(gpu, tokens)
    try:
        bad = lambda fb, par, n: gpu.kv_cache_reorder(c.h, fb, len(par), (ctypes.c_int32 * len(par))(*par), n)
        assert bad(0, [0, 4], T0) == llm_capi.LLM_ERR_INVALID       # parent outside the group
        assert bad(3, [0, 1], T0) == llm_capi.LLM_ERR_INVALID       # rows past the last beam
        assert bad(0, [0, 0], MT * TS + 1) == llm_capi.LLM_ERR_INVALID
        assert bad(2, [1, 1], T0) == llm_capi.LLM_OK                # rows 2, 3 := old row 3
        assert gpu.kv_cache_lookup(c.h, 1, 2, 1, 0) == gpu.kv_cache_lookup(c.h, 1, 3, 1, 0)
    finally:
        c.close()
