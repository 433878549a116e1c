"""The serving scheduler with its prefix cache (csrc/serve_plan.hpp,
csrc/prefix_cache.hpp) through the tuning library's serve_prefix_sim_tune: the
decisions llm_decoder_serve_step executes, without a device.

Every request is submitted before step 1 and request i ends after gen_lens[i]
tokens.  Records are (step, kind, id, row, aux, aux2): serve_plan_sim's four
kinds (an admission's aux2 = hit_blocks), DEFER (id = the head kept waiting by
the same-step rule), EVICT (id = block, aux = its tile index), PUBLISH (id =
request, aux = block, aux2 = tile index) and the two STATE records of a step
(aux = committed, aux2 = idle_pages; after the admissions and publications,
and after the retirements).
"""
import ctypes
import random

import llm_capi
from llm_capi import SERVE_ADMIT as ADMIT, SERVE_MOVE as MOVE, SERVE_RETIRE as RETIRE, \
    SERVE_TOKEN as TOKEN

P, PPT = 16, 8
GEOM = dict(max_rows=4, num_pages=1000, pages_per_tile=PPT, page_size=P, max_seq_len=640)


def _entry():
    tune = llm_capi.load_tune()
    assert hasattr(tune, "serve_prefix_sim_tune"), "the tuning library has no prefix simulation"
    return tune


def sim(prompts, max_new, gen_lens=None, cache=True, **geom):
    _entry()
    return llm_capi.serve_prefix_sim(prompts, max_new, gen_lens or max_new, prefix_cache=cache,
                                     **geom)


def of(recs, kind):
    return [r for r in recs if r[1] == kind]


def _abc():
    rng = random.Random(5)
    a = [rng.randrange(300) for _ in range(40)]
    b = a[:32] + [300 + i for i in range(8)]
    return a, b, a[:33]


def test_exact_case():
    a, b, c = _abc()
    recs, stats = sim([a, b, c], [3, 3, 2], **GEOM)
    # step 1: A alone, B deferred (A will publish its block 0), C behind it
    assert [r[2:] for r in of(recs, ADMIT) if r[0] == 1] == [(0, 0, 24, 0)]
    assert [(r[0], r[2]) for r in of(recs, llm_capi.SERVE_DEFER)] == [(1, 1)]
    assert [(r[0], r[2], r[5]) for r in of(recs, llm_capi.SERVE_PUBLISH)] == [(1, 0, 0), (1, 0, 1)]
    # step 2: B and C, two blocks hit each; nothing more is published
    assert [r[2:] for r in of(recs, ADMIT) if r[0] == 2] == [(1, 1, 32, 2), (2, 2, 40, 2)]
    state = {r[0]: r[4:] for r in of(recs, llm_capi.SERVE_STATE_ADMITTED)}
    assert state[1] == (24, 0) and state[2] == (40, 0)
    assert [(r[0], r[2]) for r in of(recs, RETIRE)] == [(3, 2), (3, 0), (4, 1)]
    end = {r[0]: r[4:] for r in of(recs, llm_capi.SERVE_STATE_END)}
    assert end[4] == (0, 16) and max(r[0] for r in recs) == 4
    assert stats == dict(positions_due=110, positions_hit=64, cached_blocks=2, idle_pages=16,
                         evicted_blocks=0, deferrals=1)
    # cache off: everything enters at step 1 and is charged in full
    off, zero = sim([a, b, c], [3, 3, 2], cache=False, **GEOM)
    assert [r[2:] for r in of(off, ADMIT)] == [(0, 0, 24, 0), (1, 1, 48, 0), (2, 2, 72, 0)]
    assert {r[0]: r[4:] for r in of(off, llm_capi.SERVE_STATE_ADMITTED)}[2] == (72, 0)
    assert set(zero.values()) == {0}


def test_exact_eviction_case():
    """Pool 40.  D (need 32) waits until B ends; 0 + 16 idle + 32 > 40 then, so
    one block goes: block 1, the leaf.  E = A[:17] hits block 0 afterwards."""
    a, b, c = _abc()
    d = [400 + i for i in range(17)]
    e = a[:17]
    recs, stats = sim([a, b, c, d, e], [3, 3, 2, 48, 1], **dict(GEOM, num_pages=40))
    pub = {r[4]: r[5] for r in of(recs, llm_capi.SERVE_PUBLISH) if r[2] == 0}  # A's: block -> tile
    assert sorted(pub.values()) == [0, 1]
    ev = of(recs, llm_capi.SERVE_EVICT)
    assert len(ev) == 1 and ev[0][0] == 5 and ev[0][4] == 1 and pub[ev[0][2]] == 1
    adm = {r[2]: r for r in of(recs, ADMIT)}
    assert adm[3][0] == 5 and adm[3][4:] == (32, 0)
    assert {r[0]: r[4:] for r in of(recs, llm_capi.SERVE_STATE_END)}[4] == (0, 16)
    assert adm[4][5] == 1, "A[:17] hits the block that stayed"
    assert adm[4][0] == 5 + 48, "E (8 private + block 0's 8) waits for D's 32 of 40"
    assert stats["evicted_blocks"] == 1 and stats["positions_hit"] == 64 + 16
    for r in recs:
        if r[1] in (llm_capi.SERVE_STATE_ADMITTED, llm_capi.SERVE_STATE_END):
            assert r[4] + r[5] <= 40


def _plain(recs):
    return [r[:5] for r in recs if r[1] <= RETIRE]


def test_cache_off_is_serve_plan_sim():
    a, b, c = _abc()
    for pool in (1000, 40, 24):
        geom = dict(GEOM, num_pages=pool)
        off, _ = sim([a, b, c], [3, 3, 2], cache=False, **geom)
        assert _plain(off) == llm_capi.serve_plan_sim([40, 40, 33], [3, 3, 2], [3, 3, 2], **geom)
        assert all(r[5] == 0 for r in off if r[1] <= RETIRE)


def _workload(rng, ps):
    headers = [[rng.randrange(50) for _ in range(ps * rng.randrange(0, 6))] for _ in range(3)]
    n = rng.randrange(1, 20)
    prompts = []
    for _ in range(n):
        p = rng.choice(headers) + [rng.randrange(50) for _ in range(rng.choice(
            [0, 1, 2, ps, ps + 1, rng.randrange(0, 40)]))]
        prompts.append(p or [rng.randrange(50)])
    max_new = [rng.choice([1, 2, rng.randrange(1, 40)]) for _ in range(n)]
    gen = [rng.choice([m, rng.randrange(1, m + 1)]) for m in max_new]
    return prompts, max_new, gen


def _replay(prompts, max_new, gen, recs, stats, pool, ps, ppt, max_rows):
    """Replays the records against a model of the cache built from the prompts
    alone, and asserts the scheduler's properties at every record."""
    n = len(prompts)
    tiles = [(len(p) + m - 1 + ps - 1) // ps for p, m in zip(prompts, max_new)]
    cached, by_id = {}, {}      # prefix tuple -> users; block id -> prefix tuple
    private, uses = {}, {}      # live request -> private pages; -> the prefixes it uses
    rows, got = {}, {i: [] for i in range(n)}
    deferred = None             # (step, id) of the last DEFER record
    admitted, evicted, hit_total, last_step = [], 0, 0, 0

    def committed():
        return sum(private.values()) + ppt * sum(u > 0 for u in cached.values())

    def idle():
        return ppt * sum(u == 0 for u in cached.values())

    for step, kind, rid, row, aux, aux2 in recs:
        assert step >= last_step
        if step != last_step:
            assert sorted(rows) == list(range(len(rows))), "rows dense after every step"
        last_step = step
        if kind == ADMIT:
            if deferred:
                assert deferred == (step - 1, rid), "a deferred head enters at the next step"
                deferred = None
            p = prompts[rid]
            chain = 0
            while chain < (len(p) - 1) // ps and tuple(p[:(chain + 1) * ps]) in cached:
                chain += 1
            assert aux2 == chain <= (len(p) - 1) // ps, "the longest cached chain from the root"
            uses[rid] = [tuple(p[:(k + 1) * ps]) for k in range(chain)]
            for pre in uses[rid]:
                cached[pre] += 1
            private[rid] = (tiles[rid] - chain) * ppt
            hit_total += chain * ps
            assert row == len(rows) < max_rows
            rows[row] = rid
            admitted.append(rid)
            assert aux == committed() and aux + idle() <= pool
        elif kind == llm_capi.SERVE_DEFER:
            assert deferred is None and row == -1
            assert rid == len(admitted), "the head of the queue"
            assert any(r[0] == step and r[1] == ADMIT for r in recs), "after another admission"
            deferred = (step, rid)
        elif kind == llm_capi.SERVE_PUBLISH:
            p = prompts[rid]
            pre = tuple(p[:(aux2 + 1) * ps])
            assert rows[row] == rid and aux2 == len(uses[rid]) < (len(p) - 1) // ps
            assert pre not in cached and aux not in by_id
            cached[pre] = 1
            by_id[aux] = pre
            uses[rid].append(pre)
            private[rid] -= ppt
            assert private[rid] >= ppt, "the tile of position n - 1 stays private"
        elif kind == llm_capi.SERVE_EVICT:
            pre = by_id.pop(rid)
            assert len(pre) == (aux + 1) * ps
            assert cached.pop(pre) == 0, "an evicted block is idle"
            assert not any(len(k) == len(pre) + ps and k[:len(pre)] == pre for k in cached), \
                "an evicted block has no cached child"
            evicted += 1
        elif kind in (llm_capi.SERVE_STATE_ADMITTED, llm_capi.SERVE_STATE_END):
            assert (aux, aux2) == (committed(), idle()) and aux + aux2 <= pool
        elif kind == TOKEN:
            assert rows[row] == rid
            got[rid].append(aux)
        elif kind == RETIRE:
            assert rows.pop(row) == rid
            del private[rid]
            for pre in uses.pop(rid):
                cached[pre] -= 1
                assert cached[pre] >= 0, "users never negative"
            assert aux == (2 if gen[rid] == max_new[rid] else 1)
        else:
            assert kind == MOVE and row not in rows and rows[aux] == rid
            rows[row] = rows.pop(aux)
    assert deferred is None and not rows and not private
    assert admitted == list(range(n)), "admissions in id order, every request once"
    assert last_step <= sum(gen), "the run terminates: a token at least per step"
    for i in range(n):
        assert got[i] == list(range(gen[i]))
    assert stats == dict(positions_due=sum(len(p) - 1 for p in prompts), positions_hit=hit_total,
                         cached_blocks=len(cached), idle_pages=idle(), evicted_blocks=evicted,
                         deferrals=len(of(recs, llm_capi.SERVE_DEFER)))
    return hit_total, evicted


def test_properties_random():
    rng = random.Random(20261)
    hits = evictions = deferrals = 0
    for _ in range(250):
        ps, ppt = rng.choice([4, 16]), rng.choice([1, 2, 8])
        max_rows = rng.choice([1, 2, 3, 4, 8])
        prompts, max_new, gen = _workload(rng, ps)
        need = [(len(p) + m - 1 + ps - 1) // ps * ppt for p, m in zip(prompts, max_new)]
        for mult in (1, 2, 5):  # down to the largest single need
            pool = max(need) * mult
            geom = dict(max_rows=max_rows, num_pages=pool, pages_per_tile=ppt, page_size=ps,
                        max_seq_len=400)
            recs, stats = sim(prompts, max_new, gen, **geom)
            h, e = _replay(prompts, max_new, gen, recs, stats, pool, ps, ppt, max_rows)
            hits, evictions, deferrals = hits + h, evictions + e, deferrals + stats["deferrals"]
            off, zero = sim(prompts, max_new, gen, cache=False, **geom)
            assert _plain(off) == llm_capi.serve_plan_sim([len(p) for p in prompts], max_new, gen,
                                                          **geom)
            assert set(zero.values()) == {0}
    assert hits > 0 and evictions > 0 and deferrals > 0, "the workloads exercise every path"


def test_refused_room_and_bad_arguments():
    tune = _entry()
    i32 = ctypes.c_int32
    tok = (i32 * 6)(1, 2, 3, 1, 2, 3)
    a = (i32 * 2)(3, 3)
    geom = (2, 2, 100, 1, 16, 64)  # n, max_rows, num_pages, pages_per_tile, page_size, max_seq_len
    out = (ctypes.c_longlong * 12)(*([-7] * 12))
    # 2 admits, 6 tokens, 2 retires and 2 states in each of 3 steps: 16 records, with or without the cache
    for cache in (0, 1):
        assert tune.serve_prefix_sim_tune(tok, a, a, a, *geom, cache, None, 0, None) == -16
    assert tune.serve_prefix_sim_tune(tok, a, a, a, *geom, 1, out, 2, None) == -16
    assert list(out) == [1, ADMIT, 0, 0, 1, 0, 1, ADMIT, 1, 1, 2, 0]
    full = (ctypes.c_longlong * 96)()
    stats = (ctypes.c_longlong * 6)()
    assert tune.serve_prefix_sim_tune(tok, a, a, a, *geom, 1, full, 16, stats) == 16
    assert list(stats) == [4, 0, 0, 0, 0, 0]
    bad = -2 ** 31
    assert tune.serve_prefix_sim_tune(None, a, a, a, *geom, 1, None, 0, None) == bad
    assert tune.serve_prefix_sim_tune(tok, None, a, a, *geom, 1, None, 0, None) == bad
    assert tune.serve_prefix_sim_tune(tok, a, a, a, *geom, 2, None, 0, None) == bad
    assert tune.serve_prefix_sim_tune(tok, a, a, a, *geom, 1, None, 4, None) == bad  # room, no out
    assert tune.serve_prefix_sim_tune(tok, a, a, a, 2, 0, 100, 1, 16, 64, 1, None, 0, None) == bad
    assert tune.serve_prefix_sim_tune(tok, a, a, a, 2, 2, 100, 1, 0, 64, 1, None, 0, None) == bad
    z = (i32 * 2)(3, 4)
    assert tune.serve_prefix_sim_tune(tok, a, a, z, *geom, 1, None, 0, None) == bad  # gen > max_new
    assert tune.serve_prefix_sim_tune(tok, a, a, a, 0, 2, 100, 1, 16, 64, 1, None, 0, None) == 0
    # a refused request refuses the run: T = 5 > max_seq_len 4; need 5 > 4 pages
    assert tune.serve_prefix_sim_tune(tok, a, a, a, 2, 2, 100, 1, 16, 4, 1, None, 0, None) == -1
    assert tune.serve_prefix_sim_tune(tok, a, a, a, 2, 2, 4, 1, 1, 64, 1, None, 0, None) == -1


def test_null_arguments_of_the_c_entries():
    """The new library entries answer NULL with LLM_ERR_INVALID on the host."""
    lib = llm_capi.load()
    inv = llm_capi.LLM_ERR_INVALID
    for name in ("llm_decoder_serve_begin_opts", "llm_decoder_serve_prefix_stats",
                 "kv_cache_hold_tile", "kv_cache_attach_tile", "kv_cache_drop_pages"):
        assert hasattr(lib, name), name
    opt, st = llm_capi.LlmServeOptions(1), llm_capi.LlmPrefixStats()
    pages = (ctypes.c_int32 * 4)()
    assert lib.llm_decoder_serve_begin_opts(None, ctypes.byref(opt)) == inv
    assert lib.llm_decoder_serve_prefix_stats(None, ctypes.byref(st)) == inv
    assert b"llm_decoder_serve_prefix_stats" in lib.llm_last_error()
    assert lib.kv_cache_hold_tile(None, 0, 0, pages) == inv
    assert lib.kv_cache_attach_tile(None, 0, 0, pages) == inv
    assert lib.kv_cache_drop_pages(None, pages) == inv
    assert lib.llm_abi_version() == 3
