"""Prefix caching while serving (llm_decoder_serve_begin_opts, prefix_cache):
shared prompt blocks against a cache-less decoder, the bookkeeping against the
CPU simulation, pool pressure, cancel, the walls and generate_many.

The models and helpers are tests/test_serve_gpu.py's (L 2 / H 4 / D 64, V 300,
max_seq 640, max_batch 4).  The workload is seven requests over two headers:

  id 0  HA (48 tokens) + 9          publishes HA's three blocks
  id 1  HA + 21 others              deferred in step 1, then hits 48 positions
                                    (a page boundary that is no multiple of 64)
  id 2  id 0's first 49 tokens      hits 48 of its 48 positions: prefills nothing
  id 3  33 tokens of its own        shares nothing
  id 4  HB (528 tokens) + 2         two prefill chunks; publishes 33 blocks
  id 5  HB + 2 others               hits 528 of 529 positions, across the
                                    512-token chunk boundary
  id 6  HA's first 32 tokens + 20   hits two of HA's blocks, publishes a third

The yardstick is test_serve_gpu's: a cache-less max_batch = 1 decoder per
request fed the served ids (_check_solo), at 2 * LOGIT_TOL for fp16 weights
and FREE_RUN_TOL through int8 -- the project's bars between two paths of one
decoder.
"""
import ctypes

import numpy as np
import pytest

import llm_capi
from _util import record
from test_decoder_gpu import FREE_RUN_TOL, LOGIT_TOL
from test_serve_gpu import (H, L, MAXB, S, V, Run, _check_solo, _kv, _make, _sim_steps,  # noqa: F401
                            _torch, f16_weights, int8_weights)

pytestmark = pytest.mark.gpu

P, PPT = 16, L * H
MAX_NEW = [6, 9, 4, 5, 6, 3, 7]
ZERO = dict.fromkeys(llm_capi.PREFIX_STATS, 0)


def _workload(seed=41):
    rng = np.random.default_rng(seed)
    tok = lambda n: rng.integers(0, V, n).tolist()
    ha, hb = tok(48), tok(528)
    p0 = ha + tok(9)
    return [p0, ha + tok(21), p0[:49], tok(33), hb + tok(2), hb + tok(2), ha[:32] + tok(20)]


def _drive(dec, prompts, max_new, cache=True, before=None, after=None):
    """test_serve_gpu._serve with the option: submit everything, step until
    nothing is live or waiting.  before(step, dec) runs ahead of each step,
    after(step, events, dec) behind it.  The Run also carries, per step, the
    pages committed after it."""
    torch = _torch()
    buf = torch.empty((MAXB, V), device="cuda")
    run = Run()
    run.committed = []
    dec.serve_begin(prefix_cache=cache)
    for i, (p, m) in enumerate(zip(prompts, max_new)):
        assert dec.submit(p, m) == i
    step = 0
    while True:
        step += 1
        if before:
            before(step, dec)
        st = dec.serve_stats()
        if st["live"] + st["waiting"] == 0:
            break
        ev = dec.serve_step(buf.data_ptr())
        assert 1 <= len(ev) <= MAXB
        lg = buf.cpu().numpy()
        for rid, tok, idx, row, fin in ev:
            assert idx == len(run.ids.setdefault(rid, []))
            run.ids[rid].append(tok)
            run.logits.setdefault(rid, []).append(lg[row].copy())
            if fin:
                run.finish[rid] = fin
        run.steps.append(ev)
        run.live_counts.append(len(ev))
        run.committed.append(dec.serve_stats()["committed_pages"])
        if after:
            after(step, ev, dec)
        assert step < 500
    return run


def _sim(prompts, max_new, num_pages, gen=None, cache=True):
    return llm_capi.serve_prefix_sim(prompts, max_new, gen or max_new, max_rows=MAXB,
                                     num_pages=num_pages, pages_per_tile=PPT, page_size=P,
                                     max_seq_len=S, prefix_cache=cache)


def _check_against_sim(run, stats, prompts, max_new, num_pages, gen=None):
    recs, sim_stats = _sim(prompts, max_new, num_pages, gen)
    assert len(run.steps) == max(r[0] for r in recs)
    assert stats == sim_stats
    assert run.committed == [r[4] for r in recs if r[1] == llm_capi.SERVE_STATE_END]
    tokens = {}
    for step, kind, rid, row, *_ in recs:
        if kind == llm_capi.SERVE_TOKEN:
            tokens.setdefault(step, []).append((rid, row))
    assert [[(e[0], e[3]) for e in ev] for ev in run.steps] == [tokens[s] for s in sorted(tokens)]
    return recs, sim_stats


def _shared_tiles(dec, ev, prompts):
    """Over the live pairs of a step without a retirement (the events' rows
    still hold): the number of tiles on which two requests whose prompts agree
    up to the tile's end map the same pages, all layers and heads.  Asserts
    that a tile both could have shared is shared when either hit or published
    it (its pages are equal) or private to both (all different)."""
    lib, h = llm_capi.load(), ctypes.c_void_p(dec.kv_handle)
    tile = lambda row, t: [lib.kv_cache_lookup(h, l, row, hd, t) for l in range(L)
                           for hd in range(H)]
    same = 0
    for i, (ra, _, _, rowa, _) in enumerate(ev):
        for rb, _, _, rowb, _ in ev[i + 1:]:
            a, b = prompts[ra], prompts[rb]
            for t in range(min(len(a) - 1, len(b) - 1) // P):
                if a[:(t + 1) * P] != b[:(t + 1) * P]:
                    break
                ta, tb = tile(rowa, t), tile(rowb, t)
                assert min(ta) >= 0 and min(tb) >= 0
                assert ta == tb or not set(ta) & set(tb)
                same += ta == tb
    return same


CONFIGS = [("f16", dict(), 2 * LOGIT_TOL), ("int8", dict(), FREE_RUN_TOL),
           ("int8_fp8kv", dict(kv_dtype="fp8"), FREE_RUN_TOL),
           ("int8_rope", dict(rope=True), FREE_RUN_TOL),
           ("int8_packed_prefill", dict(packed=True), FREE_RUN_TOL)]


@pytest.mark.parametrize("name,cfg,tol", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_parity_and_bookkeeping(gpu, request, name, cfg, tol):
    w = request.getfixturevalue("f16_weights" if name == "f16" else "int8_weights")
    dec = _make(w, MAXB, **cfg)
    assert hasattr(dec, "serve_prefix_stats"), "the decoder has no prefix cache"
    prompts = _workload()
    kv0 = _kv(dec)
    shared = []

    def after(step, ev, d):
        if not any(e[4] for e in ev):
            shared.append(_shared_tiles(d, ev, prompts))

    run = _drive(dec, prompts, MAX_NEW, after=after)
    stats = dec.serve_prefix_stats()
    assert [len(run.ids[i]) for i in range(7)] == MAX_NEW
    recs, _ = _check_against_sim(run, stats, prompts, MAX_NEW, kv0["pages"])
    hits = {r[2]: r[5] for r in recs if r[1] == llm_capi.SERVE_ADMIT}
    assert hits == {0: 0, 1: 3, 2: 3, 3: 0, 4: 0, 5: 33, 6: 2}, "the workload's hits"
    assert stats["positions_hit"] == 16 * 41 and stats["deferrals"] >= 1
    assert stats["positions_due"] == sum(len(p) - 1 for p in prompts)
    assert max(shared) >= 33, "a publisher and its hitter were live together on shared pages"
    kv1 = _kv(dec)
    assert kv1["cow"] == kv0["cow"], "a shared tile was appended to"
    assert stats["idle_pages"] == PPT * stats["cached_blocks"] > 0
    assert kv1["free"] == kv1["pages"] - PPT * stats["cached_blocks"]
    assert dec.serve_stats()["committed_pages"] == 0
    dec.serve_end()
    assert _kv(dec)["free"] == kv1["pages"] and dec.serve_prefix_stats() == ZERO
    # a new session starts with an empty index: id 2's prompt alone hits nothing
    dec.serve_begin(prefix_cache=True)
    dec.submit(prompts[2], 1)
    assert len(dec.serve_step()) == 1
    again = dec.serve_prefix_stats()
    assert (again["positions_hit"], again["positions_due"], again["cached_blocks"]) == (0, 48, 3)
    dec.serve_end()
    solo_cfg = {k: v for k, v in cfg.items() if k != "packed"}
    worst = _check_solo(_make(w, 1, **solo_cfg), prompts, run, tol)
    record("serve_prefix", test=name, logit_err=worst, steps=len(run.steps),
           hit=stats["positions_hit"], due=stats["positions_due"])


def test_pool_pressure(gpu, int8_weights):
    """48 pages; every request needs 24 (T = 40: three tiles of 8 pages) and
    leaves two idle blocks behind, so later requests enter only over evicted
    blocks; ha's blocks, hit by id 1, are gone before id 5 asks for them again."""
    dec = _make(int8_weights, MAXB, num_pages=48)
    rng = np.random.default_rng(43)
    tok = lambda n: rng.integers(0, V, n).tolist()
    ha, hb, hc = tok(32), tok(32), tok(32)
    prompts = [h + tok(5) for h in (ha, ha, hb, hb, hc, ha, hc)]
    max_new = [4] * 7
    run = _drive(dec, prompts, max_new)  # (an LLM_ERR_OOM of a step would raise)
    stats = dec.serve_prefix_stats()
    assert [len(run.ids[i]) for i in range(7)] == max_new
    _, sim_stats = _check_against_sim(run, stats, prompts, max_new, 48)
    assert stats["evicted_blocks"] == sim_stats["evicted_blocks"] > 0
    assert stats["positions_hit"] > 0
    assert max(run.committed) <= 48
    kv = _kv(dec)
    assert kv["free"] == 48 - PPT * stats["cached_blocks"] and kv["cow"] == 0
    dec.serve_end()
    assert _kv(dec)["free"] == 48
    _check_solo(_make(int8_weights, 1), prompts, run, FREE_RUN_TOL)


def test_cancel_of_a_block_user(gpu, int8_weights):
    """Id 1 (it hit HA's blocks and published a fourth) is cancelled while ids
    0, 2 and 3 are live: the blocks stay cached, id 6 still hits two of them,
    and everybody else keeps the solo parity."""
    dec = _make(int8_weights, MAXB)
    prompts = _workload(seed=45)
    seen = {}

    def before(step, d):
        if step == 4:
            cached = d.serve_prefix_stats()["cached_blocks"]
            d.cancel(1)
            seen.update(d.serve_prefix_stats(), was=cached)

    run = _drive(dec, prompts, MAX_NEW, before=before)
    assert len(run.ids[1]) == 2 and 1 not in run.finish
    assert seen["cached_blocks"] == seen["was"] >= 4, "a cancel evicts nothing"
    assert seen["idle_pages"] == PPT, "the block id 1 published; ids 0 and 2 still use HA's"
    keep = [0, 2, 3, 4, 5, 6]
    assert [len(run.ids[i]) for i in keep] == [MAX_NEW[i] for i in keep]
    stats = dec.serve_prefix_stats()
    assert stats["positions_hit"] == 16 * 41, "id 6 hit what id 1 had been using"
    kv = _kv(dec)
    assert kv["free"] == kv["pages"] - PPT * stats["cached_blocks"] and kv["cow"] == 0
    assert dec.serve_stats()["committed_pages"] == 0
    dec.serve_end()
    _check_solo(_make(int8_weights, 1), prompts, run, FREE_RUN_TOL, only=keep)


def test_walls_and_the_option_off(gpu, int8_weights):
    windowed = _make(int8_weights, MAXB, window=32)
    with pytest.raises(RuntimeError, match="sliding window"):
        windowed.serve_begin(prefix_cache=True)
    windowed.serve_begin()  # (refused, not half begun; without the option a window serves)
    windowed.serve_end()
    # the option off: the steps and stats of a decoder that knows no cache
    dec = _make(int8_weights, MAXB)
    prompts = _workload()
    kv0 = _kv(dec)
    for begin in (lambda d: d.serve_begin(), lambda d: d.serve_begin(prefix_cache=False)):
        class Off:
            def __getattr__(self, name):
                return (lambda **kw: begin(dec)) if name == "serve_begin" else getattr(dec, name)
        run = _drive(Off(), prompts, MAX_NEW)
        assert len(run.steps) == _sim_steps([len(p) for p in prompts], MAX_NEW, kv0["pages"])
        plain = llm_capi.serve_plan_sim([len(p) for p in prompts], MAX_NEW, MAX_NEW, max_rows=MAXB,
                                        num_pages=kv0["pages"], pages_per_tile=PPT, page_size=P,
                                        max_seq_len=S)
        need = [-(-(len(p) + m - 1) // P) * PPT for p, m in zip(prompts, MAX_NEW)]
        live, ends = set(), []  # the full needs of the requests live after each step
        for s in range(1, len(run.steps) + 1):
            live |= {r[2] for r in plain if r[0] == s and r[1] == llm_capi.SERVE_ADMIT}
            live -= {r[2] for r in plain if r[0] == s and r[1] == llm_capi.SERVE_RETIRE}
            ends.append(sum(need[i] for i in live))
        assert run.committed == ends
        assert dec.serve_prefix_stats() == ZERO
        kv = _kv(dec)
        assert kv["free"] == kv["pages"] and kv["cow"] == kv0["cow"]
        dec.serve_end()


def test_generate_many_with_the_cache(gpu, int8_weights):
    dec = _make(int8_weights, MAXB)
    prompts = _workload(seed=47)
    run = _drive(dec, prompts, MAX_NEW)
    assert dec.serve_prefix_stats()["positions_hit"] == 16 * 41
    dec.serve_end()
    out = dec.generate_many(prompts, MAX_NEW, prefix_cache=True)
    assert out == [run.ids[i] for i in range(7)]
    assert _kv(dec)["free"] == _kv(dec)["pages"]
