"""The continuous-batching scheduler (csrc/serve_plan.hpp) through the tuning
library's serve_plan_sim_tune: the row decisions llm_decoder_serve_step
executes, without a device.

Every request is submitted before step 1 and request i ends after gen_lens[i]
tokens.  Records are (step, kind, id, row, aux): admit (aux = pages committed
after it), token (aux = generated index), move (row = destination, aux =
source row), retire (aux = 1 ended early / 2 max_new reached).
"""
import ctypes
import random

import llm_capi
from llm_capi import SERVE_ADMIT as ADMIT, SERVE_MOVE as MOVE, SERVE_RETIRE as RETIRE, \
    SERVE_TOKEN as TOKEN

AMPLE = dict(num_pages=10 ** 6, pages_per_tile=8, page_size=16, max_seq_len=4096)


def sim(prompt_lens, max_new, gen_lens=None, **geom):
    return llm_capi.serve_plan_sim(prompt_lens, max_new, gen_lens or max_new, **geom)


def by_step(recs, kind):
    out = {}
    for step, k, rid, row, aux in recs:
        if k == kind:
            out.setdefault(step, []).append((rid, row, aux))
    return out


def test_case_a_rows_join_and_leave():
    """max_rows 2, gen_lens 1 / 3 / 2: three steps where lockstep batches of 2
    take max(1, 3) + 2 = 5."""
    recs = sim([4, 4, 4], [3, 3, 3], [1, 3, 2], max_rows=2, **AMPLE)
    tok = {s: [(rid, row) for rid, row, _ in v] for s, v in by_step(recs, TOKEN).items()}
    assert tok == {1: [(0, 0), (1, 1)], 2: [(1, 0), (2, 1)], 3: [(1, 0), (2, 1)]}
    assert {s: [(rid, row) for rid, row, _ in v] for s, v in by_step(recs, ADMIT).items()} == {
        1: [(0, 0), (1, 1)], 2: [(2, 1)]}
    assert by_step(recs, MOVE) == {1: [(1, 0, 1)]}  # id 1: row 1 -> row 0
    ret = by_step(recs, RETIRE)
    assert [(rid, row) for rid, row, _ in ret[1]] == [(0, 0)]
    assert [(rid, row) for rid, row, _ in ret[3]] == [(2, 1), (1, 0)]  # row 1 first, no move
    assert ret[1][0][2] == 1 and [a for _, _, a in ret[3]] == [1, 2]  # early / max_new reached
    assert max(r[0] for r in recs) == 3
    # within a step: admissions, tokens, then retirements with their moves
    order = [k for s, k, *_ in recs if s == 1]
    assert order == [ADMIT, ADMIT, TOKEN, TOKEN, RETIRE, MOVE]


def test_case_b_pool_pressure():
    """Three requests of 24 pages on a pool of 48: the third waits for a
    retirement although two rows are free."""
    recs = sim([25] * 3, [16] * 3, max_rows=4, num_pages=48, pages_per_tile=8, page_size=16,
               max_seq_len=4096)
    adm = by_step(recs, ADMIT)
    assert adm == {1: [(0, 0, 24), (1, 1, 48)], 17: [(2, 0, 24)]}
    assert max(r[0] for r in recs) == 32
    assert max(aux for _, k, _, _, aux in recs if k == ADMIT) <= 48
    assert [len(v) for _, v in sorted(by_step(recs, TOKEN).items())] == [2] * 16 + [1] * 16


def test_window_charges_the_window_bound():
    """window 32, page 16: a row never holds more than ceil(544 / 16) + 1 = 35
    tiles, so T = 1000 (63 tiles) is charged 35; a short request its own tiles."""
    geom = dict(max_rows=2, num_pages=10 ** 6, pages_per_tile=8, page_size=16, window=32,
                max_seq_len=4096)
    assert by_step(sim([901], [100], **geom), ADMIT)[1] == [(0, 0, 35 * 8)]
    assert by_step(sim([901], [100], **dict(geom, window=0)), ADMIT)[1] == [(0, 0, 63 * 8)]
    assert by_step(sim([20], [13], **geom), ADMIT)[1] == [(0, 0, 2 * 8)]
    # ... and fits a pool that the unwindowed need does not
    tight = dict(geom, num_pages=35 * 8)
    assert sim([901], [100], **tight) is not None
    assert sim([901], [100], **dict(tight, window=0)) is None


def test_refusals():
    geom = dict(max_rows=2, num_pages=48, pages_per_tile=8, page_size=16, max_seq_len=64)
    assert sim([33], [32], **geom) is not None       # T = 64 = max_seq_len: 4 tiles, 32 pages
    assert sim([34], [32], **geom) is None           # T = 65 > max_seq_len
    assert sim([8, 34], [4, 32], **geom) is None     # any refused request refuses the run
    big = dict(geom, max_seq_len=4096)
    assert sim([90], [7], **big) is not None         # T = 96: 6 tiles, 48 pages
    assert sim([90], [8], **big) is None             # T = 97: 7 tiles, 56 > 48 pages


def test_room_and_bad_arguments():
    tune = llm_capi.load_tune()
    a = (ctypes.c_int32 * 2)(3, 3)
    args = (a, a, a, 2, 2, 100, 1, 16, 0, 64)
    out = (ctypes.c_longlong * 10)(*([-7] * 10))
    assert tune.serve_plan_sim_tune(*args, out, 2) == -10  # 2 admit + 6 token + 2 retire
    assert list(out) == [1, ADMIT, 0, 0, 1, 1, ADMIT, 1, 1, 2]
    assert tune.serve_plan_sim_tune(*args, None, 0) == -10
    full = (ctypes.c_longlong * 60)()
    assert tune.serve_plan_sim_tune(*args, full, 10) == 10
    bad = -2 ** 31
    assert tune.serve_plan_sim_tune(None, a, a, 2, 2, 100, 1, 16, 0, 64, None, 0) == bad
    assert tune.serve_plan_sim_tune(a, a, a, 2, 0, 100, 1, 16, 0, 64, None, 0) == bad
    z = (ctypes.c_int32 * 2)(3, 4)
    assert tune.serve_plan_sim_tune(a, a, z, 2, 2, 100, 1, 16, 0, 64, None, 0) == bad  # gen > max_new
    assert tune.serve_plan_sim_tune(a, a, a, 0, 2, 100, 1, 16, 0, 64, None, 0) == 0


def test_properties_random():
    rng = random.Random(20252)
    for _ in range(300):
        n = rng.randrange(1, 24)
        max_rows = rng.choice([1, 2, 3, 4, 8])
        ps = rng.choice([1, 4, 16])
        ppt = rng.choice([1, 2, 8])
        window = rng.choice([0, 0, 8, 40])
        prompt = [rng.choice([1, 2, ps, ps + 1, rng.randrange(1, 200)]) for _ in range(n)]
        max_new = [rng.choice([1, 2, rng.randrange(1, 60)]) for _ in range(n)]
        gen = [rng.choice([m, rng.randrange(1, m + 1)]) for m in max_new]
        geom = dict(max_rows=max_rows, pages_per_tile=ppt, page_size=ps, window=window,
                    max_seq_len=400)
        # the largest single need, so every request fits; sometimes room for several
        solo = [by_step(sim([p], [m], num_pages=10 ** 9, **geom), ADMIT)[1][0][2]
                for p, m in zip(prompt, max_new)]
        pool = max(solo) * rng.choice([1, 1, 2, 5])
        recs = sim(prompt, max_new, gen, num_pages=pool, **geom)
        assert recs is not None
        assert [s for s, *_ in recs] == sorted(s for s, *_ in recs)
        assert max(s for s, *_ in recs) <= sum(gen), "the run terminates, a token at least per step"
        admitted = [rid for _, k, rid, _, _ in recs if k == ADMIT]
        assert admitted == list(range(n)), "admissions in id order, every request once"
        got = {i: [] for i in range(n)}
        rows = {}     # row -> id, replayed from the records
        committed = 0
        last_step = 0
        for step, kind, rid, row, aux in recs:
            if step != last_step:
                assert sorted(rows) == list(range(len(rows))), "rows dense after every step"
                last_step = step
                tok_rows = []
            if kind == ADMIT:
                assert row == len(rows) and row < max_rows
                rows[row] = rid
                committed += solo[rid]
                assert aux == committed <= pool
            elif kind == TOKEN:
                assert rows[row] == rid
                tok_rows.append(row)
                assert tok_rows == list(range(len(tok_rows))), "tokens in ascending row order"
                got[rid].append(aux)
            elif kind == RETIRE:
                assert rows.pop(row) == rid
                committed -= solo[rid]
                assert aux == (2 if gen[rid] == max_new[rid] else 1)
            else:
                assert kind == MOVE and row not in rows
                assert aux == max(rows) and rows[aux] == rid, "the last live row moves"
                rows[row] = rows.pop(aux)
        assert not rows and committed == 0
        for i in range(n):
            assert got[i] == list(range(gen[i])), (i, got[i], gen[i])


def test_null_arguments_rejected_before_any_device_call():
    """Every new entry answers a NULL handle (or NULL pointers) with
    LLM_ERR_INVALID on the host."""
    lib = llm_capi.load()
    inv = llm_capi.LLM_ERR_INVALID
    ev = (llm_capi.LlmServeEvent * 4)()
    n, rid = ctypes.c_int(0), ctypes.c_longlong(0)
    opt = llm_capi.LlmRequestOptions(max_new_tokens=1, eos_token=-1, top_p=1.0)
    tok = (ctypes.c_int32 * 1)(0)
    assert lib.llm_decoder_serve_begin(None) == inv
    assert lib.llm_decoder_serve_end(None) == inv
    assert lib.llm_decoder_submit(None, tok, 1, ctypes.byref(opt), ctypes.byref(rid)) == inv
    assert lib.llm_decoder_cancel(None, 0) == inv
    assert lib.llm_decoder_serve_step(None, None, ev, 4, ctypes.byref(n)) == inv
    assert lib.llm_decoder_serve_stats(None, None, None, None, None) == inv
    assert b"llm_decoder_serve_stats" in lib.llm_last_error()
    assert lib.sample_rows_each(None, 1, 10, None, None, None, None, None, None, None) == inv
    one = ctypes.c_void_p(16)
    assert lib.sample_rows_each(one, 1, 65537, None, None, None, None, None, one, None) == inv
    assert lib.sample_rows_each(one, -1, 10, None, None, None, None, None, one, None) == inv
    assert lib.sample_rows_each(None, 0, 10, None, None, None, None, None, None, None) == 0
