"""Log-probabilities while serving (llm_decoder_submit_logprobs /
llm_decoder_serve_logprobs): the seven-request workload of test_serve_gpu.py on
the INT8 decoder, requests 1, 3 and 6 asking for 0, 3 and 8 top alternatives,
request 3 sampled (temperature 0.8 and a seed).

At every step, for every asking request, the chosen token's value and the top
list are checked against the float64 log-softmax (lse = log(sum exp(x - m) +
1e-6)) of that step's own logits row within KTOL = 1e-5 + 1e-6 |ref|
(test_beam_select_gpu.py's bound), the order against a numpy stable sort by
(logit descending, id ascending); a request that did not ask yields None.  The
extra launch disturbs nothing: all ids equal a run with nobody asking, and the
step graph is re-instantiated exactly when (live rows, anyone asking) changes."""
import numpy as np
import pytest

from test_serve_gpu import (MAX_NEW, MAXB, PROMPT_LENS, V, _make, _prompts,  # noqa: F401
                            int8_weights)

pytestmark = pytest.mark.gpu

ASK = {1: 0, 3: 3, 6: 8}
SAMPLED = {3: dict(temperature=0.8, seed=1234)}


def ktol(ref):
    return 1e-5 + 1e-6 * np.abs(ref)


def _run(dec, prompts, ask, max_new=MAX_NEW, sampled=SAMPLED):
    """Serve the workload; returns (ids per request, per step (live, asking),
    graph instantiations of the run, values checked).  Checks every step's
    log-probabilities."""
    import torch
    buf = torch.empty((MAXB, V), device="cuda")
    inst0 = dec.serve_stats()["graph_instantiations"]
    dec.serve_begin()
    for i, (p, m) in enumerate(zip(prompts, max_new)):
        kw = dict(sampled.get(i, {}))
        if i in ask:
            kw["logprobs"] = ask[i]
        assert dec.submit(p, m, **kw) == i
    ids, shape, checked = {}, [], 0
    while True:
        st = dec.serve_stats()
        if st["live"] + st["waiting"] == 0:
            break
        ev = dec.serve_step(buf.data_ptr())
        lps = dec.serve_logprobs()
        lg = buf.cpu().numpy()
        assert len(lps) == len(ev)
        shape.append((len(ev), any(e[0] in ask for e in ev)))
        for (rid, tok, idx, row, fin), lp in zip(ev, lps):
            ids.setdefault(rid, []).append(tok)
            if rid not in ask:
                assert lp is None, (rid, lp)
                continue
            x = lg[row].astype(np.float64)
            m = x.max()
            lse = np.log(np.exp(x - m).sum() + 1e-6)
            chosen, top = lp
            ref = (x[tok] - m) - lse
            assert abs(chosen - ref) <= ktol(ref), (rid, idx, chosen, ref)
            order = np.lexsort((np.arange(V), -x))[:ask[rid]]
            assert [t for t, _ in top] == list(order), (rid, idx, top, order)
            for t, v in top:
                ref = (x[t] - m) - lse
                assert abs(v - ref) <= ktol(ref), (rid, idx, t, v, ref)
            checked += 1
        assert len(shape) < 500
    inst = dec.serve_stats()["graph_instantiations"] - inst0
    dec.serve_end()
    return ids, shape, inst, checked


def test_serve_logprobs(gpu, int8_weights):
    dec = _make(int8_weights, MAXB)
    prompts = _prompts(PROMPT_LENS, seed=22)
    ids, shape, inst, checked = _run(dec, prompts, ASK)
    assert checked == sum(MAX_NEW[i] for i in ASK)
    assert [len(ids[i]) for i in range(7)] == MAX_NEW
    assert inst == 1 + sum(a != b for a, b in zip(shape, shape[1:]))
    # nobody asking: the same ids, and today's graph count (live-row changes alone)
    ids0, shape0, inst0, checked0 = _run(dec, prompts, {})
    assert ids0 == ids and checked0 == 0
    assert [n for n, _ in shape0] == [n for n, _ in shape] and not any(a for _, a in shape0)
    live = [n for n, _ in shape0]
    assert inst0 == 1 + sum(a != b for a, b in zip(live, live[1:]))
    with pytest.raises(RuntimeError, match="not serving"):
        dec.serve_logprobs()


def test_asking_is_part_of_the_graph_identity(gpu, int8_weights):
    """Two rows.  Request 0 asks and ends after 3 tokens; request 2 (not asking)
    takes its row in the next step: the live-row count stays 2 and only the
    asking changes, which re-instantiates the step graph once."""
    dec = _make(int8_weights, 2)
    prompts = _prompts([5, 17, 9], seed=23)
    max_new = [3, 9, 4]
    ids, shape, inst, checked = _run(dec, prompts, {0: 2}, max_new, {})
    assert checked == 3 and [len(ids[i]) for i in range(3)] == max_new
    assert shape[:4] == [(2, True)] * 3 + [(2, False)]
    changes = 1 + sum(a != b for a, b in zip(shape, shape[1:]))
    live = [n for n, _ in shape]
    assert inst == changes == 2 + sum(a != b for a, b in zip(live, live[1:]))
    ids0, shape0, inst0, _ = _run(dec, prompts, {}, max_new, {})
    assert ids0 == ids and inst0 == inst - 1


def test_submit_logprobs_range_and_generate_many(gpu, int8_weights):
    dec = _make(int8_weights, MAXB)
    prompts = _prompts([3, 16, 17, 1, 64, 9], seed=27)
    dec.serve_begin()
    for bad in (-1, 9):
        with pytest.raises(RuntimeError, match="top_logprobs"):
            dec.submit(prompts[0], 3, logprobs=bad)
    assert dec.serve_stats()["waiting"] == 0
    dec.serve_end()
    plain = dec.generate_many(prompts, 5)
    ids, lps = dec.generate_many(prompts, 5, logprobs=2)
    assert ids == plain
    assert len(lps) == len(prompts)
    for per, toks in zip(lps, ids):
        assert len(per) == len(toks) == 5
        for (chosen, top), tok in zip(per, toks):
            assert len(top) == 2 and top[0][1] >= top[1][1] and chosen <= 0.0
            assert top[0][0] == tok and top[0][1] == chosen  # greedy: the chosen id leads the list
    ids0, lps0 = dec.generate_many(prompts, 5, logprobs=0)
    assert ids0 == plain and all(top == [] for per in lps0 for _, top in per)
    assert dec.generate_many([], 3, logprobs=1) == ([], [])
