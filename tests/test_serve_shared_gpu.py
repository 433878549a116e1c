"""Shared-prefix attention while serving (llm_decoder_set_shared_attention):
tests/test_serve_prefix_gpu.py's seven-request workload over two headers, with
rows that hit or published the same blocks grouped from one shared page on.

The yardstick is that file's: a cache-less max_batch = 1 decoder per request
fed the served ids (_check_solo), at 2 * LOGIT_TOL for fp16 weights and
FREE_RUN_TOL through int8.  Beside it, the run with sharing on delivers the
events, rows, committed pages and prefix-cache counters of the run with
sharing off, and shared_stats() counts a shared launch on exactly the steps in
which two requests of a header family are live together."""
import pytest

from test_decoder_gpu import FREE_RUN_TOL, LOGIT_TOL
from test_serve_gpu import MAXB, _check_solo, _make, f16_weights, int8_weights  # noqa: F401
from test_serve_prefix_gpu import MAX_NEW, PPT, _drive, _workload

pytestmark = pytest.mark.gpu

FAMILIES = ({0, 1, 2, 6}, {4, 5})  # HA's requests (id 6: two of its blocks) and HB's
CONFIGS = [("f16", "f16_weights", dict(), 2 * LOGIT_TOL),
           ("f16_fp8kv", "f16_weights", dict(kv_dtype="fp8"), 2 * LOGIT_TOL),
           ("int8", "int8_weights", dict(), FREE_RUN_TOL),
           ("int8_fp8kv", "int8_weights", dict(kv_dtype="fp8"), FREE_RUN_TOL)]


@pytest.mark.parametrize("name,weights,cfg,tol", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_shared_serving_parity_and_stats(gpu, request, name, weights, cfg, tol):
    w = request.getfixturevalue(weights)
    prompts = _workload()
    runs, stats, shared = {}, {}, {}
    for on in (False, True):
        dec = _make(w, MAXB, **cfg)
        if on:
            dec.set_shared_attention(1)
        assert dec.shared_attention == int(on)
        runs[on] = _drive(dec, prompts, MAX_NEW)
        stats[on], shared[on] = dec.serve_prefix_stats(), dec.shared_stats()
        dec.serve_end()
    off, run = runs[False], runs[True]
    assert run.steps == off.steps and run.finish == off.finish
    assert run.committed == off.committed and stats[True] == stats[False]
    assert shared[False] == dict(shared_steps=0, grouped_row_steps=0, page_reads_saved=0)
    together = [sum(len(f & {e[0] for e in ev}) >= 2 for f in FAMILIES) for ev in run.steps]
    assert sum(together) > 0, "the workload puts a header's requests in one step"
    s = shared[True]
    assert s["shared_steps"] == sum(t > 0 for t in together)
    assert s["grouped_row_steps"] >= 2 * sum(together)
    assert s["page_reads_saved"] >= PPT * sum(together)
    _check_solo(_make(w, 1, **cfg), prompts, run, tol)


def test_shared_attention_walls(gpu, int8_weights):
    dec = _make(int8_weights, MAXB, window=32)
    with pytest.raises(RuntimeError, match="sliding window"):
        dec.set_shared_attention(1)
    dec = _make(int8_weights, MAXB)
    dec.set_shared_attention()  # "on" without a number: the default length
    assert dec.shared_attention > 1
    with pytest.raises(RuntimeError, match="shared-prefix"):
        dec.set_window(32)
    dec.set_shared_attention(0)
    dec.set_window(32)
