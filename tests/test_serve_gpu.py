"""Continuous batching (llm_decoder_serve_*): rows join and leave a running
batch, per-request sampling, cancel, the mode walls and generate_many.

Small models (L 2 / H 4 / D 64, V 300, max_seq 640, max_batch 4): the fp16
CUDADecoder and the synthetic INT8 model, the latter also with LLM_FP8 pages,
with rope + a 32-token window, and with packed prefill.  The workload is seven
requests whose prompts sit on and around page boundaries, one of them a
two-chunk prefill (530 tokens) admitted while other rows decode; ids 1 and 6
end in the same step.

The yardstick is a max_batch = 1 decoder per request: prefill prompt[:-1],
step the prompt's last token, then the served ids -- its logits at every
generated index against the served row's.  The bars are the project's between
two paths of one decoder: 2 * LOGIT_TOL for fp16 weights
(test_prefill_decode_kernel_fallback), FREE_RUN_TOL through int8 activations.
"""
import ctypes

import numpy as np
import pytest

import llm_capi
from _util import record, rel_err
from test_decoder_gpu import FREE_RUN_TOL, LOGIT_TOL, TIE_TOL, _f16_model, _int8_model

pytestmark = pytest.mark.gpu

L, H, D, V, S, MAXB = 2, 4, 64, 300, 640, 4
PROMPT_LENS = [1, 17, 33, 40, 16, 5, 530]
MAX_NEW = [3, 12, 5, 20, 3, 9, 6]


def _torch():
    import torch
    return torch


def _prompts(lens, seed=21):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, V, n).tolist() for n in lens]


@pytest.fixture(scope="module")
def f16_weights():
    return _f16_model(np.random.default_rng(8), L, H, D, V, S)


@pytest.fixture(scope="module")
def int8_weights(oracle):
    return _int8_model(oracle, L=L, H=H, D=D, V=V, S=S, seed=31)


def _make(w, max_batch, *, kv_dtype="float16", rope=False, window=0, packed=False, num_pages=0):
    import llm_decoder
    f16 = w["wqkv"].dtype == np.float16
    cls = llm_decoder.CUDADecoder if f16 else llm_decoder.INT8Decoder
    dec = cls(L, H, D, H * D, V, S, max_batch=max_batch, num_pages=num_pages, kv_dtype=kv_dtype)
    d = {k: np.ascontiguousarray(v) for k, v in w.items() if k != "cfg"}
    for k in ("emb",) + (("wqkv", "wo", "w1", "w2") if f16 else ()):
        d[k] = d[k].view(np.uint16)
    dec.set_weights(d)
    if rope:
        dec.set_rope(theta=10000.0)
    if window:
        dec.set_window(window)
    dec.packed_prefill = packed
    return dec


def _kv(dec):
    lib, h = llm_capi.load(), ctypes.c_void_p(dec.kv_handle)
    return dict(free=lib.kv_cache_free_pages(h), pages=lib.kv_cache_num_pages(h),
                cow=lib.kv_cache_cow_copies(h))


class Run:
    def __init__(self):
        self.ids, self.logits, self.finish, self.steps, self.live_counts = {}, {}, {}, [], []


def _serve(dec, prompts, max_new, opts=None, between=None):
    """Submit everything, step until nothing is live or waiting.  between(step,
    dec): called before each step (cancellations).  Returns a Run: per id the
    tokens, the step's logits row of every token and the finish reason; per
    step the events."""
    torch = _torch()
    buf = torch.empty((MAXB, V), device="cuda")
    run = Run()
    dec.serve_begin()
    for i, (p, m) in enumerate(zip(prompts, max_new)):
        assert dec.submit(p, m, **(opts[i] if opts else {})) == i
    step = 0
    while True:
        step += 1
        if between:
            between(step, dec)
        st = dec.serve_stats()
        if st["live"] + st["waiting"] == 0:
            break
        ev = dec.serve_step(buf.data_ptr())
        assert 1 <= len(ev) <= MAXB
        lg = buf.cpu().numpy()
        assert [e[3] for e in ev] == list(range(len(ev))), "events in ascending row order"
        for rid, tok, idx, row, fin in ev:
            assert idx == len(run.ids.setdefault(rid, [])), "indices count from 0"
            assert rid not in run.finish, "nothing after a request's last event"
            run.ids[rid].append(tok)
            run.logits.setdefault(rid, []).append(lg[row].copy())
            if fin:
                run.finish[rid] = fin
        run.steps.append(ev)
        run.live_counts.append(len(ev))
        assert dec.serve_stats()["live"] <= MAXB
        assert step < 500
    return run


def _solo_logits(solo, prompt, ids):
    """The logits a one-row decoder gives at every generated index when fed the
    prompt and then `ids`."""
    torch = _torch()
    solo.begin_synthetic(1, 0, 0, False)
    if len(prompt) > 1:
        solo.prefill(0, prompt[:-1])
    lg = torch.empty((1, V), device="cuda")
    out, feed = [], prompt[-1]
    for t in ids:
        solo.step([feed], logits_ptr=lg.data_ptr())
        torch.cuda.synchronize()
        out.append(lg[0].cpu().numpy().copy())
        feed = t
    return out


def _check_solo(solo, prompts, run, tol, only=None, greedy=True):
    worst = 0.0
    for rid in (run.ids if only is None else only):
        ref = _solo_logits(solo, prompts[rid], run.ids[rid])
        for i, (a, b) in enumerate(zip(run.logits[rid], ref)):
            err = rel_err(a, b)
            worst = max(worst, err)
            assert err < tol, (rid, i, err)
            if greedy:
                assert run.ids[rid][i] == int(np.argmax(a)), (rid, i)
    return worst


def _sim_steps(prompt_lens, max_new, num_pages, window=0):
    recs = llm_capi.serve_plan_sim(prompt_lens, max_new, max_new, max_rows=MAXB,
                                   num_pages=num_pages, pages_per_tile=L * H, page_size=16,
                                   window=window, max_seq_len=S)
    return max(r[0] for r in recs)


@pytest.fixture(scope="module")
def f16_run(gpu, f16_weights):
    """The workload on the fp16 decoder: (decoder, prompts, Run, kv counters and
    stats around the run)."""
    dec = _make(f16_weights, MAXB)
    prompts = _prompts(PROMPT_LENS)
    kv0, inst0 = _kv(dec), dec.serve_stats()["graph_instantiations"]
    run = _serve(dec, prompts, MAX_NEW)
    after = dict(_kv(dec), inst=dec.serve_stats()["graph_instantiations"] - inst0)
    dec.serve_end()
    return dec, prompts, run, kv0, after, _kv(dec)


def test_bookkeeping(f16_run):
    dec, prompts, run, kv0, after, ended = f16_run
    for i, m in enumerate(MAX_NEW):
        assert len(run.ids[i]) == m and run.finish[i] == llm_capi.LLM_FINISH_LENGTH
    assert len(run.steps) == _sim_steps(PROMPT_LENS, MAX_NEW, kv0["pages"])
    assert len(run.steps) < sum(max(MAX_NEW[i:i + MAXB]) for i in range(0, 7, MAXB))  # lockstep
    last = [[e[0] for e in ev if e[4]] for ev in run.steps]
    assert any(len(x) == 2 for x in last), "two rows finish in one step"
    assert after["cow"] == kv0["cow"], "a row move copied a page"
    assert after["free"] == after["pages"] == kv0["pages"], "pages back after the last retirement"
    assert ended["free"] == ended["pages"]
    changes = 1 + sum(a != b for a, b in zip(run.live_counts, run.live_counts[1:]))
    assert after["inst"] == changes, "one step graph: re-instantiated when the row count changes"
    st = dec.serve_stats()
    assert (st["live"], st["waiting"], st["committed_pages"]) == (0, 0, 0)


def test_parity_solo_f16(f16_run, f16_weights):
    dec, prompts, run, *_ = f16_run
    worst = _check_solo(_make(f16_weights, 1), prompts, run, 2 * LOGIT_TOL)
    record("serve", test="solo_f16", logit_err=worst, steps=len(run.steps))


def test_parity_oracle_f16(f16_run, f16_weights, oracle):
    """The restated CUDADecoder stepped over prompt + ids holds every served
    logits row to LOGIT_TOL, and every served id within LOGIT_TOL * scale of
    its top logit."""
    from oracle.oracle import OracleDecoder
    dec, prompts, run, *_ = f16_run
    for rid, p in enumerate(prompts):
        od = OracleDecoder(oracle, f16_weights, 1)
        seq = p + run.ids[rid][:-1]
        for i, t in enumerate(seq):
            _, ol, _ = od.step(np.array([t], np.int32), np.array([i], np.int32))
            g = i - (len(p) - 1)
            if g < 0:
                continue
            err = rel_err(run.logits[rid][g], ol[0])
            assert err < LOGIT_TOL, (rid, g, err)
            gap = ol[0].max() - ol[0][run.ids[rid][g]]
            assert gap <= LOGIT_TOL * np.abs(ol[0]).max(), (rid, g, gap)


@pytest.mark.parametrize("cfg", [dict(), dict(kv_dtype="fp8"), dict(rope=True, window=32),
                                 dict(packed=True)],
                         ids=["int8", "int8_fp8kv", "int8_rope_window32", "int8_packed_prefill"])
def test_parity_solo_int8(gpu, int8_weights, cfg):
    dec = _make(int8_weights, MAXB, **cfg)
    prompts = _prompts(PROMPT_LENS, seed=22)
    kv0 = _kv(dec)
    run = _serve(dec, prompts, MAX_NEW)
    assert [len(run.ids[i]) for i in range(7)] == MAX_NEW
    assert len(run.steps) == _sim_steps(PROMPT_LENS, MAX_NEW, kv0["pages"], cfg.get("window", 0))
    kv1 = _kv(dec)
    assert kv1["cow"] == kv0["cow"] and kv1["free"] == kv1["pages"]
    dec.serve_end()
    solo_cfg = {k: v for k, v in cfg.items() if k != "packed"}
    worst = _check_solo(_make(int8_weights, 1, **solo_cfg), prompts, run, FREE_RUN_TOL)
    record("serve", test="solo_int8", cfg=cfg, logit_err=worst, steps=len(run.steps))


def test_pool_pressure(gpu, int8_weights):
    """A pool that holds two of four equal requests (T = 32: 2 tiles of L * H =
    8 pages each): all four complete, two at a time, no LLM_ERR_OOM."""
    dec = _make(int8_weights, MAXB, num_pages=32)
    prompts = _prompts([20] * 4, seed=23)
    run = _serve(dec, prompts, [13] * 4)
    assert [len(run.ids[i]) for i in range(4)] == [13] * 4
    assert max(run.live_counts) == 2 and len(run.steps) == 26
    assert _kv(dec)["free"] == 32
    dec.serve_end()
    _check_solo(_make(int8_weights, 1), prompts, run, FREE_RUN_TOL)


def test_eos(f16_run):
    """Request 3's token at index 2 as its eos_token: it ends with
    LLM_FINISH_EOS where that token first appears, the token delivered; its
    earlier ids are the first run's (same batch up to that step, deterministic
    kernels)."""
    dec, prompts, first, *_ = f16_run
    eos = first.ids[3][2]
    at = first.ids[3].index(eos)
    opts = [dict(eos_token_id=eos) if i == 3 else {} for i in range(7)]
    run = _serve(dec, prompts, MAX_NEW, opts)
    dec.serve_end()
    assert run.finish[3] == llm_capi.LLM_FINISH_EOS
    assert run.ids[3] == first.ids[3][:at + 1]
    for i in (0, 1, 2, 4, 5, 6):
        assert len(run.ids[i]) == MAX_NEW[i] and run.finish[i] == llm_capi.LLM_FINISH_LENGTH
    assert _kv(dec)["free"] == _kv(dec)["pages"]


def test_sampling_while_serving(gpu, int8_weights):
    """Greedy and sampled requests of different settings share the steps: two
    runs agree, and every token is the oracle sampler's on that step's logits
    row with the request's settings, its seed and counter = its position."""
    from oracle.oracle import sample_rows
    dec = _make(int8_weights, MAXB)
    lens, max_new = [1, 17, 33, 40, 16, 5], [4, 9, 6, 12, 5, 7]
    prompts = _prompts(lens, seed=24)
    opts = [dict(), dict(temperature=0.8, top_k=40, top_p=0.9, seed=77),
            dict(temperature=1.2, seed=2 ** 63 + 9), dict(temperature=1.0, top_k=1, seed=5),
            dict(temperature=0.9, top_p=0.6, seed=1), dict(temperature=0.7, top_k=8, seed=77)]
    a = _serve(dec, prompts, max_new, opts)
    dec.serve_end()
    b = _serve(dec, prompts, max_new, opts)
    dec.serve_end()
    assert a.ids == b.ids
    for rid, o in enumerate(opts):
        for i, (tok, row) in enumerate(zip(a.ids[rid], a.logits[rid])):
            ref, margin, near = sample_rows(row[None], o.get("temperature", 0.0), o.get("top_k", 0),
                                            o.get("top_p", 1.0), seed=o.get("seed", 0),
                                            counter=lens[rid] - 1 + i, neighbours=True)
            assert tok == ref[0] or (margin[0] < 1e-4 and tok in near[0]), (rid, i, tok, ref[0])
    assert any(a.ids[r][i] != int(np.argmax(a.logits[r][i]))
               for r in (1, 2, 4, 5) for i in range(len(a.ids[r]))), "nothing was sampled"


def test_cancel(gpu, int8_weights):
    """One waiting request (id 5, before step 2) and one live one (id 1,
    before step 3) are cancelled: no further event, their pages return, an
    unknown id is refused, and the others keep the solo parity."""
    dec = _make(int8_weights, MAXB)
    prompts = _prompts(PROMPT_LENS, seed=25)

    def between(step, d):
        if step == 2:
            d.cancel(5)
        if step == 3:
            d.cancel(1)
            with pytest.raises(RuntimeError, match="no waiting or live request"):
                d.cancel(1)
            with pytest.raises(RuntimeError, match="no waiting or live request"):
                d.cancel(99)

    run = _serve(dec, prompts, MAX_NEW, between=between)
    assert 5 not in run.ids and len(run.ids[1]) == 2 and 1 not in run.finish
    keep = [0, 2, 3, 4, 6]
    assert [len(run.ids[i]) for i in keep] == [MAX_NEW[i] for i in keep]
    kv = _kv(dec)
    assert kv["free"] == kv["pages"] and kv["cow"] == 0
    dec.serve_end()
    _check_solo(_make(int8_weights, 1), prompts, run, FREE_RUN_TOL, only=keep)


def test_mode_walls(gpu, int8_weights):
    dec = _make(int8_weights, MAXB)
    prompt = _prompts([9], seed=26)[0]
    before = dec.generate(prompt, 6)
    with pytest.raises(RuntimeError, match="not serving"):
        dec.submit(prompt, 3)
    with pytest.raises(RuntimeError, match="not serving"):
        dec.serve_step()
    dec.serve_begin()
    rid = dec.submit(prompt, 3)
    for bad in (dict(max_new_tokens=0), dict(max_new_tokens=S), dict(eos_token_id=V),
                dict(top_p=0.0), dict(top_k=-1)):
        with pytest.raises(RuntimeError):
            dec.submit(prompt, **dict(dict(max_new_tokens=3), **bad))
    with pytest.raises(RuntimeError, match="out of range"):
        dec.submit([V], 3)
    assert dec.serve_stats()["waiting"] == 1
    assert len(dec.serve_step()) == 1
    for call in (lambda: dec.generate(prompt, 6), lambda: dec.step([1]), lambda: dec.set_window(8),
                 lambda: dec.serve_begin(), lambda: dec.prefill(0, [1, 2]),
                 lambda: dec.set_sampling(0.5), lambda: dec.begin_synthetic(1, 0, 0, False)):
        with pytest.raises(RuntimeError, match="serving"):
            call()
    assert [e[0] for e in dec.serve_step()] == [rid]  # the walls disturbed nothing
    dec.serve_end()
    assert dec.context_len(0) == -1  # no rows stay active
    assert dec.generate(prompt, 6) == before
    dec.serve_begin()
    assert dec.serve_step() == []  # nothing live, nothing admissible: no launch
    dec.serve_end()


def test_generate_many(gpu, int8_weights):
    dec = _make(int8_weights, MAXB)
    lens = [3, 16, 17, 1, 64, 9, 31, 48, 5]
    max_new = [4, 7, 2, 9, 5, 3, 8, 6, 1]
    prompts = _prompts(lens, seed=27)
    out = dec.generate_many(prompts, max_new)
    assert [len(x) for x in out] == max_new
    assert [len(x) for x in dec.generate_many(prompts[:2], 5)] == [5, 5]  # scalar max_new_tokens
    assert dec.generate_many([], 3) == []
    # the generated ids fed to the solo decoder: each is that decoder's argmax
    # (greedy requests), or within TIE_TOL of its top logit on a near-tie
    solo = _make(int8_weights, 1)
    for rid, (p, ids) in enumerate(zip(prompts, out)):
        ref = _solo_logits(solo, p, ids)
        for i, t in enumerate(ids):
            gap = (ref[i].max() - ref[i][t]) / np.abs(ref[i]).max()
            assert t == int(np.argmax(ref[i])) or gap <= TIE_TOL, (rid, i, t, gap)
    # sampled: prompt i draws with seed + i, so equal prompts differ and a rerun agrees
    same = [prompts[4]] * 3
    s1 = dec.generate_many(same, 12, temperature=1.0, seed=100)
    assert s1 == dec.generate_many(same, 12, temperature=1.0, seed=100)
    assert s1[0] != s1[1] or s1[1] != s1[2]
