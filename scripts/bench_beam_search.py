#!/usr/bin/env python3
"""What beam search costs over the bare C4 step (profiles/beam_search_c4.json).

C4 model dims (bench.py CONFIGS["c4"]) with synthetic weights: 8 prompts x 4
beams, prompt 3840, 256 new tokens, through llm_decoder_beam_search.  Measured,
after a warm-up search, in alternating blocks (search, plain begin_beams steps
of the same decoder), median and spread over the blocks:

  * tokens/s of the whole search (prefill included) and of its decode steps
    (the search minus a 1-token search: the same prefill);
  * per-step time against the plain begin_beams step (8 x 4 rows, 3840 shared
    + 128 private tokens: the search's mean context), same process;
  * device-event time of the two selection launches (beam_select_rows);
  * host time of kv_cache_reorder (8 sequences) and of the step call that
    follows it (prepare_append + the batched copy-on-write + table sync +
    graph launch; it returns before the device finishes);
  * copy-on-write pages per step.

--bar: the INT8 yardstick of tests/test_beam_search_gpu.py -- one 77-token
sequence teacher-forced through the tests' synthetic INT8Decoder at batch 1
and in a batch of 4 rows; prints the worst logit rel_err between the two.
--tree DIR runs against the build of another checkout (the parent commit).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
PKG_NAME = "pagedattention-based-transformer-decoder-inference-framework_amd"


def med_spread(xs):
    xs = sorted(xs)
    return dict(median=statistics.median(xs), min=xs[0], max=xs[-1], n=len(xs))


def bar(args):
    import torch
    import llm_decoder
    from oracle.oracle import Oracle, synthetic_int8_model
    L, H, D, V, S, n_tok = 2, 4, 64, 500, 128, 77
    w = synthetic_int8_model(Oracle(), L=L, H=H, D=D, V=V, max_seq=S, seed=21)
    wd = {k: np.ascontiguousarray(v) for k, v in w.items() if k != "cfg"}
    wd["emb"] = w["emb"].view(np.uint16)
    seq = [int(t) for t in np.random.default_rng(5).integers(0, V, n_tok)]
    out = {}
    for rows in (1, 4):
        dec = llm_decoder.INT8Decoder(L, H, D, H * D, V, S, max_batch=rows)
        dec.set_weights(wd)
        dec.begin_synthetic(rows, 0, 0, False)
        lg = torch.empty((rows, V), dtype=torch.float32, device="cuda")
        got = np.zeros((n_tok, rows, V), np.float32)
        for i, t in enumerate(seq):
            dec.step([t] * rows, logits_ptr=lg.data_ptr())
            torch.cuda.synchronize()
            got[i] = lg.cpu().numpy()
        out[rows] = got
    worst = 0.0
    for i in range(n_tok):
        ref = out[1][i, 0].astype(np.float64)
        for r in range(4):
            e = np.max(np.abs(out[4][i, r] - ref)) / np.max(np.abs(ref))
            worst = max(worst, float(e))
    res = dict(what="INT8Decoder, 77 teacher-forced tokens: worst logit rel_err, batch 1 vs batch 4",
               int8_bar=worst, tree=str(args.tree or ROOT))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--bar", action="store_true")
    ap.add_argument("--tree", default=None, help="root of another checkout whose build to use")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "beam_search_c4.json"))
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--prompt", type=int, default=3840)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--plain-steps", type=int, default=64)
    ap.add_argument("--int8-bar", type=float, default=None,
                    help="record a --bar figure measured elsewhere in the output file")
    args = ap.parse_args()
    tree = Path(args.tree).resolve() if args.tree else ROOT
    sys.path.insert(0, str(tree / PKG_NAME))
    sys.path.insert(0, str(tree))
    if args.bar:
        bar(args)
        return
    import ctypes

    import torch
    import llm_capi
    import llm_decoder
    import bench
    cfg = bench.CONFIGS["c4"]
    S, W, P, NEW = args.seqs, args.beams, args.prompt, args.new
    rows, V = S * W, cfg["V"]
    lib = llm_capi.load()
    dec = getattr(llm_decoder, cfg["cls"])(cfg["L"], cfg["H"], cfg["D"], cfg["H"] * cfg["D"], V,
                                           P + NEW + 16, max_batch=rows, page_size=cfg["ts"])
    dec.set_weights(bench.make_weights(cfg, 0))
    kvh = ctypes.c_void_p(dec.kv_handle)
    rng = np.random.default_rng(0)
    prompts = [[int(t) for t in rng.integers(0, V, P)] for _ in range(S)]

    def search(new):
        t0 = time.perf_counter()
        res, tr = dec.beam_search_batch(prompts, beam_width=W, max_new_tokens=new,
                                        return_trace=True)
        return time.perf_counter() - t0, tr

    def plain_steps(n):
        dec.begin_beams(S, W, P, NEW // 2, 0, True)
        tok = [int(t) for t in rng.integers(0, V, rows)]
        for _ in range(4):
            dec.step(tok, want_next=False)
        dec.sync()
        calls = []
        t0 = time.perf_counter()
        for _ in range(n):
            c0 = time.perf_counter()
            dec.step(None, want_next=False)
            calls.append(time.perf_counter() - c0)
        dec.sync()
        return (time.perf_counter() - t0) / n, statistics.median(calls)

    search(8)  # warm-up: graphs captured, prefill buffers allocated
    plain_steps(8)
    t_full, t_one, t_plain, plain_call, cow = [], [], [], [], []
    parents_seen = []
    for _ in range(args.blocks):
        c0 = lib.kv_cache_cow_copies(kvh)
        t, tr = search(NEW)
        cow.append((lib.kv_cache_cow_copies(kvh) - c0) / tr["steps"])
        t_full.append(t)
        parents_seen = tr["live_parent"]
        t_one.append(search(1)[0])
        p, c = plain_steps(args.plain_steps)
        t_plain.append(p)
        plain_call.append(c)
    step_beam = [(a - b) / (NEW - 1) for a, b in zip(t_full, t_one)]

    # the selection launches alone, by device events
    lg = torch.randn((rows, V), device="cuda")
    sc = torch.zeros(rows, device="cuda")
    for _ in range(5):
        llm_capi.beam_select(lg, sc, W)
    sel = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            llm_capi.beam_select(lg, sc, W)
        e1.record()
        e1.synchronize()
        sel.append(e0.elapsed_time(e1) / 10 * 1e3)

    # host side of one step after a search: reorder (the parents of the search's
    # last steps) and the step call that appends into the shared tail pages
    search(NEW // 2)
    reorder_us, call_us = [], []
    tok = [int(t) for t in rng.integers(0, V, rows)]
    for i in range(32):
        par = parents_seen[-1 - (i % 32)]
        ctx = dec.context_len(0)
        t0 = time.perf_counter()
        for s in range(S):
            llm_capi.kv_cache_reorder(dec.kv_handle, s * W, [int(x) for x in par[s]], ctx)
        reorder_us.append((time.perf_counter() - t0) * 1e6)
        t0 = time.perf_counter()
        dec.step(tok, want_next=False)
        call_us.append((time.perf_counter() - t0) * 1e6)
        dec.sync()

    new_tokens = S * NEW  # tokens of the best hypothesis of every prompt
    res = dict(
        config="C4 dims, synthetic weights: %d prompts x %d beams, prompt %d, %d new tokens"
               % (S, W, P, NEW),
        search_s=med_spread(t_full),
        search_tokens_per_s=new_tokens / statistics.median(t_full),
        search_beam_tokens_per_s=rows * NEW / statistics.median(t_full),
        prefill_plus_one_step_s=med_spread(t_one),
        beam_step_ms=med_spread([x * 1e3 for x in step_beam]),
        plain_step_ms=med_spread([x * 1e3 for x in t_plain]),
        beam_step_over_plain=statistics.median(step_beam) / statistics.median(t_plain),
        decode_beam_tokens_per_s=rows / statistics.median(step_beam),
        plain_beam_tokens_per_s=rows / statistics.median(t_plain),
        select_launches_us=med_spread(sel),
        reorder_host_us=med_spread(reorder_us),
        step_call_host_us_after_reorder=med_spread(call_us),
        step_call_host_us_plain=med_spread([x * 1e6 for x in plain_call]),
        cow_pages_per_step=med_spread(cow),
    )
    if args.int8_bar is not None:
        res["int8_bar"] = dict(value=args.int8_bar, factor=2.0,
                               what="worst logit rel_err, one 77-token sequence at batch 1 vs "
                                    "in a batch of 4 (--bar on the parent commit); "
                                    "tests/test_beam_search_gpu.py allows factor x value")
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
