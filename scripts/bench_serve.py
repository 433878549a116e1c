#!/usr/bin/env python3
"""Continuous batching against lockstep batches, one process, C3 dims.

    python scripts/bench_serve.py [--out profiles/serve.json] [--reps 3]
    rocprofv3 --kernel-trace --stats ... -- python scripts/bench_serve.py --trace-serve

Arm "skewed": 128 requests, seeded prompt lengths in 128..1024 and max_new in
16..256.  `generate_many` (the serve loop: rows retire and are refilled)
against the unchanged `generate_batch` run in submission-order batches of 64,
each to its longest max_new.  Arm "equal": 64 requests x 128-token prompts x 64
new tokens, where the two should tie; the difference is reported next to the
same-arm run-to-run spread.

Both sides are warmed up, every timed window is synchronised on both ends, and
the sides alternate for --reps repetitions.  Generated tokens/s counts the
tokens the requests asked for (lockstep also computes, and discards, the rows
that run past their max_new).  The decode-step count of the serve side is the
scheduler simulation's (serve_plan_sim_tune: the steps llm_decoder_serve_step
runs, tests/test_serve_gpu.py); the time in admission prefill is an estimate
from a separate, untimed pass through the Python serve loop: the time of the
steps that admit, less the median step that does not, per admitting step.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pagedattention-based-transformer-decoder-inference-framework_amd"))
sys.path.insert(0, str(ROOT))

C3 = dict(L=24, H=16, D=128, V=50257, ts=16, cls="INT8Decoder")
MAXB = 64


def timed(dec, fn):
    dec.sync()
    t0 = time.perf_counter()
    out = fn()
    dec.sync()
    return time.perf_counter() - t0, out


def lockstep(dec, prompts, max_new):
    out = []
    for i in range(0, len(prompts), MAXB):
        g = max(max_new[i:i + MAXB])
        res = dec.generate_batch(prompts[i:i + MAXB], g)
        out += [r[len(p):len(p) + m] for r, p, m in zip(res, prompts[i:i + MAXB],
                                                         max_new[i:i + MAXB])]
    return out


def serve_loop_profile(dec, prompts, max_new):
    """(steps, seconds in steps that admit, seconds in the others, admitting
    steps) through the Python serve loop."""
    dec.serve_begin()
    for p, m in zip(prompts, max_new):
        dec.submit(p, m)
    adm, plain = [], []
    while True:
        st = dec.serve_stats()
        if st["live"] + st["waiting"] == 0:
            break
        dec.sync()
        t0 = time.perf_counter()
        dec.serve_step()
        dt = time.perf_counter() - t0
        admitted = st["waiting"] - dec.serve_stats()["waiting"]
        (adm if admitted else plain).append(dt)
    dec.serve_end()
    return len(adm) + len(plain), adm, plain


def arm(dec, cfg, name, prompts, max_new, reps, max_seq):
    import llm_capi
    want = sum(max_new)
    sides = {"serve": lambda: dec.generate_many(prompts, max_new),
             "lockstep": lambda: lockstep(dec, prompts, max_new)}
    for fn in sides.values():  # warm: graphs of every row count, prefill buffers
        fn()
    secs = {k: [] for k in sides}
    ids = {}
    for _ in range(reps):
        for k, fn in sides.items():
            dt, ids[k] = timed(dec, fn)
            secs[k].append(dt)
    assert [len(x) for x in ids["serve"]] == max_new
    assert [len(x) for x in ids["lockstep"]] == max_new
    pages = llm_capi.load().kv_cache_num_pages(dec.kv_handle)
    recs = llm_capi.serve_plan_sim([len(p) for p in prompts], max_new, max_new, max_rows=MAXB,
                                   num_pages=pages, pages_per_tile=cfg["L"] * cfg["H"],
                                   page_size=cfg["ts"], max_seq_len=max_seq)
    nsteps, adm, plain = serve_loop_profile(dec, prompts, max_new)
    assert nsteps == max(r[0] for r in recs)
    base = statistics.median(plain) if plain else 0.0
    res = {"requests": len(prompts), "generated_tokens": want,
           "prompt_tokens": sum(len(p) for p in prompts),
           "decode_steps": {"serve": nsteps,
                            "lockstep": sum(max(max_new[i:i + MAXB])
                                            for i in range(0, len(prompts), MAXB))},
           "admission_prefill_s_estimate": round(sum(t - base for t in adm), 4),
           "admitting_steps": len(adm),
           "median_plain_step_ms": round(base * 1e3, 3),
           "same_ids_fraction": round(float(np.mean([a == b for a, b in zip(ids["serve"],
                                                                          ids["lockstep"])])), 3)}
    for k, v in secs.items():
        med = statistics.median(v)
        res[k] = {"seconds": [round(t, 4) for t in v], "median_s": round(med, 4),
                  "spread_s": round(max(v) - min(v), 4),
                  "generated_tokens_per_s": round(want / med, 1)}
    res["serve_vs_lockstep"] = round(res["lockstep"]["median_s"] / res["serve"]["median_s"], 3)
    diff = res["serve"]["median_s"] - res["lockstep"]["median_s"]
    res["serve_minus_lockstep_s"] = round(diff, 4)
    res["difference_exceeds_spread"] = bool(
        abs(diff) > max(res["serve"]["spread_s"], res["lockstep"]["spread_s"]))
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "serve.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=C3["L"])
    ap.add_argument("--row-by-row-prefill", action="store_true",
                    help="prefill each prompt on its own (default: packed passes, both sides)")
    ap.add_argument("--trace-serve", action="store_true",
                    help="run only the serve side of the equal arm, 1 + reps times (for a "
                         "kernel trace taken in a run of its own)")
    args = ap.parse_args()
    import llm_decoder
    from bench import make_weights
    cfg = dict(C3, L=args.layers)
    max_seq = 1024 + 256
    dec = llm_decoder.INT8Decoder(cfg["L"], cfg["H"], cfg["D"], cfg["H"] * cfg["D"], cfg["V"],
                                  max_seq, max_batch=MAXB, page_size=cfg["ts"])
    dec.set_weights(make_weights(cfg, 1234))
    dec.packed_prefill = not args.row_by_row_prefill
    rng = np.random.default_rng(7)
    if args.trace_serve:  # under a profiler: the equal arm's serve side only, no timing
        equal = [rng.integers(0, cfg["V"], 128).tolist() for _ in range(MAXB)]
        for _ in range(1 + args.reps):
            dec.generate_many(equal, 64)
        dec.sync()
        return
    lens = rng.integers(128, 1025, 128).tolist()
    max_new = rng.integers(16, 257, 128).tolist()
    skew = [rng.integers(0, cfg["V"], n).tolist() for n in lens]
    equal = [rng.integers(0, cfg["V"], 128).tolist() for _ in range(MAXB)]
    res = {"config": {"dims": cfg, "max_batch": MAXB, "max_seq_len": max_seq,
                      "packed_prefill": dec.packed_prefill, "reps": args.reps,
                      "timing": "wall clock, device synchronised around every window; sides "
                                "alternate"},
           "skewed": arm(dec, cfg, "skewed", skew, max_new, args.reps, max_seq),
           "equal": arm(dec, cfg, "equal", equal, [64] * MAXB, args.reps, max_seq)}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
