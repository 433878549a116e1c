#!/usr/bin/env python3
"""Serving with the prefix cache against serving without it, one process, C3 dims.

    python scripts/bench_serve_prefix.py [--out profiles/serve_prefix.json] [--reps 3]

Arm "shared": 128 requests whose prompts are one 1024-token header plus a
unique tail of 64..256 tokens, 16..128 new tokens each.  Arm "skewed":
scripts/bench_serve.py's skewed workload (seeded prompt lengths in 128..1024,
max_new in 16..256), which shares no prefix: what the cache costs when it never
hits.

Both sides are `generate_many` on one decoder (max_batch 64, packed prefill),
with prefix_cache on and off.  Both are warmed up, every timed window is
synchronised on both ends, and the sides alternate for --reps repetitions; the
yardstick is the cache-off side of the same run.  Decode steps, prompt
positions prefilled and positions hit are the scheduler simulation's
(serve_prefix_sim_tune: the decisions llm_decoder_serve_step executes,
tests/test_serve_prefix_gpu.py).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pagedattention-based-transformer-decoder-inference-framework_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from bench_serve import C3, MAXB, timed  # noqa: E402


def arm(dec, cfg, name, prompts, max_new, reps, max_seq):
    import llm_capi
    want = sum(max_new)
    sides = {"cache_on": lambda: dec.generate_many(prompts, max_new, prefix_cache=True),
             "cache_off": lambda: dec.generate_many(prompts, max_new)}
    for fn in sides.values():  # warm: graphs of every row count, prefill buffers
        fn()
    secs = {k: [] for k in sides}
    ids = {}
    for _ in range(reps):
        for k, fn in sides.items():
            dt, ids[k] = timed(dec, fn)
            secs[k].append(dt)
    for k in sides:
        assert [len(x) for x in ids[k]] == max_new
    pages = llm_capi.load().kv_cache_num_pages(dec.kv_handle)
    res = {"requests": len(prompts), "generated_tokens": want,
           "prompt_tokens": sum(len(p) for p in prompts),
           "same_ids_fraction": round(float(np.mean([a == b for a, b in zip(
               ids["cache_on"], ids["cache_off"])])), 3)}
    for k, v in secs.items():
        recs, st = llm_capi.serve_prefix_sim(prompts, max_new, max_new, max_rows=MAXB,
                                             num_pages=pages, pages_per_tile=cfg["L"] * cfg["H"],
                                             page_size=cfg["ts"], max_seq_len=max_seq,
                                             prefix_cache=k == "cache_on")
        due = sum(len(p) - 1 for p in prompts)
        med = statistics.median(v)
        res[k] = {"seconds": [round(t, 4) for t in v], "median_s": round(med, 4),
                  "spread_s": round(max(v) - min(v), 4),
                  "generated_tokens_per_s": round(want / med, 1),
                  "decode_steps": max(r[0] for r in recs),
                  "positions_prefilled": due - st["positions_hit"],
                  "positions_hit": st["positions_hit"],
                  "deferrals": st["deferrals"], "evicted_blocks": st["evicted_blocks"]}
    diff = res["cache_on"]["median_s"] - res["cache_off"]["median_s"]
    res["off_over_on"] = round(res["cache_off"]["median_s"] / res["cache_on"]["median_s"], 3)
    res["on_minus_off_s"] = round(diff, 4)
    res["difference_exceeds_spread"] = bool(
        abs(diff) > max(res["cache_on"]["spread_s"], res["cache_off"]["spread_s"]))
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "serve_prefix.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=C3["L"])
    args = ap.parse_args()
    import llm_decoder
    from bench import make_weights
    cfg = dict(C3, L=args.layers)
    max_seq = 1024 + 256 + 128
    dec = llm_decoder.INT8Decoder(cfg["L"], cfg["H"], cfg["D"], cfg["H"] * cfg["D"], cfg["V"],
                                  max_seq, max_batch=MAXB, page_size=cfg["ts"])
    dec.set_weights(make_weights(cfg, 1234))
    dec.packed_prefill = True
    rng = np.random.default_rng(11)
    header = rng.integers(0, cfg["V"], 1024).tolist()
    shared = [header + rng.integers(0, cfg["V"], n).tolist()
              for n in rng.integers(64, 257, 128).tolist()]
    shared_new = rng.integers(16, 129, 128).tolist()
    rng = np.random.default_rng(7)  # (bench_serve.py's skewed arm)
    lens = rng.integers(128, 1025, 128).tolist()
    skew_new = rng.integers(16, 257, 128).tolist()
    skew = [rng.integers(0, cfg["V"], n).tolist() for n in lens]
    res = {"config": {"dims": cfg, "max_batch": MAXB, "max_seq_len": max_seq,
                      "packed_prefill": True, "reps": args.reps,
                      "timing": "wall clock, device synchronised around every window; sides "
                                "alternate"},
           "shared": arm(dec, cfg, "shared", shared, shared_new, args.reps, max_seq),
           "skewed": arm(dec, cfg, "skewed", skew, skew_new, args.reps, max_seq)}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
