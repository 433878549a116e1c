#!/usr/bin/env python3
"""Prompt set-up of a batch: per-row prefill (one layer pass per row and chunk,
dec.prefill row by row -- what generate_batch does by default) against packed
prefill (dec.prefill_batch: the rows' tokens through shared passes of <= 512
packed tokens), on one C3-dims INT8Decoder in one process.

    python scripts/bench_prefill_packed.py [--layers 24] [--blocks 3]
                                           [--out profiles/prefill_packed.json]

Cases: 64 prompts x 128 tokens, 64 x 1,024, and 1 x 8,192 (one segment per
pass: packed should cost what per-row costs).  Every timed run starts from
fresh rows (begin_synthetic, not timed); the two forms alternate, `--blocks`
rounds each, after the warm-up of bench_prefill.py's decoder run (one 512-token
prefill of each form).  A run is timed with device events on the current
stream around the call and with the host clock; both prefill forms wait for
the decoder's stream at the end of every pass, so the two agree and the host
time is the prompt set-up latency.  The raw times go to --out."""
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
sys.path.insert(0, str(ROOT / "scripts"))

from bench_prefill import update_json  # noqa: E402

CASES = [(64, 128), (64, 1024), (1, 8192)]


def timed(fn):
    """(device-event ms, host ms) of one call that ends synchronised."""
    import torch
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    t0 = time.perf_counter()
    fn()
    dt = time.perf_counter() - t0
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), dt * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--kv-dtype", choices=["fp16", "fp8"], default="fp16")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "prefill_packed.json"))
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    import llm_decoder
    from bench import CONFIGS, make_weights
    cfg = dict(CONFIGS["c3"], L=args.layers)
    hid, ts = cfg["H"] * cfg["D"], cfg["ts"]
    max_rows = max(b for b, _ in CASES)
    max_seq = max(n for _, n in CASES) + 64
    # pages for the largest case (rows x layers x heads x tiles), not for
    # max_batch rows of max_seq_len tokens
    tiles = max(b * ((n + ts - 1) // ts + 1) for b, n in CASES)
    dec = llm_decoder.INT8Decoder(cfg["L"], cfg["H"], cfg["D"], hid, cfg["V"], max_seq,
                                  max_batch=max_rows, page_size=ts,
                                  num_pages=cfg["L"] * cfg["H"] * tiles,
                                  kv_dtype="fp8" if args.kv_dtype == "fp8" else "float16")
    dec.set_weights(make_weights(cfg, 1234))
    rng = np.random.default_rng(1)

    def per_row(prompts):
        for r, p in enumerate(prompts):
            dec.prefill(r, p)

    def packed(prompts):
        dec.prefill_batch(list(range(len(prompts))), prompts)

    forms = {"per_row": per_row, "packed": packed}
    warm = [rng.integers(0, cfg["V"], 512).tolist()]
    for fn in forms.values():  # warm: code objects, the prefill buffers
        dec.begin_synthetic(1, 0, 1, True)
        fn(warm)
        dec.sync()
    res = {"config": f"C3 dims ({cfg['L']}L/16H/D128, INT8), {args.kv_dtype} KV, one decoder, "
                     "one process", "blocks": args.blocks, "cases": []}
    for B, n in CASES:
        prompts = [rng.integers(0, cfg["V"], n).tolist() for _ in range(B)]
        runs = {name: {"event_ms": [], "host_ms": []} for name in forms}
        for _ in range(args.blocks):
            for name, fn in forms.items():
                dec.begin_synthetic(B, 0, 1, True)
                ev, host = timed(lambda: fn(prompts))
                runs[name]["event_ms"].append(round(ev, 3))
                runs[name]["host_ms"].append(round(host, 3))
        rec = {"prompts": B, "tokens_each": n, "passes_per_row": B * ((n + 511) // 512),
               "passes_packed": (B * n + 511) // 512}
        for name, r in runs.items():
            med = statistics.median(r["host_ms"])
            rec[name] = dict(r, median_host_ms=round(med, 3),
                             spread_host_ms=round(max(r["host_ms"]) - min(r["host_ms"]), 3),
                             prompt_tok_per_s=round(B * n / med * 1e3, 1))
        rec["per_row_over_packed"] = round(rec["per_row"]["median_host_ms"] /
                                           rec["packed"]["median_host_ms"], 3)
        res["cases"].append(rec)
        print(json.dumps(rec), flush=True)
    update_json(args.out, lambda d: d.__setitem__(f"{args.layers}L_{args.kv_dtype}", res))


if __name__ == "__main__":
    main()
