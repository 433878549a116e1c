"""What a sliding window buys a decode step, same box: a bench.py config's
decoder (default c3) with llm_decoder_set_window at each --windows value (0:
off), through begin_synthetic at the config's context, graph-replayed steps
timed with device events, the arms alternating over fresh decoders (the window
can only be set before rows are active; modelled on scripts/bench_rope.py).

Per arm and round: the step's ms, the attention launch's us alone
(llm_decoder_run_attention of layer 0 on a stream of its own, device events),
its plan (llm_decoder_attention_plan) and its TB/s over its algorithmic bytes,
which are min(context, W) tokens of K and V per (row, head).

    python scripts/bench_window.py [--config c3] [--windows 0 4096 1024]
                                   [--steps 30] [--warmup 5] [--rounds 3] [--out FILE]

Prints one line per arm and round, then the JSON summary (also written to
--out, default profiles/window_<config>.json)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "pagedattention-based-transformer-decoder-inference-framework_amd")]


def run(cfg, args, window):
    import numpy as np
    import torch
    import bench
    import llm_decoder
    B, T = cfg["B"], cfg["T"]
    max_seq = T + 2 * (args.warmup + args.steps) + 16
    dec = getattr(llm_decoder, cfg["cls"])(cfg["L"], cfg["H"], cfg["D"], cfg["H"] * cfg["D"],
                                           cfg["V"], max_seq, max_batch=B, page_size=cfg["ts"])
    dec.set_weights(bench.make_weights(cfg, args.seed))
    dec.set_window(window)
    assert dec.window == window
    dec.begin_synthetic(B, T, args.seed, True)
    nsplit, form = dec.attention_plan()
    tok = [int(t) for t in np.random.default_rng(args.seed).integers(0, cfg["V"], B)]
    # a stream of its own: the C ABI reads torch's default stream (handle 0) as
    # "the decoder's own stream", which the events below would not be ordered on
    stream = torch.cuda.Stream()
    dec.step(tok, stream=stream.cuda_stream, want_next=False)
    for _ in range(args.warmup):
        dec.step(None, stream=stream.cuda_stream, want_next=False)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(args.steps):
        dec.step(None, stream=stream.cuda_stream, want_next=False)
    t1.record(stream)
    torch.cuda.synchronize()
    dec.sync()
    step_ms = t0.elapsed_time(t1) / args.steps
    # the attention launch alone, at the rows' live context
    ctx = dec.context_len(0)
    for _ in range(3):
        dec.run_attention(0, stream.cuda_stream)
    torch.cuda.synchronize()
    t0.record(stream)
    for _ in range(args.attn_iters):
        dec.run_attention(0, stream.cuda_stream)
    t1.record(stream)
    torch.cuda.synchronize()
    attn_us = t0.elapsed_time(t1) / args.attn_iters * 1e3
    es = 1 if getattr(dec, "kv_dtype", "float16") != "float16" else 2
    tokens = min(ctx, window) if window > 0 else ctx
    nbytes = 2.0 * B * cfg["H"] * tokens * cfg["D"] * es
    del dec
    torch.cuda.empty_cache()
    return {"step_ms": round(step_ms, 4), "attn_us": round(attn_us, 2), "nsplit": nsplit,
            "form": form, "context": ctx, "tokens_per_row": tokens,
            "attn_TBps": round(nbytes / attn_us / 1e6, 3)}


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(bench.CONFIGS))
    ap.add_argument("--windows", type=int, nargs="+", default=[0, 4096, 1024])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--attn-iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = bench.CONFIGS[args.config]
    runs = {str(w): [] for w in args.windows}
    for r in range(args.rounds):
        for w in args.windows:
            rec = run(cfg, args, w)
            runs[str(w)].append(rec)
            print(f"{args.config} window {w} round {r + 1}: {rec['step_ms']:.4f} ms/step, attention "
                  f"{rec['attn_us']:.1f} us ({rec['nsplit']} splits, form {rec['form']}, "
                  f"{rec['attn_TBps']:.2f} TB/s over {rec['tokens_per_row']} tokens/row)", flush=True)
    arms = {}
    for w, rs in runs.items():
        arms[w] = {"step_ms_median": statistics.median(r["step_ms"] for r in rs),
                   "step_ms_spread": round(max(r["step_ms"] for r in rs) - min(r["step_ms"] for r in rs), 4),
                   "attn_us_median": statistics.median(r["attn_us"] for r in rs),
                   "attn_TBps_median": statistics.median(r["attn_TBps"] for r in rs),
                   "nsplit": rs[0]["nsplit"], "form": rs[0]["form"],
                   "tokens_per_row": rs[0]["tokens_per_row"], "rounds": rs}
    doc = {"config": args.config, "B": cfg["B"], "L": cfg["L"], "H": cfg["H"], "D": cfg["D"],
           "context": cfg["T"], "steps": args.steps, "attn_iters": args.attn_iters, "arms": arms}
    out = Path(args.out) if args.out else ROOT / "profiles" / f"window_{args.config}.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
