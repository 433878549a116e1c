#!/usr/bin/env python3
"""fp16-KV against FP8-KV on one box: the decoder's own attention launch
(llm_decoder_run_attention) and its whole step, at a bench.py config's shape
(default C3: 24 L / 16 H / D 128, 64 rows at context 8192, shuffled pages).

One process, the same weights.  The two pools (C3: 103 GB and 52 GB) never sit
together: a decoder is destroyed before the next is created, so the arms
alternate by BLOCKS -- fp16, fp8, fp16, fp8, ... -- each block a fresh decoder
(begin_synthetic with the same seed), warmed up, then timed with device events.
Per arm the result holds the median over blocks of the launch time and the
step time, the spread across blocks (max - min), the algorithmic bytes of the
launch (from the shapes) and the achieved TB/s and fraction of 8 TB/s.

    python scripts/kv_fp8_ab.py [--config c3] [--blocks 5] [--launches 40] [--steps 10]
                                [--out profiles/kv_fp8_c3.json]

The requirement it checks (and prints): the FP8 launch is not slower than the
fp16 launch by more than the fp16 arm's own block-to-block spread."""
import argparse
import gc
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "pagedattention-based-transformer-decoder-inference-framework_amd"))

HBM_PEAK = 8.0e12


def launch_bytes(cfg, B, ctx, es):
    """Algorithmic HBM bytes of one attention launch: K and V of every (row,
    head, token), the page-table entries, q in and the fp32 rows out."""
    H, D, ts = cfg["H"], cfg["D"], cfg["ts"]
    tiles = (ctx + ts - 1) // ts
    return B * H * (2 * ctx * D * es + 4 * tiles + 2 * 4 * D)


def timed(fn, n, stream):
    """Mean ms of n calls of fn, which enqueues on `stream` (events on it too)."""
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record(stream)
    for _ in range(n):
        fn()
    e.record(stream)
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def one_block(cls, cfg, w, kv_dtype, args):
    import torch
    B, T = cfg["B"], cfg["T"]
    max_seq = T + args.steps + args.warmup + 16
    dec = cls(cfg["L"], cfg["H"], cfg["D"], cfg["H"] * cfg["D"], cfg["V"], max_seq, max_batch=B,
              page_size=cfg["ts"], kv_dtype=kv_dtype)
    dec.set_weights(w)
    dec.begin_synthetic(B, T, args.seed, True)
    # a stream of the caller's: handle 0 (torch's default stream) would mean the
    # decoder's own stream, which the events below would not see
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    assert st != 0
    for _ in range(args.warmup):
        dec.step(None, stream=st, want_next=False)
    for _ in range(args.warmup):
        dec.run_attention(0, st)
    plan = dec.attention_plan()
    ctx = dec.context_len(0) + 1  # the launch attends the row's live context
    layers = cfg["L"]
    k = [0]

    def launch():  # walk the layers: each launch reads its own layer's pages
        dec.run_attention(k[0] % layers, st)
        k[0] += 1

    launch_ms = timed(launch, args.launches, stream)
    step_ms = timed(lambda: dec.step(None, stream=st, want_next=False), args.steps, stream)
    dec.sync()
    del dec
    gc.collect()
    torch.cuda.synchronize()
    return dict(launch_us=launch_ms * 1e3, step_ms=step_ms, nsplit=plan[0], form=plan[1], ctx=ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import llm_decoder
    import bench
    cfg = bench.CONFIGS[args.config]
    assert not cfg.get("beams"), "plain (non-beam) configs only"
    torch.cuda.set_device(0)
    w = bench.make_weights(cfg, args.seed)
    cls = getattr(llm_decoder, cfg["cls"])
    arms = {"float16": [], "fp8": []}
    for blk in range(args.blocks):
        for kv_dtype in ("float16", "fp8"):
            r = one_block(cls, cfg, w, kv_dtype, args)
            arms[kv_dtype].append(r)
            print(f"block {blk} {kv_dtype}: launch {r['launch_us']:.1f} us, step "
                  f"{r['step_ms']:.3f} ms, {r['nsplit']} splits form {r['form']}",
                  file=sys.stderr, flush=True)
    res = {"config": args.config, "rows": cfg["B"], "context": cfg["T"], "blocks": args.blocks,
           "launches_per_arm": args.blocks * args.launches, "steps_per_arm": args.blocks * args.steps}
    for kv_dtype, rs in arms.items():
        es = 1 if kv_dtype == "fp8" else 2
        lu = [r["launch_us"] for r in rs]
        sm = [r["step_ms"] for r in rs]
        nbytes = launch_bytes(cfg, cfg["B"], rs[0]["ctx"], es)
        med = statistics.median(lu)
        res[kv_dtype] = {
            "launch_us_median": round(med, 2), "launch_us_blocks": [round(x, 2) for x in lu],
            "launch_us_spread": round(max(lu) - min(lu), 2),
            "step_ms_median": round(statistics.median(sm), 4),
            "step_ms_blocks": [round(x, 4) for x in sm],
            "step_ms_spread": round(max(sm) - min(sm), 4),
            "launch_bytes": nbytes, "tb_per_s": round(nbytes / (med * 1e-6) / 1e12, 3),
            "frac_of_8tbps": round(nbytes / (med * 1e-6) / HBM_PEAK, 4),
            "nsplit": rs[0]["nsplit"], "form": rs[0]["form"]}
    f16, f8 = res["float16"], res["fp8"]
    res["fp8_launch_vs_fp16"] = round(f8["launch_us_median"] / f16["launch_us_median"], 4)
    res["requirement_fp8_not_slower_than_fp16_plus_spread"] = bool(
        f8["launch_us_median"] <= f16["launch_us_median"] + f16["launch_us_spread"])
    out = Path(args.out) if args.out else ROOT / "profiles" / f"kv_fp8_{args.config}.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
