#!/usr/bin/env python3
"""Prefill attention: the MFMA chunk kernel (pa_prefill) against the same rows
through the decode kernel (pa_decode with beam_ids = row, context_lens =
p0 + i + 1), and a whole-decoder prompt prefill.

    python scripts/bench_prefill.py [--p0 7680] [--m 512] [--prompt 4096]
                                    [--kv-dtype fp16|fp8 ...]

One --kv-dtype: the kernels and the decoder on pools of that type; prints one
JSON line.  Both (--kv-dtype fp8 fp16): the same-process A/B of FP8 pa_prefill,
fp16 pa_prefill and the FP8 rows through pa_decode (what an FP8 decoder ran
for a prompt chunk before pa_prefill read FP8 pools), in alternating blocks
timed with device events; the medians and block-to-block spreads go to --out
(default profiles/prefill_fp8.json, key "kernel_ab").

--window W [W ...]: only time the (--p0, --m) chunk of C3's heads through
pa_prefill_window at each W (0: off), alternating blocks as the A/B above; the
medians, spreads and the algorithmic rate over the visible (query, key) pairs
go to --out under "window" (profiles/prefill_window.json).

--e2e N: only time `prefill` of an N-token prompt on a C3-dims INT8Decoder of
--layers layers with KV pools of the (one) --kv-dtype, and store it in --out
under "e2e"[--label] (run it once per library build on the same box, as
scripts/gpu_lib_ab.sh does for bench.py: --module-dir names the other build's
directory, with a --label each).

Attention flops are algorithmic (4·H·D per (query, key) pair, causal pairs
only), not the hi/lo MFMA count."""
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


def time_cuda(fn, iters=10):
    import torch
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def make_pools(rng, num_pages, ts, D, kv_dtype):
    """Device K / V pools [num_pages][ts][D] of `kv_dtype` ("fp16" | "fp8":
    the same random values, e4m3-encoded at scale 1)."""
    import torch
    import llm_capi
    k = (rng.standard_normal((num_pages, ts, D)) * D ** -0.25).astype(np.float32)
    v = rng.standard_normal((num_pages, ts, D)).astype(np.float32)
    if kv_dtype == "fp8":
        return tuple(torch.from_numpy(llm_capi.fp8_encode(x)).cuda().view(torch.float8_e4m3fn)
                     for x in (k, v))
    return tuple(torch.from_numpy(x.astype(np.float16)).cuda() for x in (k, v))


def make_case(H, D, ts, p0, m, kv_dtypes):
    """{dtype: (k, v)}, page table, q, out, beam ids, context lens (one seed for every dtype)."""
    import torch
    T = p0 + m
    nt = (T + ts - 1) // ts
    num_pages = H * nt + 3
    pools = {d: make_pools(np.random.default_rng(0), num_pages, ts, D, d) for d in kv_dtypes}
    rng = np.random.default_rng(1)
    pt = torch.from_numpy(rng.permutation(num_pages)[:H * nt].astype(np.int32).reshape(1, H, nt)).cuda()
    q = torch.from_numpy((rng.standard_normal((m, H, D)) * D ** -0.25).astype(np.float32)).cuda()
    out = torch.empty((m, H, D), dtype=torch.float32, device="cuda")
    bi = torch.zeros(m, dtype=torch.int32, device="cuda")
    cl = torch.arange(p0 + 1, T + 1, dtype=torch.int32, device="cuda")
    return pools, pt, q, out, bi, cl


def kernel_bench(H, D, ts, p0, m, kv_dtype="fp16"):
    import llm_capi
    T = p0 + m
    pools, pt, q, out, bi, cl = make_case(H, D, ts, p0, m, [kv_dtype])
    kp, vp = pools[kv_dtype]
    t_pf = time_cuda(lambda: llm_capi.pa_prefill(q, kp, vp, pt, row=0, p0=p0, out=out))
    t_dec = time_cuda(lambda: llm_capi.pa_decode(q, kp, vp, pt, T=T, beam_ids=bi, context_lens=cl))
    pairs = m * p0 + m * (m + 1) // 2
    flops = 4.0 * H * D * pairs
    es = 1 if kv_dtype == "fp8" else 2
    return {"H": H, "D": D, "page": ts, "p0": p0, "m": m, "kv_dtype": kv_dtype,
            "prefill_us": round(t_pf, 1), "decode_rows_us": round(t_dec, 1),
            "speedup": round(t_dec / t_pf, 2), "prefill_TFLOPs": round(flops / t_pf / 1e6, 1),
            "kv_unique_GB": round(2 * H * T * D * es / 1e9, 4)}


def kernel_ab(H, D, ts, p0, m, blocks=7, iters=10):
    """FP8 pa_prefill / fp16 pa_prefill / FP8 rows through pa_decode, one block
    of `iters` launches each in turn, `blocks` rounds: median us per launch and
    the block-to-block spread (max - min over the blocks) of each."""
    import llm_capi
    T = p0 + m
    pools, pt, q, out, bi, cl = make_case(H, D, ts, p0, m, ["fp8", "fp16"])
    (k8, v8), (k16, v16) = pools["fp8"], pools["fp16"]
    forms = {
        "fp8_prefill": lambda: llm_capi.pa_prefill(q, k8, v8, pt, row=0, p0=p0, out=out),
        "fp16_prefill": lambda: llm_capi.pa_prefill(q, k16, v16, pt, row=0, p0=p0, out=out),
        "fp8_decode_rows": lambda: llm_capi.pa_decode(q, k8, v8, pt, T=T, beam_ids=bi,
                                                      context_lens=cl, out=out),
    }
    for fn in forms.values():  # warm: code objects, workspaces
        time_cuda(fn, 3)
    times = {name: [] for name in forms}
    for _ in range(blocks):
        for name, fn in forms.items():
            times[name].append(time_cuda(fn, iters))
    res = {"H": H, "D": D, "page": ts, "p0": p0, "m": m, "blocks": blocks, "iters_per_block": iters}
    for name, ts_ in times.items():
        res[name] = {"median_us": round(statistics.median(ts_), 1),
                     "spread_us": round(max(ts_) - min(ts_), 1),
                     "blocks_us": [round(t, 1) for t in ts_]}
    med = {n: res[n]["median_us"] for n in forms}
    res["fp8_prefill_vs_decode_rows"] = round(med["fp8_decode_rows"] / med["fp8_prefill"], 2)
    res["fp8_vs_fp16_prefill"] = round(med["fp8_prefill"] / med["fp16_prefill"], 3)
    res["faster_than_decode_rows_by_more_than_its_spread"] = bool(
        med["fp8_decode_rows"] - med["fp8_prefill"] > res["fp8_decode_rows"]["spread_us"])
    return res


def window_ab(H, D, ts, p0, m, windows, kv_dtype="fp16", blocks=7, iters=10):
    """pa_prefill_window of one chunk at each window of `windows` (0: off), one
    block of `iters` launches each in turn, `blocks` rounds.  Visible pairs of a
    query at position p: min(p + 1, W)."""
    import llm_capi
    pools, pt, q, out, bi, cl = make_case(H, D, ts, p0, m, [kv_dtype])
    kp, vp = pools[kv_dtype]
    forms = {W: (lambda W=W: llm_capi.pa_prefill(q, kp, vp, pt, row=0, p0=p0, out=out, window=W))
             for W in windows}
    for fn in forms.values():
        time_cuda(fn, 3)
    times = {W: [] for W in windows}
    for _ in range(blocks):
        for W, fn in forms.items():
            times[W].append(time_cuda(fn, iters))
    res = {"H": H, "D": D, "page": ts, "p0": p0, "m": m, "kv_dtype": kv_dtype, "blocks": blocks,
           "iters_per_block": iters, "arms": {}}
    for W, ts_ in times.items():
        pairs = sum(min(p + 1, W) if W > 0 else p + 1 for p in range(p0, p0 + m))
        med = statistics.median(ts_)
        res["arms"][str(W)] = {"median_us": round(med, 1), "spread_us": round(max(ts_) - min(ts_), 1),
                               "blocks_us": [round(t, 1) for t in ts_], "visible_pairs": pairs,
                               "TFLOPs_over_visible_pairs": round(4.0 * H * D * pairs / med / 1e6, 1)}
    return res


def decoder_bench(prompt, kv_dtype="fp16", layers=None):
    import llm_decoder
    from bench import CONFIGS, make_weights
    cfg = dict(CONFIGS["c3"])
    if layers:
        cfg["L"] = layers
    hid = cfg["H"] * cfg["D"]
    dec = llm_decoder.INT8Decoder(cfg["L"], cfg["H"], cfg["D"], hid, cfg["V"], prompt + 64,
                                  max_batch=1, page_size=cfg["ts"],
                                  kv_dtype="fp8" if kv_dtype == "fp8" else "float16")
    dec.set_weights(make_weights(cfg, 1234))
    toks = np.random.default_rng(1).integers(0, cfg["V"], prompt).tolist()
    dec.begin_synthetic(1, 0, 1, True)
    dec.prefill(0, toks[:512])  # warm
    dec.sync()
    dec.begin_synthetic(1, 0, 1, True)
    t0 = time.perf_counter()
    dec.prefill(0, toks)
    dec.sync()
    dt = time.perf_counter() - t0
    del dec
    return dt


def update_json(path, fn):
    path = Path(path)
    doc = json.loads(path.read_text()) if path.exists() else {}
    fn(doc)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(doc, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p0", type=int, default=7680)
    ap.add_argument("--m", type=int, default=512)
    ap.add_argument("--prompt", type=int, default=4096)
    ap.add_argument("--no-decoder", action="store_true")
    ap.add_argument("--kv-dtype", nargs="+", choices=["fp16", "fp8"], default=["fp16"],
                    help="KV pool type; both: the same-process FP8 / fp16 / decode-rows A/B")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--window", type=int, nargs="+", default=None, metavar="W",
                    help="only time the chunk through pa_prefill_window at each W (0: off)")
    ap.add_argument("--e2e", type=int, default=0, metavar="N",
                    help="only time prefill of an N-token prompt (C3 dims, --layers layers)")
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--label", default="this")
    ap.add_argument("--module-dir", default=None, metavar="DIR",
                    help="--e2e: import llm_decoder from DIR (another revision's build of the "
                         "module, beside its own libllm_decoder_hip.so)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "prefill_fp8.json"))
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    kvd = list(dict.fromkeys(args.kv_dtype))
    if args.window is not None:
        rec = window_ab(16, 128, 16, args.p0, args.m, args.window, kvd[0], blocks=args.blocks)
        update_json(args.out, lambda d: d.__setitem__("window", rec))
        print(json.dumps({"window": rec}), flush=True)
        return
    if args.e2e:
        if len(kvd) != 1:
            ap.error("--e2e takes one --kv-dtype")
        if args.module_dir:
            sys.path.insert(0, str(Path(args.module_dir).resolve()))
        ts_ = [decoder_bench(args.e2e, kvd[0], args.layers) for _ in range(3)]
        rec = {"config": f"C3 dims ({args.layers}L/16H/D128, INT8), batch 1, {kvd[0]} KV",
               "prompt_tokens": args.e2e, "prefill_s": round(min(ts_), 4),
               "runs_s": [round(t, 4) for t in ts_],
               "prompt_tok_per_s": round(args.e2e / min(ts_), 1)}
        update_json(args.out, lambda d: d.setdefault("e2e", {}).__setitem__(args.label, rec))
        print(json.dumps({"e2e": {args.label: rec}}), flush=True)
        return
    if len(kvd) == 2:
        rec = kernel_ab(16, 128, 16, args.p0, args.m, blocks=args.blocks)
        update_json(args.out, lambda d: d.__setitem__("kernel_ab", rec))
        print(json.dumps({"kernel_ab": rec}), flush=True)
        return
    res = {"kernel": [kernel_bench(16, 128, 16, args.p0, args.m, kvd[0]),
                      kernel_bench(16, 128, 16, 0, args.m, kvd[0]),
                      kernel_bench(12, 64, 16, 1536, args.m, kvd[0])]}
    if not args.no_decoder:
        t1 = decoder_bench(args.prompt, kvd[0])
        res["decoder"] = {"config": f"C3 dims (24L/16H/D128, INT8), batch 1, {kvd[0]} KV",
                          "prompt_tokens": args.prompt, "mfma_prefill_s": round(t1, 3),
                          "mfma_prompt_tok_per_s": round(args.prompt / t1, 1)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
