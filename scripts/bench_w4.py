#!/usr/bin/env python3
"""INT4 weights against INT8 in one process: the decode step of an INT8Decoder
and of the same decoder loaded with int4=True (same dims, same synthetic
weights), the three 4-bit GEMMs alone against i8_gemm on the expanded weights,
and the accuracy record (logit error and greedy-token changes of the 4-bit
decoder against the 8-bit one, teacher forced).

The two sides alternate and every measurement repeats (--repeats); each figure
is reported as median with min and max.  Times are host clocks around windows
that end in a device synchronise, so the GEMM figures are call times that
include the host's enqueue cost, not kernel times: near the launch floor (a few
microseconds a call) they are a mix of both.  Writes one JSON document (--out).

    python scripts/bench_w4.py --config c3 --out profiles/w4.json
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
sys.path[:0] = [str(ROOT), str(ROOT / "pagedattention-based-transformer-decoder-inference-framework_amd")]

CONFIGS = {"c3": dict(L=24, H=16, D=128, V=50257), "c5": dict(L=32, H=32, D=128, V=50257),
           "tiny": dict(L=2, H=4, D=64, V=512)}
CTX = 256


def make_weights(cfg, seed):
    """Gaussian weights quantised per column to int8 (|w| <= 4 sigma -> 127):
    what a quantised model holds, unlike uniform int8, so that the accuracy
    record means something."""
    rng = np.random.default_rng(seed)
    L, hid, V = cfg["L"], cfg["H"] * cfg["D"], cfg["V"]
    inter = 4 * hid
    w = {"emb": rng.standard_normal((V, hid), dtype=np.float32).astype(np.float16).view(np.uint16)}
    for k, n in (("ln1_g", hid), ("ln2_g", hid)):
        w[k] = np.ones((L, n), np.float32)
    for k, n in (("ln1_b", hid), ("ln2_b", hid)):
        w[k] = 0.1 * rng.standard_normal((L, n), dtype=np.float32)
    w["b1"] = 0.02 * rng.standard_normal((L, inter), dtype=np.float32)
    w["b2"] = 0.02 * rng.standard_normal((L, hid), dtype=np.float32)
    for k, s, (K, N) in (("wqkv", "sw_qkv", (hid, 3 * hid)), ("wo", "sw_o", (hid, hid)),
                         ("w1", "sw1", (hid, inter)), ("w2", "sw2", (inter, hid))):
        x = rng.standard_normal((L, K, N), dtype=np.float32)
        w[k] = np.clip(np.rint(x * np.float32(127 / 4)), -127, 127).astype(np.int8)
        w[s] = np.full((L, N), 0.02 * 4 / 127, np.float32)
    return w


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def ratio(a, b):
    """int8 time over int4 time, window by window (> 1: int4 is faster)."""
    return spread([x / y for x, y in zip(a, b)])


def time_steps(dec, rows, steps, warmup):
    dec.begin_synthetic(rows, CTX, 7, True)
    dec.step([1] * rows, want_next=False)
    for _ in range(warmup):
        dec.step(None, want_next=False)
    dec.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        dec.step(None, want_next=False)
    dec.sync()
    return (time.perf_counter() - t0) / steps * 1e3  # ms per step


def bench_steps(d8, d4, args):
    out = {}
    for rows in (1, 8, 16, 64):
        t8, t4 = [], []
        for _ in range(args.repeats):
            t8.append(time_steps(d8, rows, args.steps, args.warmup))
            t4.append(time_steps(d4, rows, args.steps, args.warmup))
        out[str(rows)] = dict(int8_ms=spread(t8), int4_ms=spread(t4), speedup=ratio(t8, t4))
        print(f"step rows {rows}: int8 {out[str(rows)]['int8_ms']}, int4 {out[str(rows)]['int4_ms']}",
              file=sys.stderr, flush=True)
    return out


def bench_gemms(cfg, args):
    """Each GEMM alone, its weights as enough distinct copies (>= 512 MiB of the
    4-bit form) that a window streams them from HBM as a decode step does."""
    import torch
    import llm_capi
    hid = cfg["H"] * cfg["D"]
    rng = np.random.default_rng(3)
    out = {}
    for name, K, N in (("o_proj", hid, hid), ("fc1", hid, 4 * hid), ("fc2", 4 * hid, hid)):
        W8 = np.clip(np.rint(rng.standard_normal((K, N), dtype=np.float32) * (127 / 4)), -127, 127)
        q, m = llm_capi.w4_quantize(W8.astype(np.int8))
        E = torch.from_numpy(llm_capi.w4_expand(q, m)).cuda()
        qd, md = torch.from_numpy(q).cuda(), torch.from_numpy(m).cuda()
        copies = max(8, -(-(512 << 20) // (K * N // 2)))
        p4 = [llm_capi.w4_pack_weights(qd, md) for _ in range(copies)]
        p8 = [llm_capi.pack_weights(E, llm_capi.LLM_I8) for _ in range(copies)]
        sw = torch.full((N,), 1e-3, device="cuda")
        for M in (1, 16, 64):
            A = torch.from_numpy(rng.integers(-128, 128, (M, K), dtype=np.int8)).cuda()
            sa = torch.full((M,), 1e-3, device="cuda")
            C = torch.empty((M, N), device="cuda")
            lib, ptr = llm_capi.load(), llm_capi.ptr
            st = llm_capi.stream_ptr()

            def run(side):
                for i in range(args.gemm_calls):
                    if side == 8:
                        rc = lib.i8_gemm(ptr(A), K, ptr(p8[i % copies]), None, ptr(C), M, N, K,
                                         ptr(sa), ptr(sw), None, 0, st)
                    else:
                        rc = lib.w4_gemm(ptr(A), K, 0, ptr(p4[i % copies]), None, ptr(C), M, N, K,
                                         ptr(sa), ptr(sw), None, 0, st)
                    assert rc == 0, rc
                torch.cuda.synchronize()

            t8, t4 = [], []
            for r in range(args.repeats + 1):
                for side, ts in ((8, t8), (4, t4)):
                    t0 = time.perf_counter()
                    run(side)
                    if r:  # (window 0 warms up)
                        ts.append((time.perf_counter() - t0) / args.gemm_calls * 1e6)
            out[f"{name}_M{M}"] = dict(K=K, N=N, int8_us=spread(t8), int4_us=spread(t4),
                                       speedup=ratio(t8, t4))
            print(f"{name} M {M}: {out[f'{name}_M{M}']}", file=sys.stderr, flush=True)
        del p4, p8
    return out


def accuracy(d8, d4, cfg, rows=8, steps=8):
    """Teacher forced: both decoders take the 8-bit decoder's greedy token."""
    import torch
    V = cfg["V"]
    l8 = torch.empty((rows, V), device="cuda")
    l4 = torch.empty((rows, V), device="cuda")
    for d in (d8, d4):
        d.begin_synthetic(rows, CTX, 7, True)
    tok = list(range(1, rows + 1))
    rel, elem, flips = [], [], 0
    for _ in range(steps):
        n8 = d8.step(tok, logits_ptr=l8.data_ptr())
        n4 = d4.step(tok, logits_ptr=l4.data_ptr())
        torch.cuda.synchronize()
        a, b = l4.double(), l8.double()
        rel.append(float((a - b).abs().max() / b.abs().max()))
        elem.append(float(((a - b).abs() / b.abs().clamp_min(1e-6 * float(b.abs().max()))).max()))
        flips += sum(int(x != y) for x, y in zip(n8, n4))
        tok = list(n8)
    return dict(rows=rows, steps=steps, context=CTX, logit_rel_err_tensor_max=max(rel),
                logit_rel_err_elementwise_max=max(elem), greedy_tokens_changed=flips,
                greedy_tokens=rows * steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--gemm-calls", type=int, default=300)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "w4.json"))
    args = ap.parse_args()
    import torch
    import llm_decoder
    assert torch.cuda.is_available(), "bench_w4.py measures on a GPU: none found"
    cfg = CONFIGS[args.config]
    hid = cfg["H"] * cfg["D"]
    w = make_weights(cfg, 1)
    decs = []
    for int4 in (False, True):
        d = llm_decoder.INT8Decoder(cfg["L"], cfg["H"], cfg["D"], hid, cfg["V"], 512, max_batch=64)
        d.set_weights(w, int4=int4)
        decs.append(d)
    d8, d4 = decs
    del w
    res = dict(config=args.config, dims=cfg, context=CTX, steps=args.steps, repeats=args.repeats,
               device=torch.cuda.get_device_name(0),
               weight_bytes=dict(int8=d8.weight_bytes(), int4=d4.weight_bytes()),
               accuracy=accuracy(d8, d4, cfg), step_ms=bench_steps(d8, d4, args))
    del d8, d4, decs
    res["gemm_us"] = bench_gemms(cfg, args)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(dict(out=args.out, weight_bytes=res["weight_bytes"])))


if __name__ == "__main__":
    main()
