#!/usr/bin/env python3
"""RMSNorm as the gated kernel's prologue against the two launches it replaces,
and the decode step it changes.  One process, one GPU, the two sides of every
comparison in alternating windows; window 0 warms up.

Kernels: i8_gemm_gated_rms against rmsnorm_quant + i8_gemm_gated on the same
fp32 rows.  Each side is a captured graph of `calls` launches (launch pairs)
cycling through enough weight copies (>= 512 MiB) that they stream from HBM, so
the figure is device time per call as a step graph sees it, not the host's
enqueue.  Times are the host clock around a replay that ends in a device
synchronise.  Row counts the prologue refuses are reported as such.

Step: an INT8 decoder of C3's dimensions (24 layers, 16 heads of 128, gated
inter 5632, context 512) under set_norm("rms") + set_mlp("gated_silu") against
the same weights under LayerNorm + gated, the step graph of each replayed.
Writes profiles/rmsnorm.json."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "pagedattention-based-transformer-decoder-inference-framework_amd"))

SHAPES = ((2048, 5632), (4096, 11008))
ROWS = (8, 16, 32)
STEP_ROWS = (8, 16, 64)


def spread(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def windows(sides, repeats, per):
    """Alternating timed windows of callables; microseconds per `per` units each."""
    import torch
    out = [[] for _ in sides]
    for r in range(repeats + 1):
        for side, ts in zip(sides, out):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            side()
            torch.cuda.synchronize()
            if r:
                ts.append((time.perf_counter() - t0) * 1e6 / per)
    return out


def kernels(args, res):
    import torch
    import llm_capi
    lib, ptr = llm_capi.load(), llm_capi.ptr
    rng = np.random.default_rng(3)
    for K, N in SHAPES:
        copies = max(4, -(-(512 << 20) // (2 * K * N)))
        W = [torch.from_numpy(rng.integers(-127, 128, (K, N), dtype=np.int8)).cuda()
             for _ in range(2)]
        pg = [llm_capi.pack_weights(W[0], llm_capi.LLM_I8) for _ in range(copies)]
        pu = [llm_capi.pack_weights(W[1], llm_capi.LLM_I8) for _ in range(copies)]
        sw = torch.full((N,), 2.0 / (5400 * K ** 0.5), device="cuda")
        gamma = torch.from_numpy((1 + 0.1 * rng.standard_normal(K)).astype(np.float32)).cuda()
        for M in ROWS:
            x = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32)).cuda()
            q = torch.empty((M, K), dtype=torch.int8, device="cuda")
            sa = torch.empty((M,), device="cuda")
            H1, H2 = (torch.empty((M, N), device="cuda") for _ in range(2))
            silu = llm_capi.LLM_MLP_GATED_SILU

            def fused(i, st):
                return lib.i8_gemm_gated_rms(ptr(x), ptr(gamma), 1e-5, ptr(pg[i % copies]),
                                             ptr(pu[i % copies]), None, None, ptr(H1), None, M, N,
                                             K, ptr(sw), ptr(sw), None, None, silu, None, None, st)

            def pair(i, st):
                rc = lib.rmsnorm_quant(ptr(x), M, K, ptr(gamma), 1e-5, None, ptr(q), ptr(sa), st)
                return rc | lib.i8_gemm_gated(ptr(q), K, 0, ptr(pg[i % copies]),
                                              ptr(pu[i % copies]), None, None, ptr(H2), None, M, N,
                                              K, ptr(sa), ptr(sw), ptr(sw), None, None, silu, st)

            key = f"K{K}_N{N}_M{M}"
            if fused(0, None) != 0:
                res["kernels"][key] = dict(fused="unsupported: " + lib.llm_last_error().decode())
                continue
            assert pair(0, None) == 0
            torch.cuda.synchronize()
            same = bool(torch.equal(H1, H2))
            graphs = []
            for side in (fused, pair):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    st = llm_capi.stream_ptr()
                    for i in range(args.calls):
                        assert side(i, st) == 0
                graphs.append(g)
            tf, tp = windows([g.replay for g in graphs], args.repeats, args.calls)
            row = dict(fused_us=spread(tf), norm_plus_gated_us=spread(tp),
                       speedup=spread([p / f for p, f in zip(tp, tf)]), bit_equal=same)
            res["kernels"][key] = row
            print(f"{key}: {row}", file=sys.stderr, flush=True)
        del pg, pu


def steps(args, res):
    import torch
    import llm_decoder
    L, H, D, V, T, inter = 24, 16, 128, 50257, 512, 5632
    hid = H * D
    rng = np.random.default_rng(5)
    w = {"emb": rng.standard_normal((V, hid), dtype=np.float32).astype(np.float16).view(np.uint16)}
    for k, n in (("ln1_g", hid), ("ln2_g", hid), ("ln1_b", hid), ("ln2_b", hid), ("b1", inter),
                 ("b2", hid), ("b_up", inter)):
        w[k] = (0.05 * rng.standard_normal((L, n), dtype=np.float32)) + (k[-1] == "g")
    for k, s, (kk, n) in (("wqkv", "sw_qkv", (hid, 3 * hid)), ("wo", "sw_o", (hid, hid)),
                          ("w1", "sw1", (hid, inter)), ("w2", "sw2", (inter, hid)),
                          ("w_up", "sw_up", (hid, inter))):
        w[k] = np.repeat(rng.integers(-127, 128, (1, kk, n), dtype=np.int8), L, axis=0)
        w[s] = np.full((L, n), 0.02 * 3.0 / 127.0, np.float32)
    for B in STEP_ROWS:
        decs = []
        for norm in ("rms", "layer"):
            dec = llm_decoder.INT8Decoder(L, H, D, hid, V, T + 512, max_batch=B, inter_dim=inter)
            dec.set_norm(norm)
            dec.set_mlp("gated_silu")
            dec.set_weights(w)
            dec.begin_synthetic(B, T, 1, True)
            decs.append(dec)
        toks = list(range(1, B + 1))

        def run(dec):
            def f():
                for _ in range(args.steps):
                    dec.step(toks, want_next=False)
            return f

        tr, tl = windows([run(d) for d in decs], args.repeats, args.steps)
        row = dict(rms_gated_us=spread(tr), layernorm_gated_us=spread(tl),
                   speedup=spread([a / b for a, b in zip(tl, tr)]))
        res["step"][f"B{B}"] = row
        print(f"step B {B}: {row}", file=sys.stderr, flush=True)
        del decs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rmsnorm.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_rmsnorm.py measures on a GPU: none found"
    res = dict(device=torch.cuda.get_device_name(0), calls=args.calls, steps=args.steps,
               repeats=args.repeats, kernels={}, step={})
    kernels(args, res)
    steps(args, res)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(dict(out=args.out)))


if __name__ == "__main__":
    main()
