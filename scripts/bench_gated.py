#!/usr/bin/env python3
"""The gated-MLP launch (i8_gemm_gated, csrc/gemm_gated.hip) against the only
other way to compute H = silu(G) * U on the device: two i8_gemm calls of
N = inter plus an elementwise torch op.  One process, one GPU, the two sides in
alternating windows; each side's weights are enough distinct copies (>= 512
MiB) that a window streams them from HBM as a decode step does; window 0 warms
up.  Times are host clock over a window that ends in a device synchronise,
per call.  The two results are compared on the same inputs before timing.
Writes profiles/gated_mlp.json."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "pagedattention-based-transformer-decoder-inference-framework_amd"))

SHAPES = ((2048, 5632), (4096, 11008))
ROWS = (8, 64, 512)


def spread(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gated_mlp.json"))
    args = ap.parse_args()
    import torch
    import llm_capi
    assert torch.cuda.is_available(), "bench_gated.py measures on a GPU: none found"
    lib, ptr, st = llm_capi.load(), llm_capi.ptr, llm_capi.stream_ptr()
    rng = np.random.default_rng(3)
    res = dict(device=torch.cuda.get_device_name(0), calls=args.calls, repeats=args.repeats,
               activation="silu", shapes={})
    for K, N in SHAPES:
        copies = max(4, -(-(512 << 20) // (2 * K * N)))
        W = [torch.from_numpy(rng.integers(-127, 128, (K, N), dtype=np.int8)).cuda()
             for _ in range(2)]
        pg = [llm_capi.pack_weights(W[0], llm_capi.LLM_I8) for _ in range(copies)]
        pu = [llm_capi.pack_weights(W[1], llm_capi.LLM_I8) for _ in range(copies)]
        sw = torch.full((N,), 2.0 / (5400 * K ** 0.5), device="cuda")
        for M in ROWS:
            A = torch.from_numpy(rng.integers(-128, 128, (M, K), dtype=np.int8)).cuda()
            sa = torch.ones((M,), device="cuda")
            G, U, H2, H1 = (torch.empty((M, N), device="cuda") for _ in range(4))

            def fused(i):
                return lib.i8_gemm_gated(ptr(A), K, 0, ptr(pg[i % copies]), ptr(pu[i % copies]),
                                         None, None, ptr(H1), None, M, N, K, ptr(sa), ptr(sw),
                                         ptr(sw), None, None, llm_capi.LLM_MLP_GATED_SILU, st)

            def unfused(i):
                rc = lib.i8_gemm(ptr(A), K, ptr(pg[i % copies]), None, ptr(G), M, N, K, ptr(sa),
                                 ptr(sw), None, 0, st)
                rc |= lib.i8_gemm(ptr(A), K, ptr(pu[i % copies]), None, ptr(U), M, N, K, ptr(sa),
                                  ptr(sw), None, 0, st)
                torch.mul(torch.nn.functional.silu(G), U, out=H2)
                return rc

            assert fused(0) == 0 and unfused(0) == 0
            torch.cuda.synchronize()
            diff = float((H1.double() - H2.double()).abs().max() / H2.double().abs().max())
            tf, tu = [], []
            for r in range(args.repeats + 1):
                for side, ts in ((fused, tf), (unfused, tu)):
                    t0 = time.perf_counter()
                    for i in range(args.calls):
                        assert side(i) == 0
                    torch.cuda.synchronize()
                    if r:
                        ts.append((time.perf_counter() - t0) / args.calls * 1e6)
            row = dict(fused_us=spread(tf), two_gemms_plus_torch_us=spread(tu),
                       speedup=spread([u / f for u, f in zip(tu, tf)]), max_rel_diff=diff,
                       weight_mib_per_call=2 * K * N / 2 ** 20)
            res["shapes"][f"K{K}_N{N}_M{M}"] = row
            print(f"K {K} inter {N} M {M}: {row}", file=sys.stderr, flush=True)
        del pg, pu
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(dict(out=args.out)))


if __name__ == "__main__":
    main()
