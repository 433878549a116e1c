"""Streaming token choice (csrc/sample_wide.hip) against the row-holding kernels,
recorded in profiles/sample_wide.json.  Nothing is gated on these figures and
nothing at V <= 65536 is rerouted by them.

One process; per shape the arms alternate call by call inside each repeat, so
drift of the shared host lands on every arm alike.  Arms per (V, rows):
  sample_each_{narrow,wide}   per-row settings: temperature 0.8, top_k 40, top_p 0.9
  sample_plain_{narrow,wide}  temperature 1, no filter (the wide kernel skips passes 2-3)
  logprob8_{narrow,wide}      chosen + top 8
  lm_head_entry               the one-shot lm_head entry at hidden 2048, for scale.  It
                              packs E first (reads and writes E once more), so it is
                              about three times the weight traffic of the decoder's
                              LM head, which packs at load
narrow arms exist at V <= 65536 only.  Logits: 4 * N(0, 1), seeded.  Each figure
is the median over REPEATS of a device-event time around INNER back-to-back
launches, in microseconds per launch.
"""
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pagedattention-based-transformer-decoder-inference-framework_amd"))
sys.path.insert(0, str(ROOT / "scripts"))

from bench_prefill import update_json  # noqa: E402

VOCABS = [50257, 65536, 128256, 151936, 262144]
ROWS = [1, 16, 64]
HIDDEN, REPEATS, INNER = 2048, 9, 20


def main():
    import torch

    import llm_capi
    assert torch.cuda.is_available(), "bench_sample_wide needs a GPU"
    out = {}
    for V in VOCABS:
        g = torch.Generator(device="cuda").manual_seed(V)
        E = (0.02 * torch.randn((V, HIDDEN), device="cuda", generator=g)).half()
        for R in ROWS:
            lg = 4.0 * torch.randn((R, V), device="cuda", generator=g)
            x = torch.randn((R, HIDDEN), device="cuda", generator=g)
            t = torch.full((R,), 0.8, device="cuda")
            k = torch.full((R,), 40, dtype=torch.int32, device="cuda")
            p = torch.full((R,), 0.9, device="cuda")
            seed = torch.arange(R, dtype=torch.int64, device="cuda")
            ctr = torch.zeros(R, dtype=torch.int32, device="cuda")
            chosen = torch.zeros(R, dtype=torch.int32, device="cuda")
            arms = {}
            for w in ([False, True] if V <= 65536 else [True]):
                tag = "wide" if w else "narrow"
                arms["sample_each_" + tag] = lambda w=w: llm_capi.sample_rows_each(
                    lg, t, k, p, seed, ctr, wide=w)
                arms["sample_plain_" + tag] = lambda w=w: llm_capi.sample_rows(lg, wide=w)
                arms["logprob8_" + tag] = lambda w=w: llm_capi.logprob_rows(lg, chosen, 8, wide=w)
            arms["lm_head_entry"] = lambda: llm_capi.lm_head(x, E)
            times = {a: [] for a in arms}
            for rep in range(REPEATS + 1):  # (the first repeat warms every arm up)
                for a, fn in arms.items():
                    n = 3 if a == "lm_head_entry" else INNER
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(n):
                        fn()
                    e1.record()
                    e1.synchronize()
                    if rep:
                        times[a].append(e0.elapsed_time(e1) * 1e3 / n)
            rec = {a: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2),
                       "max_us": round(max(v), 2)} for a, v in times.items()}
            out[f"V{V}_rows{R}"] = rec
            print(V, R, {a: r["median_us"] for a, r in rec.items()}, flush=True)
        del E
    update_json(ROOT / "profiles" / "sample_wide.json", lambda doc: doc.update(
        {"what": __doc__.split("\n\n")[0], "unit": "us per launch", "repeats": REPEATS,
         "inner": INNER, "hidden": HIDDEN, "results": out}))


if __name__ == "__main__":
    main()
