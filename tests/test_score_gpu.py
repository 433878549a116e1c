"""llm_decoder_score: teacher-forced log-probabilities through the prefill
passes and the LM head's log-softmax epilogue.

Dims of test_serve_gpu.py (L 2 / H 4 / D 64, V 300, max_seq 640, max_batch 4).
Seven sequences of lengths [1, 2, 17, 33, 40, 5, 531]: more sequences than
rows (two groups), the 531-token one crosses the 512-token pass boundary (its
last targets belong to the next pass), length 1 gives an empty result.

fp16 weights: every value against the float64 log-softmax (lse = log(sum exp(x
- m) + 1e-6)) of OracleDecoder's logits row at that position.  Log-sum-exp is
1-Lipschitz in the sup norm, so logits rows within d = tol * max|ref row| of
each other give log-probabilities within 2 d: the bound is 2 * LOGIT_TOL *
max|row| + KTOL.  INT8 weights (plain, LLM_FP8 pages, rope + window 32, packed
prefill): against a one-row decoder of the same configuration teacher-forced
by `step`, 2 * FREE_RUN_TOL * max|row| + KTOL -- that pair of paths' own bar in
test_serve_gpu.py.  With packed prefill off the passes of a sequence do not
depend on its neighbours: scoring the seven together equals scoring each
alone, bit for bit."""
import numpy as np
import pytest

from test_decoder_gpu import FREE_RUN_TOL, LOGIT_TOL
from test_serve_gpu import MAXB, S, V, _kv, _make, _prompts, f16_weights, int8_weights  # noqa: F401

pytestmark = pytest.mark.gpu

LENS = [1, 2, 17, 33, 40, 5, 531]


def ktol(ref):
    return 1e-5 + 1e-6 * np.abs(ref)


def _logprob64(row, t):
    x = row.astype(np.float64)
    m = x.max()
    return (x[t] - m) - np.log(np.exp(x - m).sum() + 1e-6)


def _check(got, seqs, rows_of, tol, what):
    """got: score()'s arrays; rows_of(seq): the reference logits row at every
    position of seq[:-1]."""
    worst = 0.0
    assert len(got) == len(seqs)
    for s, (g, seq) in enumerate(zip(got, seqs)):
        assert g.dtype == np.float32 and g.shape == (len(seq) - 1,)
        if len(seq) == 1:
            continue
        rows = rows_of(seq)
        for i in range(1, len(seq)):
            ref = _logprob64(rows[i - 1], seq[i])
            bound = 2 * tol * np.abs(rows[i - 1]).max() + ktol(ref)
            err = abs(float(g[i - 1]) - ref)
            worst = max(worst, err / bound)
            assert err <= bound, (what, s, i, err, bound)
    print(f"score {what}: worst err / bound {worst:.3f}")


def test_score_f16_oracle(gpu, f16_weights, oracle):
    from oracle.oracle import OracleDecoder
    dec = _make(f16_weights, MAXB)
    seqs = _prompts(LENS, seed=41)

    def rows_of(seq):
        od = OracleDecoder(oracle, f16_weights, 1)
        return [od.step(np.array([t], np.int32), np.array([i], np.int32))[1][0].copy()
                for i, t in enumerate(seq[:-1])]

    _check(dec.score(seqs), seqs, rows_of, LOGIT_TOL, "f16")


def _solo_rows(solo):
    import torch
    lg = torch.empty((1, V), device="cuda")

    def rows_of(seq):
        solo.begin_synthetic(1, 0, 0, False)
        out = []
        for t in seq[:-1]:
            solo.step([t], logits_ptr=lg.data_ptr())
            torch.cuda.synchronize()
            out.append(lg[0].cpu().numpy().copy())
        return out
    return rows_of


@pytest.mark.parametrize("cfg", [dict(), dict(kv_dtype="fp8"), dict(rope=True, window=32),
                                 dict(packed=True)],
                         ids=["int8", "int8_fp8kv", "int8_rope_window32", "int8_packed_prefill"])
def test_score_int8_solo(gpu, int8_weights, cfg):
    dec = _make(int8_weights, MAXB, **cfg)
    seqs = _prompts(LENS, seed=42)
    got = dec.score(seqs)
    solo_cfg = {k: v for k, v in cfg.items() if k != "packed"}
    _check(got, seqs, _solo_rows(_make(int8_weights, 1, **solo_cfg)), FREE_RUN_TOL, str(cfg))
    kv = _kv(dec)
    assert kv["free"] == kv["pages"]


def test_score_exact_state_and_refusals(gpu, int8_weights):
    dec = _make(int8_weights, MAXB)
    seqs = _prompts(LENS, seed=43)
    prompt = seqs[3][:9]
    before = dec.generate(prompt, 6)
    together = dec.score(seqs)
    # state: no rows active, every page free, generate undisturbed
    assert dec.context_len(0) == -1
    kv = _kv(dec)
    assert kv["free"] == kv["pages"]
    assert dec.generate(prompt, 6) == before
    # exactness (packed prefill off): together == each alone == a second call
    assert together[0].shape == (0,)
    for s, seq in enumerate(seqs):
        alone = dec.score([seq])[0]
        assert np.array_equal(alone.view(np.uint32), together[s].view(np.uint32)), s
    again = dec.score(seqs)
    for a, b in zip(again, together):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert dec.score([]) == []
    # refusals, nothing run
    for bad in ([seqs[2], []], [seqs[2][:5] + [V]], [[1] * (S + 1)]):
        with pytest.raises(RuntimeError, match="llm_decoder_score"):
            dec.score(bad)
    assert len(dec.score([[1] * S])[0]) == S - 1  # len - 1 = S - 1 < S: the longest allowed
    dec.serve_begin()
    with pytest.raises(RuntimeError, match="serving"):
        dec.score(seqs[:2])
    dec.serve_end()
    assert dec.context_len(0) == -1 and _kv(dec)["free"] == kv["pages"]
    assert dec.generate(prompt, 6) == before
