"""lm_head_logprobs (csrc/lm_head.hip): the LM head with the log-softmax
epilogue against lm_head's own logits of the same x and E.

Exact: the target logit and the row maximum in `stats` are lm_head's logits
bit for bit (the same MFMA sequence), and logprob is (x_t - m) - lse recomputed
in float32 from `stats`.  Against float64: lse = log(sum exp(x - m) + 1e-6) and
the log-probability within KTOL = 1e-5 + 1e-6 |ref| (test_beam_select_gpu.py's
bound for the same fp32 arithmetic).

Shapes: V 1000 and 50257 (no multiple of 16: a partial last tile and a short
last workgroup) at K 64, V 1000 at K 320 (crosses the 256-wide chunk with a
tail); M 1 / 16 / 17 / 33 / 65 / 130: every row-tile form, a partial row block
and grid.y > 1.  Rows: ordinary spread, one logit ~60 above the rest (s rounds
to 1), all logits equal (s = V).  Targets: id 0, V - 1, an id in the last
partial tile, -1 and V (ignore indices), random ids."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PEAK = 62.0


def ktol(ref):
    return 1e-5 + 1e-6 * np.abs(ref)


_E = {}


def _embedding(V, K):
    """E fp16 [V][K]: small random rows, and row V // 2 a +-1 pattern (the peak
    rows' direction)."""
    if (V, K) not in _E:
        rng = np.random.default_rng(1000 * K + V)
        E = (0.05 * rng.standard_normal((V, K))).astype(np.float16)
        E[V // 2] = rng.choice([-1.0, 1.0], K).astype(np.float16)
        _E[(V, K)] = E
    return _E[(V, K)]


def _rows(E, kinds, seed):
    V, K = E.shape
    rng = np.random.default_rng(seed)
    e = E[V // 2].astype(np.float64)
    x = np.zeros((len(kinds), K), np.float32)
    for r, kind in enumerate(kinds):
        if kind == "ordinary":  # logits of spread ~1.2 sqrt(K / 64), none singled out
            v = 3.0 * rng.standard_normal(K)
            x[r] = v - (v @ e) / (e @ e) * e
        elif kind == "peak":  # logit V // 2 = 62, the others |.| < ~2
            x[r] = PEAK / K * e
        # "equal": x = 0, every logit 0
    return x


def _targets(V, M, seed):
    rng = np.random.default_rng(seed)
    fixed = [0, 0, V - 1, V - 2, -1, V // 2, V]  # V - 2: in the last partial tile, not its end
    t = rng.integers(0, V, M)
    t[:min(M, len(fixed))] = fixed[:M]
    return t.astype(np.int32)


def _check(x, E, targets):
    import torch
    import llm_capi
    V = E.shape[0]
    dx = torch.from_numpy(x).cuda()
    dE = torch.from_numpy(E).cuda()
    dt = torch.from_numpy(targets).cuda()
    lg = llm_capi.lm_head(dx, dE).cpu().numpy()
    lp, stats = llm_capi.lm_head_logprobs(dx, dE, dt)
    lp2, stats2 = llm_capi.lm_head_logprobs(dx, dE, dt)
    torch.cuda.synchronize()
    lp, stats = lp.cpu().numpy(), stats.cpu().numpy()
    assert np.array_equal(lp2.cpu().numpy().view(np.uint32), lp.view(np.uint32)), "two runs differ"
    assert np.array_equal(stats2.cpu().numpy().view(np.uint32), stats.view(np.uint32))
    lp_only, none = llm_capi.lm_head_logprobs(dx, dE, dt, want_stats=False)
    assert none is None and np.array_equal(lp_only.cpu().numpy().view(np.uint32), lp.view(np.uint32))

    valid = (targets >= 0) & (targets < V)
    rows = np.arange(len(targets))
    xt = np.where(valid, lg[rows, np.where(valid, targets, 0)], np.float32(0))
    # exact: lm_head's logits bit for bit
    assert np.array_equal(stats[:, 2], xt), "target logit"
    assert np.array_equal(stats[:, 0], lg.max(axis=1)), "row maximum"
    re = (stats[:, 2] - stats[:, 0]) - stats[:, 1]  # float32
    assert re.dtype == np.float32
    assert np.array_equal(lp[valid], re[valid]), "logprob from stats"
    assert (lp[~valid] == 0).all() and (stats[~valid, 2] == 0).all(), "ignore index"
    # float64
    l64 = lg.astype(np.float64)
    m = l64.max(axis=1)
    lse = np.log(np.exp(l64 - m[:, None]).sum(axis=1) + 1e-6)
    err = np.abs(stats[:, 1] - lse)
    print("lse err / tol", (err / ktol(lse)).max())
    assert (err <= ktol(lse)).all(), (err.max(), (err / ktol(lse)).max())
    ref = (xt.astype(np.float64) - m) - lse
    err = np.abs(lp - ref)[valid]
    print("logprob err / tol", (err / ktol(ref[valid])).max() if valid.any() else 0.0)
    assert (err <= ktol(ref[valid])).all(), (err.max(), (err / ktol(ref[valid])).max())
    return lg, lp, stats


@pytest.mark.parametrize("M", [1, 16, 17, 33, 65, 130])
@pytest.mark.parametrize("V,K", [(1000, 64), (50257, 64), (1000, 320)])
def test_lm_head_logprobs(gpu, V, K, M):
    E = _embedding(V, K)
    if M == 1:  # one row per launch: each kind in turn, each with a target of its own
        for i, (kind, t) in enumerate([("ordinary", V - 2), ("peak", V // 2), ("equal", V - 1),
                                       ("ordinary", -1), ("peak", 0)]):
            lg, lp, stats = _check(_rows(E, [kind], 7 + i), E, np.array([t], np.int32))
        return
    kinds = ["ordinary", "peak", "equal"] + ["ordinary"] * (M - 5) + ["peak", "equal"]
    x = _rows(E, kinds, 100 * M + K)
    targets = _targets(V, M, M)
    targets[1] = 0          # a peak row scored away from its peak: about -62
    targets[M - 2] = V // 2  # a peak row scored at its peak: about 0
    lg, lp, stats = _check(x, E, targets)
    # the planted rows are what they were planted for
    assert (lg[2] == 0).all() and abs(stats[2, 1] - np.log(V)) < 1e-5  # s = V
    top2 = np.sort(lg[1])[-2:]
    assert top2[1] - top2[0] > 55 and abs(stats[1, 1]) < 2e-6  # s rounds to 1: lse ~ log(1 + 1e-6)
    assert lp[1] < -55 and abs(lp[M - 2]) < 1e-5
