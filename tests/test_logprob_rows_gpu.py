"""logprob_rows (csrc/logprobs.hip): chosen and top-n log-probabilities of
materialised logits rows against numpy.

Ids exactly: the top_n largest raw logits by a stable sort on (logit
descending, id ascending).  Values against float64, lse = log(sum exp(x - m) +
1e-6) and logprob(t) = (x_t - m) - lse, within KTOL = 1e-5 + 1e-6 |ref|
(test_beam_select_gpu.py's bound for the same fp32 arithmetic); m exactly.

Five rows: ordinary, duplicated top values (the lower id first), -inf entries
(so many at V = 17 that the top 8 reach into them: they keep their id order),
a wide spread, all equal.  V 17 / 1000 / 50257 / 65536: every values-per-thread
form of the row kernels, the last one full."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = 5


def ktol(ref):
    return 1e-5 + 1e-6 * np.abs(ref)


def _close(a, ref):
    """a within KTOL of ref; infinities must agree exactly."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    inf = np.isinf(ref)
    ok = np.where(inf, a == ref, np.abs(a - np.where(inf, 0, ref)) <= ktol(np.where(inf, 0, ref)))
    return bool(ok.all())


_CASE = {}


def _case(V):
    """(logits fp32 [5][V], float64 m, lse, sorted ids [5][V]) -- computed once per V."""
    if V not in _CASE:
        rng = np.random.default_rng(V)
        lg = (2.0 * rng.standard_normal((ROWS, V))).astype(np.float32)
        # row 1: the maximum three times and another value twice
        a = np.sort(rng.choice(V, 5, replace=False))
        lg[1, a[[0, 2, 4]]] = lg[1].max() + np.float32(1.5)
        lg[1, a[[1, 3]]] = lg[1].max() - np.float32(0.25)
        # row 2: -inf everywhere but at 5 ids (V 17) or on ~70 % of the ids
        keep = rng.choice(V, 5, replace=False) if V < 100 else np.flatnonzero(rng.random(V) < 0.3)
        mask = np.ones(V, bool)
        mask[keep] = False
        lg[2, mask] = -np.inf
        lg[3] *= np.float32(8.0)
        lg[4] = np.float32(rng.standard_normal())
        l64 = lg.astype(np.float64)
        m = l64.max(axis=1)
        lse = np.log(np.exp(l64 - m[:, None]).sum(axis=1) + 1e-6)
        ids = np.arange(V)
        order = np.stack([np.lexsort((ids, -l64[r])) for r in range(ROWS)])
        _CASE[V] = lg, m, lse, order
    return _CASE[V]


@pytest.mark.parametrize("chosen", ["null", "given"])
@pytest.mark.parametrize("top_n", [0, 1, 8])
@pytest.mark.parametrize("V", [17, 1000, 50257, 65536])
def test_logprob_rows(gpu, V, top_n, chosen):
    import torch
    import llm_capi
    lg, m, lse, order = _case(V)
    dl = torch.from_numpy(lg).cuda()
    ch = None
    if chosen == "given":
        # the argmax, the last id, a -inf entry, and two ignore indices (-1, V)
        ch = np.array([order[0, 0], V - 1, int(np.flatnonzero(np.isinf(lg[2]))[0]), -1, V], np.int32)
    dch = torch.from_numpy(ch).cuda() if ch is not None else None
    clp, tlp, tid, stats = llm_capi.logprob_rows(dl, dch, top_n)
    clp2, tlp2, tid2, stats2 = llm_capi.logprob_rows(dl, dch, top_n)
    torch.cuda.synchronize()
    tlp, tid, stats = tlp.cpu().numpy(), tid.cpu().numpy(), stats.cpu().numpy()
    assert np.array_equal(tid2.cpu().numpy(), tid)
    assert np.array_equal(tlp2.cpu().numpy().view(np.uint32), tlp.view(np.uint32))
    assert np.array_equal(stats2.cpu().numpy().view(np.uint32), stats.view(np.uint32))

    assert np.array_equal(stats[:, 0], lg.max(axis=1)), "m is the row maximum"
    assert _close(stats[:, 1], lse), (stats[:, 1], lse)
    assert tid.shape == (ROWS, top_n) and tlp.shape == (ROWS, top_n)
    assert np.array_equal(tid, order[:, :top_n]), (tid, order[:, :top_n])
    rows = np.arange(ROWS)[:, None]
    ref = (lg.astype(np.float64)[rows, order[:, :top_n]] - m[:, None]) - lse[:, None]
    assert _close(tlp, ref), (tlp, ref)
    if top_n == 8:
        assert list(tid[1, :3]) == sorted(tid[1, :3]) and tlp[1, 0] == tlp[1, 2], "planted ties"
        assert list(tid[4]) == list(range(8)), "equal logits: ids ascend from 0"
        if V == 17:
            assert np.isinf(tlp[2, 5:]).all() and list(tid[2, 5:]) == sorted(tid[2, 5:])
    if ch is None:
        assert clp is None
    else:
        clp = clp.cpu().numpy()
        assert np.array_equal(clp2.cpu().numpy().view(np.uint32), clp.view(np.uint32))
        cref = (lg.astype(np.float64)[np.arange(3), ch[:3]] - m[:3]) - lse[:3]
        assert _close(clp[:3], cref), (clp, cref)
        assert clp[2] == -np.inf
        assert (clp[3:] == 0).all(), "ignore indices write 0"
        if top_n >= 1:  # the argmax as chosen id: the same bits as the top entry
            assert clp[0] == tlp[0, 0]
    # no stats wanted: the same results
    _, tlp3, tid3, none = llm_capi.logprob_rows(dl, dch, top_n, want_stats=False)
    assert none is None and np.array_equal(tid3.cpu().numpy(), tid)
