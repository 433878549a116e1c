"""The streaming token-choice kernels (csrc/sample_wide.hip) through
sample_rows_wide / sample_rows_each_wide / logprob_rows_wide.

Sampler: every row against oracle.sample_rows (float64 sums) run on that row
alone; where the oracle's draw lies within 1e-4 (relative) of a CDF boundary
the device may return the token on either side of it (test_sample_each_gpu.py's
allowance), for at most 2 of a vocabulary's 24 sampled draws.  The oracle alone
puts 0, 0, 0, 1, 1 of them that close at V 1000, 2049, 65537, 100003, 262144,
so no generator seed had to change.  V 1000 is less than one 2,048-token tile,
2049 and 65537 end a tile with one token, 100003 rows start at every 16-byte
misalignment, 262144 is the largest vocabulary in use.

Log-probabilities: tests/test_logprob_rows_gpu.py's rows, float64 reference
and tolerance (KTOL), at vocabularies on both sides of the old bound."""
import numpy as np
import pytest

import llm_capi
from test_logprob_rows_gpu import ROWS, _case, _close

pytestmark = pytest.mark.gpu

#            temperature, top_k, top_p
SETTINGS = [(0.0, 0, 1.0), (1.0, 1, 1.0), (0.7, 40, 1.0), (1.0, 0, 0.9), (1.3, 0, 1.0),
            (1.0, 5, 0.5), (1.0, 0, 1.0), (0.9, 1000, 0.95)]
COUNTERS = [0, 3, 17, 600]


def _oracle_ok(got, row, T, k, p, seed, ctr):
    """(token accepted, allowance used) for one row against the oracle."""
    from oracle.oracle import sample_rows
    ref, margin, near = sample_rows(row[None], T, k, p, seed=seed, counter=ctr, neighbours=True)
    if got == ref[0]:
        return True, False
    return bool(margin[0] < 1e-4 and got in near[0]), True


def _each(logits, order, ctr):
    import torch
    dev = lambda a, dt: torch.from_numpy(np.array(a, dt)).cuda()
    t = dev([SETTINGS[i][0] for i in order], np.float32)
    k = dev([SETTINGS[i][1] for i in order], np.int32)
    p = dev([SETTINGS[i][2] for i in order], np.float32)
    s = dev([11 + i for i in order], np.int64)
    c = dev([ctr] * len(order), np.int32)
    out = llm_capi.sample_rows_each(torch.from_numpy(logits[order]).cuda(), t, k, p, s, c,
                                    wide=True)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("V", [1000, 2049, 65537, 100003, 262144])
def test_sampler_against_the_oracle(gpu, V):
    logits = (6.0 * np.random.default_rng(V).standard_normal((8, V))).astype(np.float32)
    logits[0, [7, V - 1]] = logits[0].max() + 1  # a tied maximum: the first wins
    rows = list(range(8))
    allowed = 0
    for ctr in COUNTERS:
        got = _each(logits, rows, ctr)
        for r, (T, k, p) in enumerate(SETTINGS):
            ok, used = _oracle_ok(got[r], logits[r], T, k, p, 11 + r, ctr)
            assert ok, (V, ctr, r, got[r])
            allowed += used
        assert got[0] == 7 and got[1] == int(np.argmax(logits[1]))
        if ctr == 17:
            order = [4, 7, 0, 5, 2, 6, 1, 3]
            np.testing.assert_array_equal(_each(logits, order, ctr), got[order])
            np.testing.assert_array_equal(_each(logits, rows, ctr), got)
    assert allowed <= 2, (V, allowed)


def test_degenerate_rows(gpu):
    import torch
    V = 65537
    one = lambda lg, **kw: int(llm_capi.sample_rows(torch.from_numpy(lg).cuda(), wide=True,
                                                    **kw).cpu()[0])
    flat = np.full((1, V), 1.25, np.float32)  # one histogram bin holds all V: the list overflows
    for kw in (dict(top_k=10), dict(top_p=0.5)):
        for ctr in (0, 5):
            got = one(flat, seed=3, counter=ctr, **kw)
            ok, _ = _oracle_ok(got, flat[0], 1.0, kw.get("top_k", 0), kw.get("top_p", 1.0), 3, ctr)
            assert ok, (kw, ctr, got)
    live = np.full((1, V), -np.inf, np.float32)
    live[0, [12, 40000, V - 1]] = 0.0
    seen = set()
    for ctr in range(6):
        got = one(live, seed=9, counter=ctr)
        ok, _ = _oracle_ok(got, live[0], 1.0, 0, 1.0, 9, ctr)
        assert ok and got in (12, 40000, V - 1), (ctr, got)
        seen.add(got)
    assert len(seen) > 1
    assert one(np.full((1, V), -np.inf, np.float32), seed=1) == 0


@pytest.mark.parametrize("top_n", [0, 1, 8])
@pytest.mark.parametrize("V", [17, 2049, 65537, 262144])
def test_logprob_rows_wide(gpu, V, top_n):
    import torch
    lg, m, lse, order = _case(V)
    dl = torch.from_numpy(lg).cuda()
    ch = np.array([order[0, 0], V - 1, int(np.flatnonzero(np.isinf(lg[2]))[0]), -1, V], np.int32)
    dch = torch.from_numpy(ch).cuda()
    clp, tlp, tid, stats = [x.cpu().numpy() for x in llm_capi.logprob_rows(dl, dch, top_n,
                                                                           wide=True)]
    assert np.array_equal(stats[:, 0], lg.max(axis=1)), "m is the row maximum"
    assert _close(stats[:, 1], lse), (stats[:, 1], lse)
    assert np.array_equal(tid, order[:, :top_n]), (tid, order[:, :top_n])
    rows = np.arange(ROWS)[:, None]
    l64 = lg.astype(np.float64)
    assert _close(tlp, (l64[rows, order[:, :top_n]] - m[:, None]) - lse[:, None])
    assert _close(clp[:3], (l64[np.arange(3), ch[:3]] - m[:3]) - lse[:3])
    assert clp[2] == -np.inf and (clp[3:] == 0).all()
    if V <= 65536:  # the row-holding kernel on the same input
        clp0, tlp0, tid0, stats0 = [x.cpu().numpy() for x in llm_capi.logprob_rows(dl, dch, top_n)]
        assert np.array_equal(tid0, tid)
        assert _close(tlp, tlp0.astype(np.float64)) and _close(stats[:, 1], stats0[:, 1])
