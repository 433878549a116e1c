"""sample_rows_each: sample_rows with every row's own settings in one launch
(the token choice of a serving step).  V 1000 and 50257 are the 16- and
128-values-per-thread instantiations of the kernel (the second keeps most of
the row in LDS).  Six rows cover both greedy forms and every filter
combination; each row must equal the oracle sampler run on that row alone
with the row's seed and counter (the draw's row term is 0), so a row's token
cannot depend on its place in the launch.  Where the oracle's draw lies
within 1e-4 (relative) of a CDF boundary the device may return the token on
either side of it -- test_decoder_device_sampling's allowance.
"""
import numpy as np
import pytest

import llm_capi

pytestmark = pytest.mark.gpu

#            temperature, top_k, top_p
SETTINGS = [(0.0, 0, 1.0), (1.0, 1, 1.0), (0.7, 40, 1.0), (1.0, 0, 0.9), (1.3, 0, 1.0),
            (1.0, 5, 0.5)]
SEEDS = [11, 2 ** 63 + 5, 77, 123456789012345, 0, 2 ** 64 - 1]
COUNTERS = [0, 3, 17, 600, 1, 8191]


def _torch():
    import torch
    return torch


def _device_args(order):
    torch = _torch()
    t = torch.tensor([SETTINGS[i][0] for i in order], dtype=torch.float32, device="cuda")
    k = torch.tensor([SETTINGS[i][1] for i in order], dtype=torch.int32, device="cuda")
    p = torch.tensor([SETTINGS[i][2] for i in order], dtype=torch.float32, device="cuda")
    s = torch.from_numpy(np.array([SEEDS[i] for i in order], np.uint64).view(np.int64)).cuda()
    c = torch.tensor([COUNTERS[i] for i in order], dtype=torch.int32, device="cuda")
    return t, k, p, s, c


@pytest.fixture(scope="module", params=[1000, 50257])
def case(request, gpu):
    """(V, logits [6][V] on the host, the device's ids in row order)."""
    torch = _torch()
    V = request.param
    rng = np.random.default_rng(V)
    logits = (3.0 * rng.standard_normal((6, V))).astype(np.float32)
    logits[0, [7, V - 1]] = logits[0].max() + 1  # a tied maximum: the first wins
    out = llm_capi.sample_rows_each(torch.from_numpy(logits).cuda(), *_device_args(range(6)))
    torch.cuda.synchronize()
    return V, logits, out.cpu().numpy()


def test_each_row_equals_the_oracle_on_that_row(case):
    from oracle.oracle import sample_rows
    V, logits, got = case
    for r, ((T, k, p), seed, ctr) in enumerate(zip(SETTINGS, SEEDS, COUNTERS)):
        ref, margin, near = sample_rows(logits[r:r + 1], T, k, p, seed=seed, counter=ctr,
                                        neighbours=True)
        ok = got[r] == ref[0] or (margin[0] < 1e-4 and got[r] in near[0])
        assert ok, (V, r, got[r], ref[0], margin[0], near[0])
    assert got[0] == 7  # the greedy rows: first maximum
    assert got[1] == int(np.argmax(logits[1]))


def test_permuted_rows_permute_the_output(case):
    torch = _torch()
    V, logits, got = case
    order = [4, 0, 5, 2, 1, 3]
    out = llm_capi.sample_rows_each(torch.from_numpy(logits[order]).cuda(), *_device_args(order))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), got[order])


def test_null_arrays_are_sample_rows(case):
    """Every array NULL: the scalars' path, sample_rows(T 1, no filter, seed 0,
    counter 0) bit for bit (the draw keeps its row term)."""
    torch = _torch()
    V, logits, _ = case
    lg = torch.from_numpy(logits).cuda()
    a = llm_capi.sample_rows_each(lg)
    b = llm_capi.sample_rows(lg, 1.0, 0, 1.0, seed=0, counter=0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    # ... and only some NULL: rows by their counters, the scalars for the rest
    c = _device_args(range(6))[4]
    m = llm_capi.sample_rows_each(lg, counter=c).cpu().numpy()
    for r in range(6):
        one = llm_capi.sample_rows(lg, 1.0, 0, 1.0, seed=0, counter=COUNTERS[r]).cpu().numpy()
        assert m[r] == one[r], (V, r)
