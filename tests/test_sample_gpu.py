"""Device token sampling (csrc/sample.hip) at every instantiation and edge.

launch_sample_rows picks tokens-per-thread 16 / 32 / 64 / 128 from V; the
suites below run all four against the numpy restatement (oracle.sample_rows)
and against properties that hold for any correct inverse-CDF draw: a drawn
token is always in the float64 keep set, the thread claims tile [0, Z) (no draw
falls to the token-0 fallback), ties and bans behave as documented."""
import numpy as np
import pytest

import _sample_scan as scan

gpu_test = pytest.mark.gpu

SETTINGS = [(0.0, 0, 1.0), (1.0, 1, 1.0), (1.0, 0, 1.0), (0.7, 50, 1.0), (1.2, 0, 0.9),
            (1.0, 20, 0.8), (0.5, 0, 0.5)]
# one V per instantiation (tokens per thread 16, 32, 64, 128), none a multiple of 16
EDGE_V = [1003, 12005, 32003, 50257]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sample(logits_dev, T=1.0, k=0, p=1.0, seed=0, counter=0):
    import llm_capi
    return llm_capi.sample_rows(logits_dev, T, k, p, seed=seed, counter=counter).cpu().numpy()


def _draws(logits_row, rows, counters, **kw):
    """Tokens of `rows` identical rows (the row id varies the draw) x counters."""
    d = _dev(np.tile(np.asarray(logits_row, np.float32), (rows, 1)))
    return np.concatenate([_sample(d, counter=c, **kw) for c in counters])


# ---------------------------------------------------------------------------
# A1: draws aimed at the seams between two threads' claims
# ---------------------------------------------------------------------------
GAP_V, GAP_SEED = 8192, 5


def _gap_case():
    banned = np.concatenate([[0], np.random.default_rng(5).choice(np.arange(1, GAP_V), 3000,
                                                                  replace=False)])
    logits = scan.banned_row(GAP_V, banned)
    return logits, scan.find_draws(GAP_SEED, scan.claim_gaps(logits))


@pytest.fixture(scope="module")
def gap_case():
    return _gap_case()


def test_gap_draw_search(gap_case):
    """The host model finds draws that land between two threads' claims (CPU
    only; the device test below does not depend on the model being right)."""
    logits, hits = gap_case
    assert int((logits == 0).sum()) == 5191
    assert len(hits) >= 20, len(hits)
    assert hits[0][:2] == (0, 120853), hits[0]


@gpu_test
def test_sample_rows_claims_tile_the_cdf(gpu, gap_case):
    """Rows of 0 / -inf logits (probabilities bit-determined: expf(0) = 1, the
    sum an exact integer), T = 1, no filter, at draws whose target sits on the
    seam between two threads' partial sums.  Whatever the fp32 association,
    the token is unbanned and is one of the two unbanned tokens on either side
    of the float64 CDF position of u.  (A claim rule `lo <= target < lo + part`
    leaves such targets unclaimed and returns the banned token 0.)"""
    logits, hits = gap_case
    kept = np.nonzero(logits == 0)[0]
    K = len(kept)
    bad = []
    d = _dev(np.tile(logits, (4, 1)))
    for row, counter, ui in hits:
        got = int(_sample(d[:row + 1], seed=GAP_SEED, counter=counter)[row])
        x = ui / 2.0 ** 24 * K  # float64 CDF position in units of one kept token
        b = int(round(x))       # nearest token boundary: between kept[b - 1] and kept[b]
        allowed = {int(kept[min(max(b - 1, 0), K - 1)]), int(kept[min(b, K - 1)])}
        assert int(kept[min(int(x), K - 1)]) in allowed
        if logits[got] != 0 or got not in allowed:
            bad.append((row, counter, got, sorted(allowed)))
    assert not bad, f"{len(bad)} of {len(hits)} seam draws wrong (row, counter, got, allowed): {bad[:8]}"


# ---------------------------------------------------------------------------
# A3: bulk invariant -- every drawn token is in the float64 keep set
# ---------------------------------------------------------------------------
BULK_V = 8192
# (logit, count) by descending probability; the rest of the vocabulary is the
# lowest level (token 0 in it), and 100 tokens are banned (-inf)
BULK_LEVELS = [(6.0, 20), (5.0, 30), (2.0, 950)]
BULK_LOW, BULK_BANNED = -3.0, 100


def _bulk_row():
    rng = np.random.default_rng(11)
    order = 1 + rng.permutation(BULK_V - 1)  # token 0 stays in the lowest level
    lg = np.full(BULK_V, BULK_LOW, np.float32)
    groups, at = [], 0
    for level, n in BULK_LEVELS:
        lg[order[at:at + n]] = level
        groups.append(order[at:at + n])
        at += n
    lg[order[at:at + BULK_BANNED]] = -np.inf
    low = np.nonzero(lg == np.float32(BULK_LOW))[0]
    assert 0 in low
    groups.append(low)
    return lg, groups


def _bulk_keep(lg, groups, T, k, p):
    """Float64 keep set of the documented filter on grouped (tied) probabilities;
    asserts that it is unambiguous: k on a group boundary, top_p at least 1e-3
    of the total mass away from every group-boundary cumulative mass."""
    levels = np.array([float(lg[g[0]]) for g in groups])
    sizes = np.array([len(g) for g in groups])
    mass = sizes * np.exp((levels - levels.max()) / T)
    cum = np.cumsum(mass) / mass.sum()  # cumulative mass at each group boundary
    above = np.concatenate([[0.0], cum[:-1]])  # mass strictly above each group
    keep = np.ones(len(groups), bool)
    if 0 < k < BULK_V:
        assert k in np.cumsum(sizes), "top_k must sit on a group boundary"
        keep &= np.cumsum(sizes) <= k  # all tokens equal to the k-th probability are kept
    if p < 1.0:
        assert np.abs(cum - p).min() >= 1e-3, (cum, p)
        keep &= above < p
    assert keep.any()
    mask = np.zeros(BULK_V, bool)
    for g, kp in zip(groups, keep):
        mask[g] = kp
    return mask


@gpu_test
@pytest.mark.parametrize("T,k,p", [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.2, 0, 0.9), (1.0, 20, 0.8)])
def test_sample_rows_bulk_keep_set(gpu, T, k, p):
    """65 536 draws (4096 identical rows x 16 counters) of a row whose
    probabilities tie in groups: every drawn token is in the float64 keep set
    (never a banned token, never a filtered one, never the fallback token 0
    unless it is kept)."""
    import torch
    import llm_capi
    lg, groups = _bulk_row()
    mask = _bulk_keep(lg, groups, T, k, p)
    assert mask[0] == (k == 0 and p == 1.0)  # token 0 is kept only without a filter
    d = _dev(lg).unsqueeze(0).expand(4096, BULK_V).contiguous()
    toks = torch.stack([llm_capi.sample_rows(d, T, k, p, seed=31, counter=c)
                        for c in range(16)]).cpu().numpy().ravel()
    assert toks.min() >= 0 and toks.max() < BULK_V
    out = toks[~mask[toks]]
    assert out.size == 0, (out.size, np.unique(out)[:10])
    # the draws spread: far more distinct tokens than any one thread's chunk
    assert len(np.unique(toks)) > min(int(mask.sum()), 1000) // 2


# ---------------------------------------------------------------------------
# A4: every instantiation against the numpy restatement
# ---------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("V", [1, 2, 1000, 8192, 8193, 16384, 16385, 32000, 32768, 32769, 65536])
@pytest.mark.parametrize("T,k,p", SETTINGS)
def test_sample_rows_every_vpt_vs_oracle(gpu, V, T, k, p):
    """Same token as oracle.sample_rows per row; where the draw lands within
    1e-4 of a CDF boundary, one of the two kept tokens beside that boundary."""
    from oracle.oracle import sample_rows
    rng = np.random.default_rng(V + int(T * 10) + k)
    logits = (rng.standard_normal((6, V)) * 3).astype(np.float32)
    d = _dev(logits)
    for counter in (0, 1, 17):
        got = _sample(d, T, k, p, seed=5, counter=counter)
        ref, margin, near = sample_rows(logits, T, k, p, seed=5, counter=counter, neighbours=True)
        ok = (got == ref) | ((margin < 1e-4) & ((got == near[:, 0]) | (got == near[:, 1])))
        assert ok.all(), (counter, got, ref, margin, near)
        if T > 0 and k > 1:  # the token is within the top-k
            for r in range(6):
                assert logits[r, got[r]] >= np.sort(logits[r])[-min(k, V)]


@gpu_test
def test_sample_rows_refuses_v_over_65536(gpu):
    import torch
    import llm_capi
    lib = llm_capi.load()
    V = 65537
    logits = torch.zeros((2, V), device="cuda")
    out = torch.full((2,), -77, dtype=torch.int32, device="cuda")
    st = lib.sample_rows(llm_capi.ptr(logits), 2, V, 1.0, 0, 1.0, 5, 0, llm_capi.ptr(out),
                         llm_capi.stream_ptr())
    torch.cuda.synchronize()
    assert st in (llm_capi.LLM_ERR_INVALID, llm_capi.LLM_ERR_UNSUPPORTED, llm_capi.LLM_ERR_RANGE), st
    assert b"65536" in lib.llm_last_error()
    assert out.cpu().tolist() == [-77, -77]


# ---------------------------------------------------------------------------
# A5: edges, at one V per instantiation
# ---------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("V", EDGE_V)
def test_sample_rows_bans(gpu, V):
    """-inf logits are never drawn, under no filter, top-k and top-p alike."""
    rng = np.random.default_rng(V)
    lg = rng.standard_normal(V).astype(np.float32)
    banned = rng.random(V) < 0.5
    banned[0] = True
    banned[V - 1] = False
    lg[banned] = -np.inf
    for kw in (dict(), dict(k=40), dict(p=0.9), dict(T=1.5, k=V - 1)):
        toks = _draws(lg, 256, range(4), seed=V, **kw)
        assert not banned[toks].any(), (kw, toks[banned[toks]][:8])
        assert len(np.unique(toks)) > 20


@gpu_test
@pytest.mark.parametrize("V", EDGE_V)
def test_sample_rows_spike(gpu, V):
    """One logit 1e4 above the rest (every other probability underflows to 0):
    that token always wins, wherever it sits."""
    rng = np.random.default_rng(V + 1)
    base = rng.standard_normal(V).astype(np.float32)
    for at in (0, V // 2 + 1, V - 1):
        lg = base.copy()
        lg[at] = 1e4
        for kw in (dict(), dict(k=5), dict(p=0.9), dict(T=0.7, k=3, p=0.5)):
            toks = _draws(lg, 32, (0, 9), seed=3, **kw)
            assert (toks == at).all(), (at, kw, np.unique(toks))


@gpu_test
@pytest.mark.parametrize("V", EDGE_V)
def test_sample_rows_low_temperature(gpu, V):
    """T = 0.01 with the top logit 2 above the runner-up: every other
    probability is exp(-200) = 0 in fp32, so the draw is the argmax."""
    rng = np.random.default_rng(V + 2)
    lg = (rng.standard_normal(V) * 3).astype(np.float32)
    top = int(rng.integers(V))
    lg[top] = lg.max() + 2.0
    for kw in (dict(), dict(k=10), dict(p=0.5)):
        toks = _draws(lg, 32, (0, 5), T=0.01, seed=8, **kw)
        assert (toks == top).all(), (kw, np.unique(toks))


@pytest.fixture(scope="module")
def low_draws():
    """Counters whose draw for (seed 21, row 0) is u < 0.25 / 65536: for any
    V <= 65536 the target lies well inside the first kept token's mass when
    the probabilities are within a factor 2 of uniform."""
    c = np.arange(1 << 22, dtype=np.uint64)
    ui = scan.uniform_index(21, 0, c)
    hits = np.nonzero(ui < (1 << 24) // (4 * 65536))[0][:6]
    assert len(hits) == 6
    return [int(h) for h in hits]


@gpu_test
@pytest.mark.parametrize("V", EDGE_V)
def test_sample_rows_top_k_near_v(gpu, V, low_draws):
    """Token 0 is the unique minimum (logit -0.5, every other 0), at draws whose
    target lies in the first kept token's mass: without a top-k, and with
    top_k >= V, that is token 0; top_k = V - 1 drops exactly token 0, and the
    first kept token is 1."""
    lg = np.zeros((1, V), np.float32)
    lg[0, 0] = -0.5
    d = _dev(lg)
    for c in low_draws:
        for k, want in ((0, 0), (V, 0), (V + 7, 0), (V - 1, 1)):
            got = int(_sample(d, 1.0, k, 1.0, seed=21, counter=c)[0])
            assert got == want, (c, k, got)


@gpu_test
@pytest.mark.parametrize("V", EDGE_V)
def test_sample_rows_top_p_keeps_tied_top(gpu, V):
    """top_p = 1e-6 keeps only the top token; with tied top tokens it keeps all
    of them (the mass strictly above each is 0) and nothing else, as does
    top_p = 0.5 when the tied tokens hold nearly all the mass."""
    rng = np.random.default_rng(V + 3)
    lg = rng.standard_normal(V).astype(np.float32)
    lg[V // 3] = lg.max() + 2.0
    toks = _draws(lg, 64, range(2), p=1e-6, seed=4)
    assert (toks == V // 3).all(), np.unique(toks)
    tied = np.array([1, V // 2, V - 2, V - 1])
    lg[tied] = 12.0
    for p in (1e-6, 0.5):
        toks = _draws(lg, 64, range(4), p=p, seed=4)
        assert set(toks.tolist()) == set(tied.tolist()), (p, np.unique(toks))


@gpu_test
@pytest.mark.parametrize("V", EDGE_V)
def test_sample_rows_last_token(gpu, V):
    """V is no multiple of 16: a kept token at index V - 1 (the last thread's
    partly filled chunk) is drawn, alone and beside token 0."""
    assert V % 16
    lg = np.full(V, -np.inf, np.float32)
    lg[V - 1] = 0.3
    toks = _draws(lg, 16, (0, 1), seed=6)
    assert (toks == V - 1).all(), np.unique(toks)
    lg[0] = 0.3
    toks = _draws(lg, 64, (0, 1), seed=6)
    assert set(toks.tolist()) == {0, V - 1}
    assert 32 < int((toks == V - 1).sum()) < 96  # 128 fair draws: 64 +- 5.7 sigma


@gpu_test
@pytest.mark.parametrize("V", EDGE_V)
@pytest.mark.parametrize("T,k", [(0.0, 0), (1.0, 1), (-1.0, 5)])
def test_sample_rows_greedy_ties(gpu, V, T, k):
    """Greedy: the first maximum wins across lanes, waves and chunks; a maximum
    at V - 1 is found; an all -inf row returns an id in [0, V)."""
    rng = np.random.default_rng(V + 4)
    L = rng.standard_normal((6, V)).astype(np.float32)
    L[0, [V // 5, V // 2, V - 1]] = 50.0     # tie across threads: the first
    L[1, V - 1] = 50.0                       # the last token
    L[2, :] = 0.25                           # all tied: token 0
    L[3, V // 2:V // 2 + 3] = 50.0           # tie inside one chunk
    L[4, :] = -np.inf
    L[5, :V - 1] = -np.inf                   # only the last token is finite
    got = _sample(_dev(L), T, k, 1.0, seed=1, counter=2)
    want = np.argmax(L, axis=1)
    assert (want[:4] == [V // 5, V - 1, 0, V // 2]).all() and want[5] == V - 1
    rows = [0, 1, 2, 3, 5]
    np.testing.assert_array_equal(got[rows], want[rows])
    assert 0 <= got[4] < V


@gpu_test
@pytest.mark.parametrize("V", EDGE_V)
def test_sample_rows_all_banned_row(gpu, V):
    """A row of -inf only: status OK and an id in [0, V), with and without
    filters; the rows beside it are unaffected."""
    rng = np.random.default_rng(V + 5)
    L = rng.standard_normal((3, V)).astype(np.float32)
    L[1] = -np.inf
    d = _dev(L)
    for kw in (dict(), dict(k=7), dict(p=0.8)):
        got = _sample(d, seed=2, counter=3, **kw)
        assert 0 <= got[1] < V
        assert got[0] == _sample(d[:1], seed=2, counter=3, **kw)[0]
