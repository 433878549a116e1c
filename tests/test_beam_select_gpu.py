"""beam_select_rows (csrc/beam_select.hip) against the float64 restatement
tests/_beam.py select_ref: token and parent ids exactly, scores within
1e-5 + 1e-6 |score| (fp32 log-sum-exp against float64).

Inputs are drawn so that adjacent float64 candidate scores of a sequence differ
by more than 1e-3 (asserted here, on the CPU) except for the planted exact
ties: a pair of beams with identical logits and scores (order by parent, then
token) and a row whose logits are all equal (ids ascend).  Some rows carry a
-inf score (beams that are not live)."""
import numpy as np
import pytest

from _beam import select_ref

pytestmark = pytest.mark.gpu


def _case(V, W, S, seed):
    """logits [S * W][V] fp32, score_in [S * W] fp32, or None if two candidates
    of a sequence that are not planted ties lie within 1e-3."""
    rng = np.random.default_rng(seed)
    R = S * W
    logits = (2.0 * rng.standard_normal((R, V))).astype(np.float32)
    score = (-5.0 * rng.random(R)).astype(np.float32)
    # the planted rows get scores that put their candidates among the reported 2W
    special = {}
    if W > 1:
        special[(0, W - 1)] = "dead"
        score[W - 1] = -np.inf
    dseq = S - 1
    if (S > 1 and W >= 2) or W >= 3:
        special[(dseq, 0)] = special[(dseq, 1)] = "dup"
        logits[dseq * W + 1] = logits[dseq * W]
        score[dseq * W] = score[dseq * W + 1] = 3.0
    eq = (1, 0) if S > 1 else (0, 0) if W == 1 else None
    if eq is not None:
        special[eq] = "equal"
        logits[eq[0] * W + eq[1]] = np.float32(rng.standard_normal())
        score[eq[0] * W + eq[1]] = 12.0
    ref = select_ref(logits, score, W)
    for s in range(S):
        sc = ref[0][s]
        sc = sc[np.isfinite(sc)]
        d = sc[:-1] - sc[1:]
        if ((d != 0) & (d <= 1e-3)).any():
            return None
    return logits, score, ref, special


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("W", [1, 2, 3, 4])
@pytest.mark.parametrize("V", [33, 500, 50257])
def test_beam_select_matches_float64(gpu, V, W, S):
    import torch
    import llm_capi
    case = None
    for seed in range(100 * V + 10 * W + S, 100 * V + 10 * W + S + 4000, 40):
        case = _case(V, W, S, seed)
        if case is not None:
            break
    assert case is not None, "no draw with candidate scores > 1e-3 apart"
    logits, score, (rs, rp, rt), special = case
    K = 2 * W
    # the CPU side of the contract: adjacent float64 scores differ by > 1e-3 or are planted ties
    for s in range(S):
        sc = rs[s][np.isfinite(rs[s])]
        d = sc[:-1] - sc[1:]
        assert (((d == 0) | (d > 1e-3))).all()
        assert len(sc) >= K
    dl, ds = torch.from_numpy(logits).cuda(), torch.from_numpy(score).cuda()
    cs, cp, ct = llm_capi.beam_select(dl, ds, W)
    torch.cuda.synchronize()
    cs, cp, ct = cs.cpu().numpy(), cp.cpu().numpy(), ct.cpu().numpy()
    assert np.array_equal(cp, rp[:, :K]), (cp, rp[:, :K])
    assert np.array_equal(ct, rt[:, :K]), (ct, rt[:, :K])
    err = np.abs(cs.astype(np.float64) - rs[:, :K])
    tol = 1e-5 + 1e-6 * np.abs(rs[:, :K])
    assert (err <= tol).all(), (err.max(), (err / tol).max())
    # the planted cases did what they were planted for
    kinds = set(special.values())
    if "dup" in kinds:
        s = S - 1
        pairs = list(zip(cs[s], cp[s], ct[s]))
        ties = [(a, b) for a, b in zip(pairs, pairs[1:]) if a[0] == b[0]]
        assert ties and all(a[1:] < b[1:] for a, b in ties), pairs
    if "equal" in kinds:
        (s, b), = [k for k, v in special.items() if v == "equal"]
        toks = [int(t) for p, t in zip(cp[s], ct[s]) if p == b]
        assert toks == list(range(K)), toks  # equal logits: ids ascend from 0
    if W == 1:  # raw-logit ranking: the winner is argmax_rows' id
        am = llm_capi.argmax_rows(dl).cpu().numpy()
        assert np.array_equal(ct[:, 0], am)
    # a second call gives the same bits (fixed reduction order, no atomics)
    cs2, cp2, ct2 = llm_capi.beam_select(dl, ds, W)
    assert np.array_equal(cs2.cpu().numpy().view(np.uint32), cs.view(np.uint32))
    assert np.array_equal(cp2.cpu().numpy(), cp) and np.array_equal(ct2.cpu().numpy(), ct)
