"""The beam search's host bookkeeping (csrc/beam_plan.hpp) through the tuning
library's beam_book_tune: what llm_decoder_beam_search does with the device's
candidates, without a device, against the plain-Python restatement
tests/_beam.py::bookkeeping.

Sums and final scores are compared as float32 BITS: the sums are copies of
candidate scores, and both sides compute sum / len^alpha in double with the
same libm pow and round once to float32 (tests/test_beam_search_gpu.py holds
the library to the same bits).
"""
import ctypes

import numpy as np
import pytest

import llm_capi
from _beam import bookkeeping

V = 12          # small, so EOS is frequent
EOS = 7
STEPS = 6
OUT_OF_RANGE = b"the device returned a candidate out of range"
TOO_FEW_LIVE = b"fewer than beam_width live candidates"


def candidates(seed, S, W, eos, steps=STEPS):
    """A candidate stream [steps][S][2W] as the device reports one: scores in
    rank order (descending, ties allowed), parents in [0, W), tokens in [0, V)
    with at most W EOS per row (EOS appears at most once per parent)."""
    rng = np.random.default_rng(seed)
    K = 2 * W
    cs = -np.sort(rng.integers(1, 40, (steps, S, K)), axis=2).astype(np.float32) / 4 \
        - np.arange(steps, dtype=np.float32)[:, None, None] * 8
    cp = rng.integers(0, W, (steps, S, K)).astype(np.int32)
    ct = rng.integers(0, V, (steps, S, K)).astype(np.int32)
    if eos >= 0:
        ct[rng.random(ct.shape) < 0.3] = eos
        for row in ct.reshape(-1, K):
            for j in np.flatnonzero(row == eos)[W:]:
                row[j] = (eos + 1 + rng.integers(0, V - 1)) % V  # any token but EOS
    return cs, cp, ct


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_against_reference(cs, cp, ct, W, max_new, eos, alpha):
    # llm_beam_options::length_penalty is a C float: the penalty of a search
    # asked for 0.7 is float32(0.7), and that is what both sides are given
    alpha = float(np.float32(alpha))
    ref = bookkeeping(cs, cp, ct, W=W, max_new=max_new, eos_token=eos, length_penalty=alpha)
    rc, got = llm_capi.beam_book(cs, cp, ct, W, V, max_new, eos, alpha)
    assert rc == llm_capi.LLM_OK
    assert got["steps"] == ref["steps"]
    assert got["live_parent"].tolist() == ref["live_parent"].tolist()
    assert got["live_token"].tolist() == ref["live_token"].tolist()
    assert got["length"].tolist() == ref["length"].tolist()
    for s, hyps in enumerate(ref["ids"]):
        for w, ids in enumerate(hyps):
            assert got["ids"][s, w].tolist() == ids + [-1] * (max_new - len(ids)), (s, w)
    assert bits(got["sum_logprob"]).tolist() == bits(ref["sum_logprob"]).tolist()
    assert bits(got["score"]).tolist() == bits(ref["score"]).tolist()
    return ref


@pytest.mark.parametrize("alpha", [1.0, 0.0])
def test_hand_case(alpha):
    """test_beam_args.py::test_reference_bookkeeping_by_hand through the hook."""
    cs = np.array([[[-1.0, -2.0, -3.0, -4.0]], [[-1.5, -2.5, -2.75, -5.0]]], np.float32)
    cp = np.array([[[0, 0, 0, 0]], [[1, 0, 0, 1]]], np.int32)
    ct = np.array([[[4, 5, 6, 7]], [[9, 3, 9, 2]]], np.int32)
    rc, r = llm_capi.beam_book(cs, cp, ct, 2, 10, 2, 9, alpha)
    assert rc == llm_capi.LLM_OK and r["steps"] == 2
    assert r["live_parent"].tolist() == [[[0, 0]], [[0, 1]]]
    assert r["live_token"].tolist() == [[[4, 5]], [[3, 2]]]
    assert r["ids"].tolist() == [[[5, 9], [4, 3]]] and r["length"].tolist() == [[2, 2]]
    assert r["sum_logprob"].tolist() == [[-1.5, -2.5]]
    assert r["score"].tolist() == ([[-0.75, -1.25]] if alpha == 1.0 else [[-1.5, -2.5]])


@pytest.mark.parametrize("eos", [EOS, -1])
@pytest.mark.parametrize("W", [1, 2, 4])
@pytest.mark.parametrize("S", [1, 3])
def test_random_streams(S, W, eos):
    for seed in range(6):
        cs, cp, ct = candidates(1000 * S + 100 * W + seed, S, W, eos)
        for alpha in (0.0, 0.5, 0.7, 1.0):
            # fewer, as many and more steps asked for than the stream holds
            for max_new in (STEPS - 2, STEPS, STEPS + 2):
                check_against_reference(cs, cp, ct, W, max_new, eos, alpha)


def done_after(cs, cp, ct, W, k):
    """The sequences' done flags after k steps."""
    return bookkeeping(cs, cp, ct, W=W, max_new=k, eos_token=EOS, length_penalty=1.0)["done"]


def test_seed_eos_at_rank_w_or_later_is_ignored():
    """Seed 4 (S 1, W 2): the first step reports an EOS at rank 2 and none
    above it, so nothing is finished by it."""
    cs, cp, ct = candidates(4, 1, 2, EOS)
    assert EOS in ct[0, 0, 2:] and EOS not in ct[0, 0, :2]
    check_against_reference(cs, cp, ct, 2, STEPS, EOS, 0.7)
    ref = bookkeeping(cs, cp, ct, W=2, max_new=1, eos_token=EOS, length_penalty=0.7)
    assert all(EOS not in ids for ids in ref["ids"][0])


def test_seed_one_sequence_done_while_others_run_on():
    """Seed 1 (S 3, W 2): after step 2 some sequence is done and another is
    not, and the search goes on -- the done one still advances its beams (its
    live parents / tokens of the later steps are compared like any other's)."""
    cs, cp, ct = candidates(1, 3, 2, EOS)
    d = done_after(cs, cp, ct, 2, 2)
    assert any(d) and not all(d)
    ref = check_against_reference(cs, cp, ct, 2, STEPS, EOS, 0.5)
    assert ref["steps"] > 2


def test_seed_all_done_before_max_new():
    """Seed 0 (S 3, W 1): every sequence is done after fewer than max_new steps."""
    cs, cp, ct = candidates(0, 3, 1, EOS)
    ref = check_against_reference(cs, cp, ct, 1, STEPS, EOS, 1.0)
    assert all(ref["done"]) and ref["steps"] < STEPS


def test_seed_live_beams_enter_the_pool():
    """Seed 18 (S 3, W 4): a sequence is not done after the last step, so its
    live beams are ranked with what it finished."""
    cs, cp, ct = candidates(18, 3, 4, EOS)
    ref = check_against_reference(cs, cp, ct, 4, STEPS, EOS, 0.7)
    assert not all(ref["done"]) and ref["steps"] == STEPS
    s = ref["done"].index(False)
    assert any(ids[-1] != EOS for ids in ref["ids"][s])


def test_candidate_out_of_range():
    tune = llm_capi.load_tune()
    for field, bad in (("parent", 2), ("parent", -1), ("token", V), ("token", -1)):
        cs, cp, ct = candidates(0, 1, 2, -1, steps=2)
        (cp if field == "parent" else ct)[1, 0, 3] = bad
        rc, r = llm_capi.beam_book(cs, cp, ct, 2, V, 2, -1, 1.0)
        assert rc == llm_capi.LLM_ERR_HIP and r is None, (field, bad)
        assert OUT_OF_RANGE in tune.llm_last_error()


def test_fewer_than_beam_width_live_candidates():
    tune = llm_capi.load_tune()
    cs = np.array([[[-1.0, -2.0, -3.0, -4.0]]], np.float32)
    cp = np.zeros((1, 1, 4), np.int32)
    ct = np.array([[[EOS, EOS, 3, EOS]]], np.int32)
    rc, r = llm_capi.beam_book(cs, cp, ct, 2, V, 3, EOS, 1.0)
    assert rc == llm_capi.LLM_ERR_HIP and r is None
    assert TOO_FEW_LIVE in tune.llm_last_error()


def test_bad_hook_arguments():
    tune = llm_capi.load_tune()
    cs, cp, ct = candidates(0, 1, 2, EOS, steps=2)
    out_i = np.zeros(64, np.int32)
    out_f = np.zeros(64, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(W=2, vocab=V, steps=2, S=1, max_new=2, eos=EOS, alpha=1.0, null=None):
        ptrs = [p(cs), p(cp), p(ct), p(out_i), p(out_i), p(out_f), p(out_f), p(out_i), p(out_i),
                p(out_i)]
        if null is not None:
            ptrs[null] = None
        return tune.beam_book_tune(*ptrs[:3], steps, S, W, vocab, max_new, eos, alpha, *ptrs[3:])

    assert call() == llm_capi.LLM_OK
    for i in range(10):
        assert call(null=i) == llm_capi.LLM_ERR_INVALID, i
    assert b"NULL" in tune.llm_last_error()
    for W in (0, 5, -1):
        assert call(W=W) == llm_capi.LLM_ERR_INVALID
    assert call(W=2, vocab=3) == llm_capi.LLM_ERR_INVALID  # 2W > V
    assert b"V >= 2W" in tune.llm_last_error()
    for kw in (dict(steps=0), dict(S=0), dict(max_new=0), dict(eos=V), dict(eos=-2),
               dict(alpha=-1.0), dict(alpha=float("nan"))):
        assert call(**kw) == llm_capi.LLM_ERR_INVALID, kw
