"""CPU checks of tests/_oproj.py, the host side of tests/test_oproj_rows_gpu.py,
and of the W_o head-slice layout the decoder uploads (csrc/oproj_slices.hpp,
through the tuning library's host-only oproj_head_slices_tune)."""
import itertools

import numpy as np
import pytest

import _oproj as op


@pytest.mark.parametrize("H,D,o_n", [(1, 32, 8), (3, 32, 200), (12, 64, 768), (64, 32, 2048),
                                     (8, 128, 1024)])
def test_head_slices_match_the_layout(H, D, o_n):
    """Distinct bit patterns (a counter, so a misplaced element cannot hide
    behind an equal one), byte for byte; and the layout read back index by
    index on a sample."""
    import llm_capi
    rng = np.random.default_rng([H, D, o_n])
    wo = (np.arange(H * D * o_n, dtype=np.uint32) * 2654435761 >> 7).astype(np.uint16)
    wo = wo.reshape(H * D, o_n)
    got = llm_capi.oproj_head_slices(wo.view(np.float16), H, D)
    want = op.slices_ref(wo, H, D)
    assert got.dtype == np.uint16 and got.shape == (H, D // 8, o_n, 8)
    assert got.tobytes() == want.tobytes()
    flat = got.ravel()
    KG = D // 8
    for _ in range(200):
        h, kg, n, j = (int(rng.integers(x)) for x in (H, KG, o_n, 8))
        assert flat[((h * KG + kg) * o_n + n) * 8 + j] == wo[h * D + 8 * kg + j, n]


def test_head_slices_refuse_bad_arguments():
    import llm_capi
    tune = llm_capi.load_tune()
    buf = np.zeros(64, np.uint16)
    assert tune.oproj_head_slices_tune(None, 1, 8, 8, buf.ctypes.data) == llm_capi.LLM_ERR_INVALID
    assert tune.oproj_head_slices_tune(buf.ctypes.data, 1, 12, 4, buf.ctypes.data) == \
        llm_capi.LLM_ERR_INVALID


def test_fixed_point_terms_and_negative_sums():
    # one head: the term is the count plus the value in units of 2^-32
    t, c = op.term_ref(1.5, 4)
    assert (t, c) == ((1 << 56) + (3 << 31), False)
    t, c = op.term_ref(-1.5, 4)
    assert (t, c) == ((1 << 56) - (3 << 31), False)
    # half-way cases of the 2^-32 grid round to even
    assert op.term_ref(2.0 ** -33, 1)[0] == (1 << 56)
    assert op.term_ref(3 * 2.0 ** -33, 1)[0] == (1 << 56) + 2
    assert op.term_ref(-3 * 2.0 ** -33, 1)[0] == (1 << 56) - 2
    # a negative sum borrows from the count bits: the count is still read back
    x, flag, cnt, v = op.fixed_point_ref([-3.25, 1.0, -0.5])
    assert (x, flag, cnt) == (np.float32(-2.75), False, 3)
    assert v < 3 << 56  # (the raw top byte alone would read 2)
    assert v >> 56 == 2
    x, flag, cnt, _ = op.fixed_point_ref([-2.0 ** -32])
    assert (x, flag, cnt) == (np.float32(-2.0 ** -32), False, 1)
    # cancellation to an exact zero with non-zero terms
    x, flag, cnt, v = op.fixed_point_ref([1234.5, -1000.25, -234.25])
    assert (x, flag, cnt, v) == (np.float32(0), False, 3, 3 << 56)
    # the completed value rounds once to fp32, half to even
    assert op._round_f32((1 << 24) + 1, 0) == np.float32(1 << 24)
    assert op._round_f32((1 << 24) + 3, 0) == np.float32((1 << 24) + 4)
    assert op._round_f32(-((1 << 25) + 2), 32) == np.float32(-(2.0 ** -7))
    assert op._round_f32(-((1 << 25) + 6), 32) == np.float32(-((1 << 25) + 8) * 2.0 ** -32)


@pytest.mark.parametrize("H", [1, 2, 64])
def test_count_survives_at_the_clamp_limit(H):
    """H terms at the limit of either sign stay below 2^23 in magnitude: the
    count reads H, the value is H * limit, and a term past the limit (or not
    finite) is clamped and flagged."""
    lim = float(op.oacc_limit(H))
    assert lim * H <= op.RANGE < 2 ** 23
    for sign in (1.0, -1.0):
        x, flag, cnt, v = op.fixed_point_ref([sign * lim] * H)
        assert (flag, cnt) == (False, H)
        assert x == np.float32(sign * lim * H)
        # every prefix of the arrivals counts right (the returning atomics read these)
        t = op.term_ref(sign * lim, H)[0]
        assert [op.count_ref(k * t) for k in range(H + 1)] == list(range(H + 1))
    over = float(np.nextafter(np.float32(lim), np.float32(np.inf)))
    for bad, want in ((over, lim), (-over, -lim), (float("inf"), lim), (float("-inf"), -lim),
                      (float("nan"), lim), (3.6e9, lim)):
        t, c = op.term_ref(bad, H)
        assert c and t == op.term_ref(want, H)[0], bad
        x, flag, cnt, _ = op.fixed_point_ref([bad] + [-lim] * (H - 1), H)
        assert flag and cnt == H
        assert x == np.float32(want - lim * (H - 1))


def test_order_independence():
    rng = np.random.default_rng(7)
    terms = [float(np.float32(t)) for t in rng.standard_normal(6) * 1000]
    terms[2] = float("nan")
    want = op.fixed_point_ref(terms)
    for perm in itertools.islice(itertools.permutations(terms), 0, 720, 7):
        assert op.fixed_point_ref(perm) == want
    # fp32 addition of the same terms is not order-independent: the reason for the integers
    a = [np.float32(1e8), np.float32(1.0), np.float32(-1e8)]
    assert (a[0] + a[1]) + a[2] != (a[0] + a[2]) + a[1]


def test_x_fixed_ref_is_the_plain_sum_where_nothing_rounds():
    rng = np.random.default_rng(8)
    c = op.exact_case(rng, 3, 4, 32, 9)
    terms = op.head_terms(c.v.reshape(3, -1), c.wo, 4, 32)
    x, cl = op.x_fixed_ref(terms, 4)
    assert not cl.any()
    np.testing.assert_array_equal(x.view(np.uint32), c.x.view(np.uint32))


@pytest.mark.parametrize("H,D,o_n", [(1, 64, 8), (3, 32, 200), (12, 64, 769), (64, 32, 64),
                                     (8, 128, 300)])
def test_exact_case_sums_are_exact_in_fp32(H, D, o_n):
    """The builder's promise: every partial sum a kernel can form is exactly
    representable (op.assert_fp32_exact), also at the worst values the draw
    allows, and the fp32 evaluation in several orders gives the same bits."""
    rng = np.random.default_rng([H, D, o_n])
    rows = 4
    c = op.exact_case(rng, rows, H, D, o_n, r0=2)
    assert c.v.min() >= -8 and c.v.max() <= 8
    w64 = c.wo.astype(np.float64)
    assert np.abs(w64).max() <= 2 and (w64 * 64 == np.rint(w64 * 64)).all()
    op.assert_fp32_exact(c.v, c.wo, H, D)
    worst_v = np.full((1, H, D), 8)
    worst_w = np.full((H * D, 2), 2.0, np.float16)
    op.assert_fp32_exact(worst_v, worst_w, H, D)
    # fp32 accumulation forwards, backwards and pairwise
    o = c.v.reshape(rows, H * D).astype(np.float32)
    w = c.wo.astype(np.float32)
    prod = o[:, :, None] * w[None]
    for order in (np.arange(H * D), np.arange(H * D)[::-1], rng.permutation(H * D)):
        acc = np.zeros((rows, o_n), np.float32)
        for k in order:
            acc = acc + prod[:, k]
        np.testing.assert_array_equal(acc, c.x)
    assert c.x[2, 1] < 0
    if H >= 2:
        assert c.x[2, 0] == 0


def test_x_bound_covers_fp32_accumulation():
    """The derived bound holds for a plain fp32 evaluation in the kernel's
    grouping (two-element dots accumulated per head, heads added on the 2^-32
    grid), and a one-ulp-of-fp16 error in one input breaks it."""
    rng = np.random.default_rng(9)
    B, H, D, o_n = 4, 3, 32, 50
    o16 = np.clip(1 + 0.25 * rng.standard_normal((B, H * D)), 0.25, None).astype(np.float16)
    wo = (0.02 * rng.standard_normal((H * D, o_n))).astype(np.float16)
    o, w = o16.astype(np.float32), wo.astype(np.float32)
    x = np.zeros((B, o_n), np.float32)
    vals = np.empty((B, H, o_n), np.float32)
    for h in range(H):
        p = np.zeros((B, o_n), np.float32)
        for k in range(h * D, (h + 1) * D, 2):
            p = (p + o[:, k, None] * w[None, k]) + o[:, k + 1, None] * w[None, k + 1]
        vals[:, h] = p
    x, cl = op.x_fixed_ref(vals, H)
    assert not cl.any()
    err = np.abs(x.astype(np.float64) - op.x_ref64(o16, wo))
    bound = op.x_bound(o16, wo, H, D)
    assert (err <= bound).all() and (err / bound).max() < 0.5
    bent = o16.copy()
    bent[1, 40] = np.nextafter(bent[1, 40], np.float16(9))
    assert (np.abs(x.astype(np.float64) - op.x_ref64(bent, wo)) > op.x_bound(bent, wo, H, D)).any()
