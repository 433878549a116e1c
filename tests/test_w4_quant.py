"""The 4-bit weight format on the host (include/llm_decoder.h "INT4 weights"):
w4_quantize / w4_expand ranges, error bound, fixed point and nibble layout."""
import numpy as np
import pytest


def _edge_matrix():
    """384 x 16: +-127 / -128 columns, all-zero groups, a group of one value."""
    rng = np.random.default_rng(5)
    W = rng.integers(-127, 128, (384, 16)).astype(np.int8)
    W[:128, 0] = 127
    W[:128, 1] = -127
    W[:128, 2] = -128
    W[128:256, :] = 0          # all-zero groups in every column
    W[256:, 3] = 0
    W[300, 3] = 5
    return W


@pytest.mark.parametrize("name", ["128x16", "384x48", "edge"])
def test_w4_quantize_ranges_error_and_fixed_point(name):
    import llm_capi
    if name == "edge":
        W8 = _edge_matrix()
    else:
        K, N = (int(x) for x in name.split("x"))
        W8 = np.random.default_rng(K).integers(-127, 128, (K, N)).astype(np.int8)
    K, N = W8.shape
    q, m = llm_capi.w4_quantize(W8)
    assert q.shape == (K // 2, N) and m.shape == (K // 128, N)
    assert m.min() >= 1 and m.max() <= 18
    nib = np.stack([q & 15, q >> 4], axis=1).reshape(K, N).astype(np.int16)  # even k low
    qv = np.where(nib >= 8, nib - 16, nib)
    assert qv.min() >= -7 and qv.max() <= 7
    E = llm_capi.w4_expand(q, m)
    mk = np.repeat(m.astype(np.int16), 128, axis=0)
    np.testing.assert_array_equal(E, (qv * mk).astype(np.int8))
    assert np.all(2 * np.abs(E.astype(np.int16) - W8) <= mk)
    # representable weights are a fixed point
    q2, m2 = llm_capi.w4_quantize(E)
    np.testing.assert_array_equal(llm_capi.w4_expand(q2, m2), E)
    if name == "edge":
        assert m[1].max() == 1 and not E[128:256].any()
        assert list(m[0, :3]) == [18, 18, 18] and list(E[0, :3]) == [126, -126, -126]
        assert m[2, 3] == 1 and E[300, 3] == 5


def test_w4_nibble_layout_by_hand():
    """Column n of a 128 x 16 matrix holds weights k - 64 + n scaled so that
    the multiplier and every nibble are known without the quantiser's code."""
    import llm_capi
    W8 = np.zeros((128, 16), np.int8)
    W8[0, :] = 21            # max 21 -> m = 3, q = 7
    W8[1, :] = -21           # q = -7 -> nibble 0x9
    W8[2, 5] = 4             # 4 / 3 = 1.33 -> 1
    W8[3, 5] = -5            # -1.67 -> -2 -> nibble 0xE
    W8[127, 15] = 10         # 3.33 -> 3, odd k: high nibble of byte (63, 15)
    q, m = llm_capi.w4_quantize(W8)
    assert (m == 3).all()
    assert (q[0] == 0x97).all()                  # k 0 low nibble 7, k 1 high nibble 9
    assert q[1, 5] == 0xE1 and q[1, 4] == 0
    assert q[63, 15] == 0x30
    assert not q[2:63].any()
