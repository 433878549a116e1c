"""w4_gemm (csrc/gemm_w4.hip) against a numpy int64 product on w4_expand's
output: exact int32 sums, and C equal in every bit to i8_gemm on the packed
expanded weights and to the float32 two-rounding formula (bit-exact for act
none / relu; GELU at 1e-6, the bar tests/test_gemm_gpu.py holds i8_gemm to:
the device erff is not the correctly rounded erf)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pack_a(A):
    """int8 [M][K] -> MFMA A-fragment order (csrc/common.hpp a_frag_off_i8)."""
    M, K = A.shape
    KS = K // 64
    out = np.zeros((M + 15) // 16 * KS * 1024, np.int8)
    m, k = np.arange(M)[:, None], np.arange(K)[None, :]
    out[(((m >> 4) * KS + (k >> 6)) * 64 + (m & 15) + 16 * ((k & 63) >> 4)) * 16 + (k & 15)] = A
    return out


def _check(A, q, m, packed, sa, sw, bias, act):
    import llm_capi
    M, K = A.shape
    N = q.shape[1]
    W8 = llm_capi.w4_expand(q, m)
    Wp = llm_capi.w4_pack_weights(_dev(q), _dev(m))
    assert Wp.numel() == K * N // 2 + K * N // 128
    kw = dict(sa=_dev(sa), sw=_dev(sw), bias=_dev(bias), act=act)
    if packed:
        acc, C = llm_capi.w4_gemm(_dev(_pack_a(A)), Wp, N, M=M, K=K, **kw)
    else:
        wide = np.full((M, K + 32), 77, np.int8)  # lda > K: the padding must not be read
        wide[:, :K] = A
        acc, C = llm_capi.w4_gemm(_dev(wide)[:, :K], Wp, N, **kw)
    ref = A.astype(np.int64) @ W8.astype(np.int64)
    assert np.abs(ref).max() < 2 ** 31
    np.testing.assert_array_equal(acc.cpu().numpy(), ref)
    _, C8 = llm_capi.i8_gemm(_dev(A), llm_capi.pack_weights(_dev(W8), llm_capi.LLM_I8), N, **kw)
    C = C.cpu().numpy()
    np.testing.assert_array_equal(C.view(np.uint32), C8.cpu().numpy().view(np.uint32))
    one = np.float32(1)
    scale = (one if sa is None else sa[:, None]) * (one if sw is None else sw[None, :])
    y = ref.astype(np.float32) * np.float32(scale)
    if bias is not None:
        y = y + bias[None, :]
    if act == 1:
        y = np.maximum(y, np.float32(0))
    if act < 2:
        np.testing.assert_array_equal(C, y.astype(np.float32))
    else:
        from scipy.special import erf
        y = y.astype(np.float64)
        np.testing.assert_allclose(C, 0.5 * y * (1 + erf(y / np.sqrt(2))), rtol=1e-6, atol=1e-6)


# M: both decode row tiles and the 64-row prefill blocks; K: one group, an odd
# group count (the waves' split has a remainder), a project dim; N: below a
# column block, a partial last block, and 384 tiles (two column tiles per
# workgroup at 17..32 rows: with one group, with an odd count, and with two
# groups per wave, so both of a wave's batches are in flight).  flags: packed
# A, sa, sw, bias.
@pytest.mark.parametrize("M,K,N,flags,act", [
    (1, 128, 16, "----", 0), (1, 2048, 48, "pawb", 0), (15, 384, 48, "-awb", 1),
    (15, 2048, 16, "p-w-", 2), (17, 384, 272, "pawb", 2), (17, 128, 6144, "-awb", 1),
    (17, 384, 6144, "pa-b", 0), (32, 2048, 6144, "-aw-", 0),
    (17, 2048, 272, "-a-b", 0), (64, 2048, 272, "paw-", 0), (64, 384, 48, "-a-b", 1),
    (64, 128, 16, "p--b", 2), (515, 384, 48, "pawb", 0), (515, 128, 272, "--w-", 2),
    (515, 2048, 16, "-awb", 1),
])
def test_w4_gemm_exact(gpu, M, K, N, flags, act):
    import llm_capi
    rng = np.random.default_rng(M * 7 + K + N)
    A = rng.integers(-128, 128, (M, K), dtype=np.int8)
    # an amplitude of its own per (group, column), so that the multipliers span
    # [1, 18] and differ between neighbouring groups, columns and column
    # tiles: a multiplier read from another group or tile changes the sums
    g, n = np.arange(K // 128)[:, None], np.arange(N)[None, :]
    amp = np.minimum(127, 7 * (1 + (5 * g + 7 * n) % 18)).repeat(128, axis=0)
    q, m = llm_capi.w4_quantize(np.rint(rng.uniform(-1, 1, (K, N)) * amp).astype(np.int8))
    assert m.min() == 1 and m.max() == 18 and len(np.unique(m)) >= 12
    sa = rng.uniform(1e-3, 1e-2, M).astype(np.float32) if "a" in flags else None
    sw = rng.uniform(1e-3, 1e-2, N).astype(np.float32) if "w" in flags else None
    bias = rng.standard_normal(N).astype(np.float32) if "b" in flags else None
    _check(A, q, m, "p" in flags, sa, sw, bias, act)


def test_w4_gemm_full_range(gpu):
    """K 16384, every A -128 or 127, q +-7, m 18, signs aligned: |acc| reaches
    K * 127 * 126 (a lost shift, a 24-bit overflow or a missing sign shows)."""
    K, N = 16384, 16
    rng = np.random.default_rng(1)
    sign = rng.integers(0, 2, (K, N)).astype(bool)
    qv = np.where(sign, 7, -7).astype(np.int16) & 15
    q = (qv[0::2] | (qv[1::2] << 4)).astype(np.uint8)
    m = np.full((K // 128, N), 18, np.uint8)
    A = np.empty((1, K), np.int8)
    A[0] = np.where(sign[:, 3], 127, -128)  # aligned with column 3: the positive extreme
    _check(A, q, m, False, None, None, None, 0)
    _check(-1 - A, q, m, True, None, None, None, 0)  # (-128 <-> 127: the negative extreme)
