"""i8_gemm_gated / f16_gemm_gated (csrc/gemm_gated.hip) through llm_capi.

I8: the acc_out pair equals the numpy int64 products bit for bit, and H is
held to a float64 evaluation of the header's formula from those sums.  F16: H
against float64 on the fp16-rounded inputs.  The H bound is 4x the largest
relative error |h - ref| / max(|ref|, 1e-3 max|ref|) of the fp32 numpy
restatement of the same formula (fp32-accumulating for F16) on the same
inputs, the factor for the device's exp / erf differing by a few ulp.  The
packed fp16 image is the fp16 rounding of H bit for bit.
Shapes: waves with no k-steps (K 64), a partial row block (M 17, 80), two row
blocks (M 80), and a partial column tile ((32, 64, 8208): the only size at
which 17..32 rows take two column tiles per workgroup, 513 tiles)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _frag_off(M, K, KS, kstep):
    """Offsets of [M][K] in MFMA A-fragment order (csrc/common.hpp a_frag_off_i8 / _f16)."""
    g = kstep // 4  # elements per lane
    m, k = np.arange(M)[:, None], np.arange(K)[None, :]
    return (((m >> 4) * KS + k // kstep) * 64 + (m & 15) + 16 * (k % kstep // g)) * g + k % g


def _pack_a(A, kstep):
    M, K = A.shape
    out = np.zeros((M + 15) // 16 * K * 16, A.dtype)
    out[_frag_off(M, K, K // kstep, kstep)] = A
    return out


def _erf(x):
    from scipy.special import erf
    return erf(x.astype(np.float64))


def _formula(G, U, mlp, f):
    """act(G) * U in float type f, one rounding per operation, in the kernel's order."""
    one = f(1)
    if mlp == 2:
        a = (f(0.5) * G) * (one + _erf(G * f(0.70710678118654752)).astype(f))
    else:
        with np.errstate(over="ignore"):
            a = G / (one + np.exp(-G))
    return a * U


def _worst(h, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(h - ref) / np.maximum(np.abs(ref), 1e-3 * np.abs(ref).max())))


@pytest.mark.parametrize("dtype", ["i8", "f16"])
@pytest.mark.parametrize("K,N", [(64, 16), (192, 48), (2048, 272)])
@pytest.mark.parametrize("M", [1, 16, 17, 64, 80])
def test_gemm_gated(gpu, M, K, N, dtype):
    _run(M, K, N, dtype)


@pytest.mark.parametrize("dtype", ["i8", "f16"])
def test_gemm_gated_two_column_tiles(gpu, dtype):
    _run(32, 64, 8208, dtype)


def _run(M, K, N, dtype):
    import llm_capi
    rng = np.random.default_rng(M * 131 + K + N)
    i8 = dtype == "i8"
    kstep = 64 if i8 else 32
    if i8:
        A = rng.integers(-128, 128, (M, K), dtype=np.int8)
        Wg, Wu = (rng.integers(-128, 128, (K, N), dtype=np.int8) for _ in range(2))
        sa = rng.uniform(0.5, 1.5, M).astype(F)
        # G and U of a few units: the activations' curved range
        swg, swu = (rng.uniform(0.5, 1.5, N).astype(F) * F(2 / (5400 * np.sqrt(K)))
                    for _ in range(2))
        ag, au = (A.astype(np.int64) @ W.astype(np.int64) for W in (Wg, Wu))
        Sg, Su = sa[:, None] * swg[None, :], sa[:, None] * swu[None, :]  # fp32 products
        g32, u32 = ag.astype(F) * Sg, au.astype(F) * Su
        g64, u64 = ag * Sg.astype(np.float64), au * Su.astype(np.float64)
    else:
        A = rng.standard_normal((M, K)).astype(np.float16)
        Wg, Wu = ((rng.standard_normal((K, N)) * 1.5 / np.sqrt(K)).astype(np.float16)
                  for _ in range(2))
        g32, u32 = (A.astype(F) @ W.astype(F) for W in (Wg, Wu))
        g64, u64 = (A.astype(np.float64) @ W.astype(np.float64) for W in (Wg, Wu))
    bg, bu = (rng.standard_normal(N).astype(F) for _ in range(2))
    packed = M % 2 == 1 or M == 64
    if packed:
        Ad, kw = _dev(_pack_a(A, kstep)), dict(M=M, K=K)
    else:
        wide = np.full((M, K + 32), 77, A.dtype)  # lda > K: the padding must not be read
        wide[:, :K] = A
        Ad, kw = _dev(wide)[:, :K], {}
    code = llm_capi.LLM_I8 if i8 else llm_capi.LLM_F16
    Pg, Pu = (llm_capi.pack_weights(_dev(W), code) for W in (Wg, Wu))
    if i8:
        kw.update(sa=_dev(sa), sw_gate=_dev(swg), sw_up=_dev(swu))
    off16 = _frag_off(M, N, (N + 31) // 32, 32)
    for mlp in (llm_capi.LLM_MLP_GATED_SILU, llm_capi.LLM_MLP_GATED_GELU):
        for bias in (False, True):
            accg, accu, H, H16 = llm_capi.gemm_gated(
                Ad, Pg, Pu, N, mlp=mlp, b_gate=_dev(bg) if bias else None,
                b_up=_dev(bu) if bias else None, **kw)
            if i8:
                np.testing.assert_array_equal(accg.cpu().numpy(), ag)
                np.testing.assert_array_equal(accu.cpu().numpy(), au)
            b = (bg[None, :], bu[None, :]) if bias else (F(0), F(0))
            ref = _formula(g64 + np.float64(b[0]), u64 + np.float64(b[1]), mlp, np.float64)
            # (floored at one fp32 ulp: on a handful of outputs the restatement's
            # five roundings can all land well, which no other evaluation owes)
            base = max(_worst(_formula(g32 + b[0], u32 + b[1], mlp, F), ref), 2.0 ** -23)
            H = H.cpu().numpy()
            err = _worst(H, ref)
            print(f"gated {dtype} M {M} K {K} N {N} mlp {mlp} bias {bias}: fp32 numpy {base:.3e} "
                  f"bound {4 * base:.3e} device {err:.3e}")
            assert err <= 4 * base, (mlp, bias, err, base)
            np.testing.assert_array_equal(H16.cpu().numpy().view(np.uint16)[off16],
                                          H.astype(np.float16).view(np.uint16))
