"""Gated MLP, the host-side rules (no device): the new entries are declared and
exported, and the gated GEMMs refuse bad shapes and modes before any launch
(fake pointers: nothing is dereferenced).  The decoder's setter rules need a
decoder: tests/test_gated_decoder_gpu.py."""
import ctypes

import pytest

P = ctypes.c_void_p(16)


def _i8(lib, K=64, N=16, mlp=1, A=P, lda=64, M=1):
    return lib.i8_gemm_gated(A, lda, 0, P, P, None, None, P, None, M, N, K, None, None, None,
                             None, None, mlp, None)


def _f16(lib, K=32, N=16, mlp=1):
    return lib.f16_gemm_gated(P, K, 0, P, P, P, None, 1, N, K, None, None, mlp, None)


@pytest.mark.parametrize("call,status,msg", [
    (lambda l: _i8(l, K=96, lda=96), 2, b"K % 64"),        # LLM_ERR_UNSUPPORTED: packed layout
    (lambda l: _i8(l, N=24), 2, b"N % 16"),
    (lambda l: _f16(l, K=48), 2, b"K % 32"),
    (lambda l: _i8(l, mlp=0), 1, b"LLM_MLP_GATED_SILU"),   # LLM_ERR_INVALID: plain is no activation
    (lambda l: _f16(l, mlp=3), 1, b"LLM_MLP_GATED_SILU"),
    (lambda l: _i8(l, A=None), 1, b"NULL operand"),
    (lambda l: _i8(l, lda=32), 1, b"lda"),
    (lambda l: _i8(l, M=-1), 1, b"bad M/N/K"),
    (lambda l: _i8(l, M=0), 0, None),                     # zero rows: a successful no-op
])
def test_gated_gemm_refusals(call, status, msg):
    import llm_capi
    lib = llm_capi.load()
    assert call(lib) == status
    if msg:
        assert msg in lib.llm_last_error()


def test_gated_symbols_declared():
    import llm_capi
    lib = llm_capi.load()
    declared = llm_capi.declared_symbols()
    for name in ("i8_gemm_gated", "f16_gemm_gated", "llm_decoder_set_mlp", "llm_decoder_mlp",
                 "llm_decoder_set_up_weights"):
        assert name in declared and hasattr(lib, name)
    assert lib.llm_decoder_mlp(None) == -1
    assert lib.llm_decoder_set_mlp(None, 1) == llm_capi.LLM_ERR_INVALID
