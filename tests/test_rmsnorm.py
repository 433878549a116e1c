"""RMSNorm, the host-side rules (no device): the seven entries are declared,
exported and prototyped, and the launches refuse bad arguments before anything
runs (fake pointers: nothing is dereferenced).  Numerics and the decoder mode:
tests/test_rmsnorm_gpu.py."""
import ctypes

import pytest

P = ctypes.c_void_p(16)
NAMES = ("rmsnorm_quant", "i8_gemm_rms", "f16_gemm_rms", "i8_gemm_gated_rms",
         "f16_gemm_gated_rms", "llm_decoder_set_norm", "llm_decoder_norm")


def _row(lib, x=P, rows=1, cols=64, eps=1e-5, out=P):
    return lib.rmsnorm_quant(x, rows, cols, P, eps, out, None, None, None)


def _i8(lib, x=P, M=1, K=64, eps=1e-5):
    return lib.i8_gemm_rms(x, P, eps, P, P, M, 16, K, None, None, 0, None, None, None)


def _f16(lib, M=1, K=32, eps=1e-5):
    return lib.f16_gemm_rms(P, P, eps, P, P, M, 16, K, None, 0, None, None)


def _gi8(lib, x=P, M=1, K=64, eps=1e-5):
    return lib.i8_gemm_gated_rms(x, P, eps, P, P, None, None, P, None, M, 16, K, None, None, None,
                                 None, 1, None, None, None)


def _gf16(lib, M=1, K=32, eps=1e-5):
    return lib.f16_gemm_gated_rms(P, P, eps, P, P, P, None, M, 16, K, None, None, 1, None, None)


@pytest.mark.parametrize("call,status,msg", [
    (lambda l: _row(l, x=None), 1, b"NULL pointer"),
    (lambda l: _row(l, out=None), 1, b"no output"),
    (lambda l: _row(l, eps=0.0), 1, b"eps"),
    (lambda l: _row(l, cols=16388), 1, b"16384"),
    (lambda l: _row(l, rows=0), 0, None),
    (lambda l: _i8(l, x=None), 1, b"NULL operand"),
    (lambda l: _i8(l, K=96), 1, b"multiple of 64"),
    (lambda l: _f16(l, K=48), 1, b"multiple of 32"),
    (lambda l: _i8(l, eps=-1.0), 1, b"eps"),
    (lambda l: _f16(l, eps=0.0), 1, b"eps"),
    (lambda l: _i8(l, M=16, K=2048), 2, b"ln_fusable"),      # 128 KiB of fp32 rows per workgroup
    (lambda l: _f16(l, M=64, K=512), 2, b"ln_fusable"),
    (lambda l: _i8(l, M=0), 0, None),
    (lambda l: _f16(l, M=0), 0, None),
    (lambda l: _gi8(l, x=None), 1, b"NULL operand"),
    (lambda l: _gi8(l, K=96), 2, b"K % 64"),
    (lambda l: _gf16(l, K=48), 2, b"K % 32"),
    (lambda l: _gi8(l, eps=0.0), 1, b"eps"),
    (lambda l: _gf16(l, eps=-1.0), 1, b"eps"),
    (lambda l: _gi8(l, M=65), 2, b"gated_rms_fusable"),      # decode row counts only
    (lambda l: _gi8(l, K=4096), 2, b"gated_rms_fusable"),    # past 8 chunks per lane
    (lambda l: _gf16(l, M=64, K=2048), 2, b"gated_rms_fusable"),  # a 256 KiB fp16 image
    (lambda l: _gi8(l, M=0), 0, None),
    (lambda l: _gf16(l, M=0), 0, None),
])
def test_rms_refusals(call, status, msg):
    import llm_capi
    lib = llm_capi.load()
    assert call(lib) == status
    if msg:
        assert msg in lib.llm_last_error()


def test_rms_symbols_declared():
    import llm_capi
    lib = llm_capi.load()
    declared = llm_capi.declared_symbols()
    for name in NAMES:
        assert name in declared and hasattr(lib, name) and name in llm_capi._SIGS
    assert lib.llm_decoder_norm(None) == -1
    assert lib.llm_decoder_set_norm(None, 1, 1e-5) == llm_capi.LLM_ERR_INVALID
