"""CPU checks of the log-probability entries: lm_head_logprobs, logprob_rows,
llm_decoder_score, llm_decoder_submit_logprobs and llm_decoder_serve_logprobs
are declared in include/llm_decoder.h, exported with C linkage and prototyped
in llm_capi; the ABI version is unchanged; and their host refusals return
LLM_ERR_INVALID with fake pointers (nothing is dereferenced, nothing is
launched: safe without a GPU)."""
import ctypes
import subprocess

NEW = ["lm_head_logprobs", "logprob_rows", "llm_decoder_score", "llm_decoder_submit_logprobs",
       "llm_decoder_serve_logprobs"]


def test_symbols_declared_exported_prototyped():
    import llm_capi
    lib = llm_capi.load()
    declared = llm_capi.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", str(llm_capi.LIB_PATH)],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/llm_decoder.h"
        assert name in exported, f"{name} is not exported"
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, f"{name} has no prototype"
    assert lib.llm_abi_version() == 3
    assert llm_capi.LLM_MAX_TOP_LOGPROBS == 8


def test_lm_head_logprobs_refusals():
    import llm_capi
    lib = llm_capi.load()
    INV = llm_capi.LLM_ERR_INVALID
    p = ctypes.c_void_p(16)
    ok = (p, p, p, p, None)  # x, E, targets, logprob, stats (nullable)
    assert lib.lm_head_logprobs(*ok, 0, 10, 64, None) == 0  # M == 0: a no-op
    assert lib.lm_head_logprobs(None, None, None, None, None, 0, 10, 64, None) == 0
    for i in range(4):  # every operand but stats
        args = list(ok)
        args[i] = None
        assert lib.lm_head_logprobs(*args, 1, 10, 64, None) == INV
        assert b"NULL" in lib.llm_last_error()
    assert lib.lm_head_logprobs(*ok, 1, 10, 33, None) == INV
    assert b"multiple of 32" in lib.llm_last_error()
    # packed E: ceil(V / 16) * (K / 32) KiB = 2^32 bytes
    assert lib.lm_head_logprobs(*ok, 1, 1 << 22, 512, None) == INV
    assert b"32-bit offsets" in lib.llm_last_error()
    assert lib.lm_head_logprobs(*ok, -1, 10, 64, None) == INV


def test_logprob_rows_refusals():
    import llm_capi
    lib = llm_capi.load()
    INV = llm_capi.LLM_ERR_INVALID
    p = ctypes.c_void_p(16)

    def call(rows=2, V=100, chosen=p, top_n=3, clp=p, tlp=p, tid=p, logits=p):
        return lib.logprob_rows(logits, rows, V, chosen, top_n, clp, tlp, tid, None, None)

    assert call(rows=0) == 0
    for bad in (-1, 9):
        assert call(top_n=bad) == INV
        assert b"top_n" in lib.llm_last_error()
    assert call(V=0, top_n=0) == INV          # V < max(1, top_n)
    assert call(V=7, top_n=8) == INV
    assert call(V=65537) == INV
    assert b"65536" in lib.llm_last_error()
    assert call(logits=None) == INV
    assert call(clp=None) == INV              # chosen given: chosen_lp is required
    assert call(tlp=None) == INV              # top_n > 0: top_lp and top_id are required
    assert call(tid=None) == INV
    assert b"NULL" in lib.llm_last_error()


def test_decoder_entry_refusals():
    import llm_capi
    lib = llm_capi.load()
    INV = llm_capi.LLM_ERR_INVALID
    assert lib.llm_decoder_score(None, None, None, 1, 0, None) == INV
    assert lib.llm_decoder_serve_logprobs(None, None, None, None, None) == INV
    # the count is checked before the decoder is touched (a fake handle)
    d = ctypes.c_void_p(16)
    opt = llm_capi.LlmRequestOptions(max_new_tokens=1, eos_token=-1, temperature=0.0, top_k=0,
                                     top_p=1.0, seed=0)
    prompt = (ctypes.c_int32 * 1)(1)
    rid = ctypes.c_longlong(-1)
    for bad in (-1, 9):
        assert lib.llm_decoder_submit_logprobs(d, prompt, 1, ctypes.byref(opt), bad,
                                               ctypes.byref(rid)) == INV
        assert b"top_logprobs" in lib.llm_last_error()
    assert lib.llm_decoder_submit_logprobs(None, prompt, 1, ctypes.byref(opt), 0,
                                           ctypes.byref(rid)) == INV
    assert rid.value == -1


def test_pybind_surface():
    import llm_decoder
    for cls in (llm_decoder.CUDADecoder, llm_decoder.INT8Decoder):
        for m in ("score", "serve_logprobs", "submit", "generate_many"):
            assert hasattr(cls, m)
        assert "logprobs" in cls.submit.__doc__ and "logprobs" in cls.generate_many.__doc__
