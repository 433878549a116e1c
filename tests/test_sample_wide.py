"""CPU checks of the streaming token-choice entries (csrc/sample_wide.hip):
sample_rows_wide, sample_rows_each_wide and logprob_rows_wide are declared,
exported and prototyped, and refuse bad arguments on the host with their own
name in llm_last_error (fake pointers: nothing is dereferenced or launched)."""
import ctypes

import pytest

P = ctypes.c_void_p(16)


def _sample(lib, logits=P, rows=2, V=100, top_k=0, top_p=1.0, out=P):
    return lib.sample_rows_wide(logits, rows, V, 1.0, top_k, top_p, 0, 0, out, None)


def _each(lib, logits=P, rows=2, V=100, out=P, **_):
    return lib.sample_rows_each_wide(logits, rows, V, None, None, None, None, None, out, None)


def _logprob(lib, logits=P, rows=2, V=100, top_n=3, out=P, **_):
    return lib.logprob_rows_wide(logits, rows, V, P, top_n, out, out, out, None, None)


@pytest.mark.parametrize("call", [_sample, _each, _logprob], ids=lambda f: f.__name__)
def test_wide_entries_refuse_on_the_host(call):
    import llm_capi
    lib = llm_capi.load()
    name = {_sample: b"sample_rows_wide", _each: b"sample_rows_each_wide",
            _logprob: b"logprob_rows_wide"}[call]
    assert name.decode() in llm_capi.declared_symbols()
    bad = [dict(logits=None), dict(out=None), dict(rows=-1), dict(V=0), dict(V=(1 << 20) + 1)]
    if call is _sample:
        bad += [dict(top_p=0.0), dict(top_k=-1)]
    if call is _logprob:
        bad += [dict(top_n=9), dict(top_n=-1), dict(V=2, top_n=3)]
    for kw in bad:
        assert call(lib, **kw) == llm_capi.LLM_ERR_INVALID, kw
        assert lib.llm_last_error().startswith(name + b":"), (kw, lib.llm_last_error())
    assert call(lib, rows=0) == llm_capi.LLM_OK
    assert call(lib, rows=0, V=1 << 20) == llm_capi.LLM_OK
