"""Packed prefill in the decoder (llm_decoder_prefill_rows, dec.prefill_batch,
dec.packed_prefill): the prompts of several rows through shared layer passes
of <= 512 packed tokens, against the per-row prefill of the same prompts; each
followed by one decode step whose logits, ids and context lengths are compared
(the pattern of tests/test_decoder_gpu.py::_prefill_vs_stepping).

Bars, restated from the project's: FREE_RUN_TOL = 2.5e-2 for INT8 weights (a
last-bit difference may flip an int8 activation), 1e-3 for fp16 weights.

Short regime (every prompt's prefilled part ends within 64 positions): every
attention is one pass, where the packed kernel's result does not depend on the
tile's other queries; the int8 GEMMs are exact and every other stage is
row-wise, so packed and per-row agree bit for bit."""
import numpy as np
import pytest

from _fp8 import f16_model, make_decoder

pytestmark = pytest.mark.gpu
FREE_RUN_TOL = 2.5e-2
F16_TOL = 1e-3
SHORT = (2, 17, 33, 64, 65, 9)
RAGGED = (600, 37, 1, 513, 200)


def _rel_err(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _int8_model(oracle, *, H=4, D=64, V=500, S=128, seed=12):
    from oracle.oracle import synthetic_int8_model
    return synthetic_int8_model(oracle, L=2, H=H, D=D, V=V, max_seq=S, seed=seed)


def _prompts(V, lens, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, V, n).tolist() for n in lens]


def _run(make, prompts, V, packed):
    """Prefill all but each prompt's last token (packed: one prefill_batch over
    all rows; else row by row), then one step: (logits, next ids, context lens)."""
    import torch
    n = len(prompts)
    dec = make(n)
    dec.begin_synthetic(n, 0, 0, False)
    if packed:
        dec.prefill_batch(list(range(n)), [p[:-1] for p in prompts])
    else:
        for r, p in enumerate(prompts):
            if len(p) > 1:
                dec.prefill(r, p[:-1])
    assert [dec.context_len(r) for r in range(n)] == [len(p) - 1 for p in prompts]
    lg = torch.empty((len(prompts), V), device="cuda")
    nxt = dec.step([p[-1] for p in prompts], logits_ptr=lg.data_ptr(), want_next=True)
    torch.cuda.synchronize()
    ctx = [dec.context_len(r) for r in range(len(prompts))]
    assert ctx == [len(p) for p in prompts]
    return lg.cpu().numpy(), list(nxt), ctx


def _both(make, prompts, V):
    return _run(make, prompts, V, packed=False), _run(make, prompts, V, packed=True)


@pytest.mark.parametrize("kv", ["float16", "fp8"])
def test_short_regime_is_bit_equal(gpu, oracle, kv):
    w = _int8_model(oracle)
    V = w["cfg"]["V"]
    (la, ia, ca), (lb, ib, cb) = _both(lambda n: make_decoder(w, n, kv_dtype=kv),
                                       _prompts(V, SHORT), V)
    np.testing.assert_array_equal(lb, la)
    assert ib == ia and cb == ca


def test_ragged_several_passes_int8(gpu, oracle):
    """1,346 prefilled tokens in three passes: row 0 continues from pass 1 into
    pass 2, row 3 from pass 2 into pass 3, row 2 has nothing to prefill."""
    w = _int8_model(oracle, S=1024)
    V = w["cfg"]["V"]
    (la, ia, _), (lb, ib, _) = _both(lambda n: make_decoder(w, n, kv_dtype="float16"),
                                     _prompts(V, RAGGED), V)
    for r in range(len(RAGGED)):
        err = _rel_err(lb[r], la[r])
        gap = float((la[r].max() - la[r][ib[r]]) / np.abs(la[r]).max())
        print(f"row {r}: logit err {err:.3e}, id gap {gap:.3e}")
        assert err < FREE_RUN_TOL, (r, err)
        assert gap <= FREE_RUN_TOL, (r, gap)


def test_ragged_several_passes_fp16(gpu):
    rng = np.random.default_rng(4)
    V = 300
    w = f16_model(rng, 2, 4, 64, V, 1024)
    (la, ia, _), (lb, ib, _) = _both(
        lambda n: make_decoder(w, n, kv_dtype="float16", cls="CUDADecoder"),
        _prompts(V, RAGGED), V)
    for r in range(len(RAGGED)):
        err = _rel_err(lb[r], la[r])
        gap = float((la[r].max() - la[r][ib[r]]) / np.abs(la[r]).max())
        print(f"row {r}: logit err {err:.3e}, id gap {gap:.3e}")
        assert err < F16_TOL, (r, err)
        assert gap <= F16_TOL, (r, gap)


def test_decode_kernel_fallback(gpu, oracle):
    """D = 256: the packed pass's attention is the decode kernel over the per-row
    page-table rows and context lengths."""
    w = _int8_model(oracle, H=2, D=256, V=400, S=128, seed=13)
    V = w["cfg"]["V"]
    prompts = _prompts(V, (40, 9))
    make = lambda n: make_decoder(w, n, kv_dtype="float16")
    assert make(1).prefill_kernel == "decode"
    (la, ia, _), (lb, ib, _) = _both(make, prompts, V)
    for r in range(2):
        err = _rel_err(lb[r], la[r])
        gap = float((la[r].max() - la[r][ib[r]]) / np.abs(la[r]).max())
        print(f"row {r}: logit err {err:.3e}, id gap {gap:.3e}")
        assert err < FREE_RUN_TOL, (r, err)
        assert gap <= FREE_RUN_TOL, (r, gap)


def test_switch_generate_and_beam_search(gpu, oracle):
    w = _int8_model(oracle)
    V = w["cfg"]["V"]
    prompts = _prompts(V, SHORT)
    dec = make_decoder(w, 2 * len(prompts), kv_dtype="float16")
    assert dec.packed_prefill is False
    gen_off = dec.generate_batch(prompts, 6)
    beam_off = dec.beam_search_batch(prompts, beam_width=2, max_new_tokens=5)
    one_off = dec.generate(prompts[2], 4, 1.0)
    dec.packed_prefill = True
    assert dec.packed_prefill is True
    assert dec.generate_batch(prompts, 6) == gen_off
    assert dec.beam_search_batch(prompts, beam_width=2, max_new_tokens=5) == beam_off
    assert dec.generate(prompts[2], 4, 1.0) == one_off
    (ids, score), = dec.beam_search(prompts[1], beam_width=1, max_new_tokens=4)
    dec.packed_prefill = False
    assert dec.packed_prefill is False
    assert dec.beam_search(prompts[1], beam_width=1, max_new_tokens=4) == [(ids, score)]
    assert dec.generate_batch(prompts, 6) == gen_off


def test_errors_move_no_row(gpu, oracle):
    w = _int8_model(oracle, S=64)
    V = w["cfg"]["V"]
    dec = make_decoder(w, 4, kv_dtype="float16")
    dec.begin_synthetic(3, 0, 0, False)
    dec.prefill_batch([0, 2], [[1, 2, 3], [4] * 20])
    ctx = [dec.context_len(r) for r in range(3)]
    assert ctx == [3, 0, 20]
    bad = {
        "repeated row": ([0, 1, 0], [[1], [2], [3]]),
        "inactive row": ([1, 3], [[1], [2]]),
        "token id >= V": ([0, 1], [[1, 2], [3, V]]),
        "past max_seq_len": ([1, 2], [[1], [5] * 44]),   # 20 + 44 = max_seq_len
    }
    for name, (rows, toks) in bad.items():
        with pytest.raises(RuntimeError):
            dec.prefill_batch(rows, toks)
        assert [dec.context_len(r) for r in range(3)] == ctx, name
    with pytest.raises(ValueError):
        dec.prefill_batch([0, 1], [[1]])
    dec.prefill_batch([1, 2], [[1], [5] * 43])   # the longest that fits
    assert [dec.context_len(r) for r in range(3)] == [3, 1, 63]
