"""INT8Decoder with 4-bit o_proj / fc1 / fc2 (set_weights(int4=True)) against
the oracle INT8 decoder given dec.expanded_weights(): a prefill of 40 tokens
per row, then 8 teacher-forced decode steps at the north_star bar (logits 1e-3
tensor-wide and elementwise, exact tokens), and the weight queries."""
import numpy as np
import pytest

from _fp8 import Pages, ref_decode
from _util import assert_parity, decoder_kv_at
from test_decoder_gpu import LOGIT_TOL, TIE_TOL, _int8_model, _Taps, _weights_dict

pytestmark = pytest.mark.gpu
PROMPT, STEPS = 40, 8


def _decoder(w, rows, kv_dtype, rope, **kw):
    import llm_decoder
    c = w["cfg"]
    dec = llm_decoder.INT8Decoder(c["L"], c["H"], c["D"], c["hid"], c["V"], c["max_seq"],
                                  max_batch=rows, kv_dtype=kv_dtype)
    dec.set_weights(_weights_dict(w), **kw)
    if rope:
        dec.set_rope(theta=10000.0)
    return dec


@pytest.mark.parametrize("rows,kv_dtype,rope", [
    (1, "float16", False), (17, "float16", False), (64, "float16", False),
    (17, "fp8", False), (17, "float16", True)])
def test_w4_decoder_matches_oracle_on_expanded_weights(gpu, oracle, rows, kv_dtype, rope):
    import torch
    from oracle.oracle import OracleDecoder
    w = _int8_model(oracle, L=2, H=4, D=64, V=300, S=64, seed=21)
    c = w["cfg"]
    L, V = c["L"], c["V"]
    dec = _decoder(w, rows, kv_dtype, rope, int4=True)
    w8 = dict(w, **dec.expanded_weights())
    for k in ("wo", "w1", "w2"):
        assert w8[k].shape == w[k].shape and np.abs(w8[k].astype(int) - w[k]).max() <= 9
    rng = np.random.default_rng(rows)
    prompts = [rng.integers(0, V, PROMPT).tolist() for _ in range(rows)]
    es = 1 if kv_dtype == "fp8" else 2

    def prefilled(d):
        d.begin_synthetic(rows, 0, 0, False)
        d.prefill_batch(list(range(rows)), prompts)
        pages = Pages(d, es)
        pool = pages.pool()
        return pages, [pages.context(pool, l, rows, PROMPT) for l in range(L)]

    # prompt chunks run the unfused launches with either weight type, so the
    # 4-bit decoder's pages equal, in every byte, an 8-bit decoder's on the
    # expanded weights
    _, ctx8 = prefilled(_decoder(w8, rows, kv_dtype, rope))
    pages, ctx = prefilled(dec)
    for l in range(L):
        np.testing.assert_array_equal(ctx[l], ctx8[l])

    odec = OracleDecoder(oracle, w8, rows)
    for l in range(L):
        for which in (0, 1):
            kv = ctx[l][which]
            kv = ref_decode(kv, 1.0).astype(np.float16) if es == 1 else kv.view(np.float16)
            odec.kv(l, which)[:rows, :, :PROMPT] = kv
    taps = _Taps(dec, w, rows)
    logits = torch.empty((rows, V), device="cuda")
    tok = rng.integers(0, V, rows).tolist()
    for s in range(STEPS):
        pos = np.full(rows, PROMPT + s, np.int32)
        g_next = dec.step(tok, logits_ptr=logits.data_ptr())
        torch.cuda.synchronize()
        fq, fs = taps.read(rows)
        if es == 1:
            kv = ref_decode(pages.at(pages.pool(), rows, pos, L), 1.0).astype(np.float16)
        else:
            kv = decoder_kv_at(dec, rows, pos, L)
        o_logits, o_next, stats, _ = odec.step_attn(np.array(tok, np.int32), pos, fq, fs,
                                                    forced_kv=kv)
        assert_parity(logits.cpu().numpy(), o_logits, LOGIT_TOL, axis=1, what=f"step {s} logits")
        # GEMM inputs downstream of the 4-bit GEMMs: LN2 (2), fc1 out (3), the
        # next LN1 (0); the attention output (1) too, except under rope, where
        # the oracle's own q is not rotated (tests/test_rope_decoder_gpu.py)
        st = stats[:, [0, 2, 3] if rope else [0, 1, 2, 3]]
        assert st[:, :, 1].max() <= 1 and st[:, :, 2].max() < 1e-5, (s, stats)
        for b in range(rows):
            if g_next[b] != o_next[b]:
                gap = o_logits[b][o_next[b]] - o_logits[b][g_next[b]]
                assert gap <= TIE_TOL * np.abs(o_logits[b]).max(), (s, b, gap)
        tok = list(g_next)


def test_w4_weight_queries(gpu, oracle, tmp_path):
    import llm_capi
    import llm_decoder
    lib = llm_capi.load()
    w = _int8_model(oracle, L=2, H=4, D=64, V=300, S=64, seed=21)
    c = w["cfg"]
    L, hid, inter = c["L"], c["hid"], c["inter"]
    qkv = lib.gemm_packed_bytes(llm_capi.LLM_I8, hid, 3 * hid)
    mats = [(hid, hid), (hid, inter), (inter, hid)]
    d4 = _decoder(w, 1, "float16", False, int4=True)
    assert d4.weight_bits() == 4
    assert d4.weight_bytes() == L * (qkv + sum(K * N // 2 + K * N // 128 for K, N in mats))
    d8 = _decoder(w, 1, "float16", False)
    assert d8.weight_bits() == 8
    assert d8.weight_bytes() == L * (qkv + sum(lib.gemm_packed_bytes(llm_capi.LLM_I8, K, N)
                                               for K, N in mats))
    with pytest.raises(RuntimeError):
        d8.expanded_weights()
    # the same model as an INT8 weight directory (weights/README.md), loaded
    # with int4=True: the 4-bit set that set_weights(int4=True) gives
    wd = _weights_dict(w)
    wd["emb"].view(np.float16).tofile(tmp_path / "embedding.f16")
    for l in range(L):
        p = tmp_path / f"layer_{l}"
        p.mkdir()
        np.concatenate([wd["ln1_g"][l], wd["ln1_b"][l]]).tofile(p / "ln1.bin")
        np.concatenate([wd["ln2_g"][l], wd["ln2_b"][l]]).tofile(p / "ln2.bin")
        np.concatenate([wd["b1"][l], wd["b2"][l]]).tofile(p / "mlp_biases.bin")
        for name, wk, sk in [("attn_wqkv", "wqkv", "sw_qkv"), ("attn_wo", "wo", "sw_o"),
                             ("mlp_fc1", "w1", "sw1"), ("mlp_fc2", "w2", "sw2")]:
            wd[wk][l].tofile(p / f"{name}.i8")
            wd[sk][l].tofile(p / f"{name}.scale")
    df = llm_decoder.INT8Decoder(L, c["H"], c["D"], hid, c["V"], c["max_seq"])
    df.load_quantized_weights(str(tmp_path), int4=True)
    assert df.weight_bits() == 4 and df.weight_bytes() == d4.weight_bytes()
    e4, ef = d4.expanded_weights(), df.expanded_weights()
    for k in ("wo", "w1", "w2"):
        np.testing.assert_array_equal(ef[k], e4[k])
    assert df.generate([7, 11, 13], 6) == d4.generate([7, 11, 13], 6)
