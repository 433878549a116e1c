"""Rotary position embedding, host side: llm_rope_table against the formula,
the argument checks of the four C entries (made on the host, before any device
call), and the numpy statement of the rotation (tests/_rope.py::rope_ref) that
the GPU tests hold the kernels to."""
import ctypes

import numpy as np
import pytest

from _rope import KvHistory, identity_table, rope_ref, stage1_stats, table_f64


def _table(theta, D, num_pos):
    import llm_capi
    return llm_capi.rope_table(theta, D, num_pos)


@pytest.mark.parametrize("theta,D,num_pos", [(10000.0, 64, 512), (10000.0, 128, 300),
                                             (500000.0, 128, 512), (2.5, 2, 40)])
def test_rope_table_matches_formula(theta, D, num_pos):
    got = _table(theta, D, num_pos)
    assert got.dtype == np.float32 and got.shape == (num_pos, D)
    ref = table_f64(theta, D, num_pos)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float(np.max(err / ulp))
    print(f"theta {theta} D {D}: worst error {worst:.3f} ulp")
    assert (err <= ulp).all(), worst
    # position 0: cos 1, sin 0, exactly
    np.testing.assert_array_equal(got[0], identity_table(1, D)[0])


def test_pybind_rope_table_is_the_c_entry():
    import llm_decoder
    a = llm_decoder.rope_table(10000.0, 64, 33)
    assert a.dtype == np.float32 and a.shape == (33, 64)
    np.testing.assert_array_equal(a, _table(10000.0, 64, 33))
    for cls in (llm_decoder.CUDADecoder, llm_decoder.INT8Decoder):
        assert hasattr(cls, "set_rope") and hasattr(cls, "rope")


def test_arguments_rejected_on_the_host():
    import llm_capi
    lib = llm_capi.load()
    INVALID = llm_capi.LLM_ERR_INVALID
    assert lib.llm_abi_version() == 3
    buf = np.zeros((4, 8), np.float32)
    p = buf.ctypes.data
    assert lib.llm_rope_table(10000.0, 8, 4, p) == 0
    assert lib.llm_rope_table(10000.0, 8, 4, None) == INVALID
    assert lib.llm_rope_table(10000.0, 7, 4, p) == INVALID      # odd head_dim
    assert b"even" in lib.llm_last_error()
    assert lib.llm_rope_table(10000.0, 0, 4, p) == INVALID
    assert lib.llm_rope_table(0.0, 8, 4, p) == INVALID          # theta <= 0
    assert lib.llm_rope_table(-3.0, 8, 4, p) == INVALID
    assert lib.llm_rope_table(float("nan"), 8, 4, p) == INVALID
    assert lib.llm_rope_table(10000.0, 8, 0, p) == INVALID      # num_pos >= 1
    # rope_rows: fake non-NULL pointers are rejected before anything is read
    one = ctypes.c_void_p(16)
    assert lib.rope_rows(None, 64, one, 1, 1, 64, one, 4, None) == INVALID
    assert lib.rope_rows(one, 64, None, 1, 1, 64, one, 4, None) == INVALID
    assert lib.rope_rows(one, 64, one, 1, 1, 64, None, 4, None) == INVALID
    assert lib.rope_rows(one, 63, one, 1, 1, 63, one, 4, None) == INVALID  # odd head_dim
    assert b"even" in lib.llm_last_error()
    assert lib.rope_rows(one, 64, one, 1, 2, 64, one, 4, None) == INVALID  # stride < H * D
    assert lib.rope_rows(one, 64, one, -1, 1, 64, one, 4, None) == INVALID
    assert lib.rope_rows(None, 64, None, 0, 1, 64, None, 4, None) == 0     # no rows: a no-op
    # the decoder entries on NULL
    assert lib.llm_decoder_set_rope(None, None) == INVALID
    assert lib.llm_decoder_set_rope(None, p) == INVALID
    assert lib.llm_decoder_rope(None) == -1


def test_rope_ref_properties():
    rng = np.random.default_rng(0)
    H, D, S = 3, 64, 50
    table = _table(10000.0, D, S)
    x = rng.standard_normal((S + 2, H * D)).astype(np.float32)
    pos = np.concatenate([np.arange(S), [S, -1]])
    y = rope_ref(x, pos, table)
    assert y.dtype == np.float32 and y.shape == x.shape
    # position 0 is the identity; positions outside the table are untouched bits
    np.testing.assert_array_equal(y[0].view(np.uint32), x[0].view(np.uint32))
    np.testing.assert_array_equal(y[S:].view(np.uint32), x[S:].view(np.uint32))
    assert not np.array_equal(y[1], x[1])
    # a rotation: every pair keeps its norm
    n0 = np.hypot(x[:, 0::2].astype(np.float64), x[:, 1::2].astype(np.float64))
    n1 = np.hypot(y[:, 0::2].astype(np.float64), y[:, 1::2].astype(np.float64))
    assert np.max(np.abs(n1 - n0) / np.maximum(n0, 1e-30)) < 1e-6
    # the table of -t (sin negated) undoes it
    inv = table.copy()
    inv[:, 1::2] = -inv[:, 1::2]
    back = rope_ref(y, pos, inv)
    assert np.max(np.abs(back - x)) < 1e-6 * np.max(np.abs(x)) * 4
    # the 3-d form [rows][H][D] is the same computation
    np.testing.assert_array_equal(rope_ref(x.reshape(-1, H, D), pos, table).reshape(x.shape), y)
    # written out for one pair
    t, d = 7, 10
    c, s = table[t, d], table[t, d + 1]
    assert y[t, d] == np.float32(x[t, d] * c) - np.float32(x[t, d + 1] * s)
    assert y[t, d + 1] == np.float32(x[t, d] * s) + np.float32(x[t, d + 1] * c)


def test_stage1_helper_reproduces_the_oracle_attention(oracle):
    """stage1_stats with no table restates the oracle decoder's own path from
    the stage-0 activations to the o_proj input: fed the oracle's own int8
    activations and K / V, it finds no difference at stage 1."""
    from oracle.oracle import OracleDecoder, synthetic_int8_model
    w = synthetic_int8_model(oracle, L=2, H=4, D=64, V=200, max_seq=40, seed=3)
    c = w["cfg"]
    B, hid, Kmax = 2, c["hid"], max(c["hid"], c["inter"])
    odec = OracleDecoder(oracle, w, B)
    hist = KvHistory(c["L"], B, c["H"], c["D"], c["max_seq"])
    rng = np.random.default_rng(1)
    for s in range(20):
        tok = rng.integers(0, 200, B).astype(np.int32)
        pos = np.full(B, s, np.int32)
        _, _, _, attn = odec.step_attn(tok, pos)
        kv = np.stack([np.stack([odec.kv(l, which)[:, :, s] for which in (0, 1)], axis=1)
                       for l in range(c["L"])])  # [L][B][2][H][D]
        hist.append(kv, pos)
        # the oracle's own activations: stage 0 from its LayerNorm of the
        # embedding (layer 0 only), stage 1 from its attention output
        fq = np.zeros((c["L"], 4, B, Kmax), np.int8)
        fs = np.ones((c["L"], 4, B), np.float32)
        a0 = oracle.layer_norm(w["emb"][tok].astype(np.float32), w["ln1_g"][0], w["ln1_b"][0])
        fq[0, 0, :, :hid], fs[0, 0] = oracle.quantize_rows(a0)
        fq[0, 1, :, :hid], fs[0, 1] = oracle.quantize_rows(attn[0])
        _, stats = stage1_stats(oracle, w, fq, fs, hist, s, table=None, layers=[0])
        assert stats[0, 0] == 0 and stats[0, 2] == 0, (s, stats)
