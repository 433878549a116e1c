"""The decoder's gated MLP (llm_decoder_set_mlp): 2-layer INT8 and FP16
decoders (hid 128, 2 heads of 64, inter 320 -- the decoder takes multiples of
64 only) in gated_silu with taps on.

From tap stage 2 (the gated kernel's input) and the weights, numpy computes H
in float64 and, for INT8, quantises it by the project's rule: tap stage 3 must
match within 1 LSB, at most 1 % of the elements off by it, the row scales to
1e-6 (the fp32 numpy restatement is held to the same cap beside it, so the cap
is reachable at this seed).  FP16: stage 3 is fp16(H) within one ulp, at most
1 % off.  The step's logits are held to float64 fc2 + LM head from the tapped
fc2 input at test_decoder_gpu.py's teacher-forced bar, and the same step after
a 20-token prefill of row 0 to the prompt stepped token by token."""
import numpy as np
import pytest

from _util import rel_err

pytestmark = pytest.mark.gpu
L, H, D, HID, INTER, V, S, B = 2, 2, 64, 128, 320, 300, 64, 3
LOGIT_TOL = 1e-3


def _model(kind, oracle):
    from oracle.oracle import synthetic_int8_model
    rng = np.random.default_rng(31)
    if kind == "i8":
        w = synthetic_int8_model(oracle, L=L, H=H, D=D, V=V, max_seq=S, seed=31, inter=INTER)
        ups = [oracle.quantize_cols((0.05 * rng.standard_normal((HID, INTER))).astype(np.float32))
               for _ in range(L)]
        w["w_up"] = np.stack([u[0] for u in ups])
        w["sw_up"] = np.stack([u[1] for u in ups]).astype(np.float32)
    else:
        w = {"cfg": dict(L=L, H=H, D=D, hid=HID, inter=INTER, V=V, max_seq=S)}
        w["emb"] = rng.standard_normal((V, HID)).astype(np.float16)
        for k in ("ln1_g", "ln2_g"):
            w[k] = (1 + 0.1 * rng.standard_normal((L, HID))).astype(np.float32)
        for k in ("ln1_b", "ln2_b", "b1", "b2"):
            n = INTER if k == "b1" else HID
            w[k] = (0.1 * rng.standard_normal((L, n))).astype(np.float32)
        for k, (kk, n) in dict(wqkv=(HID, 3 * HID), wo=(HID, HID), w1=(HID, INTER),
                               w2=(INTER, HID), w_up=(HID, INTER)).items():
            w[k] = (0.05 * rng.standard_normal((L, kk, n))).astype(np.float16)
    w["b_up"] = (0.1 * rng.standard_normal((L, INTER))).astype(np.float32)
    return w


def _decoder(kind, w, mlp, max_batch=B):
    import llm_decoder
    dec = getattr(llm_decoder, "INT8Decoder" if kind == "i8" else "CUDADecoder")(
        L, H, D, HID, V, S, max_batch=max_batch, inter_dim=INTER)
    if mlp:
        dec.set_mlp(mlp)
    d = {k: np.ascontiguousarray(v) for k, v in w.items() if k != "cfg"}
    if mlp in (None, "plain"):
        for k in ("w_up", "sw_up", "b_up"):
            d.pop(k, None)
    for k in ("emb",) + (() if kind == "i8" else ("wqkv", "wo", "w1", "w2", "w_up")):
        if k in d:
            d[k] = d[k].view(np.uint16)
    dec.set_weights(d)
    return dec


def _silu_gate(G, U, f):
    return G / (f(1) + np.exp(-G)) * U


def _quantise(h):
    """The project's row quantiser on float64 values: (q, 1 / scale)."""
    scale = 127.0 / (np.abs(h).max(axis=1, keepdims=True) + 1e-6)
    y = h * scale
    return np.clip(np.sign(y) * np.floor(np.abs(y) + 0.5), -128, 127), 1.0 / scale[:, 0]


@pytest.mark.parametrize("kind", ["i8", "f16"])
def test_gated_decoder_taps_and_logits(gpu, oracle, kind):
    import torch
    from oracle.oracle import unpack_a_f16, unpack_a_i8
    w = _model(kind, oracle)
    dec = _decoder(kind, w, "gated_silu")
    assert dec.mlp == "gated_silu"
    i8 = kind == "i8"
    es, b16 = (1 if i8 else 2), 16
    tq = torch.zeros(L * 4 * b16 * INTER * es, dtype=torch.int8, device="cuda")
    ts = torch.zeros(L * 4 * B, dtype=torch.float32, device="cuda")
    dec.set_taps(tq.data_ptr(), ts.data_ptr())
    rng = np.random.default_rng(5)
    prompt = rng.integers(0, V, 20).tolist()
    last = rng.integers(0, V, B).tolist()
    logits = torch.empty((B, V), device="cuda")
    dec.begin_synthetic(B, 0, 0, False)
    dec.prefill(0, prompt)
    dec.step(last, logits_ptr=logits.data_ptr())
    torch.cuda.synchronize()
    gl = logits.cpu().numpy()

    raw = tq.cpu().numpy()
    raw = (raw if i8 else raw.view(np.uint16)).reshape(L, 4, b16 * INTER)
    sc = ts.cpu().numpy().reshape(L, 4, B).astype(np.float64)
    unpack = unpack_a_i8 if i8 else unpack_a_f16
    for l in range(L):
        a2 = unpack(raw[l, 2, :b16 * HID], B, HID)
        a3 = unpack(raw[l, 3, :b16 * INTER], B, INTER)
        w1, wu = w["w1"][l], w["w_up"][l]
        if i8:
            ag, au = (a2.astype(np.int64) @ m.astype(np.int64) for m in (w1, wu))
            sg, su = (sc[l, 2].astype(np.float32)[:, None] * w[k][l][None, :]
                      for k in ("sw1", "sw_up"))
            h64 = _silu_gate(ag * sg.astype(np.float64) + w["b1"][l],
                             au * su.astype(np.float64) + w["b_up"][l], np.float64)
            h32 = _silu_gate(ag.astype(np.float32) * sg + w["b1"][l],
                             au.astype(np.float32) * su + w["b_up"][l], np.float32)
            q, inv = _quantise(h64)
            for name, got in (("fp32 numpy", _quantise(h32.astype(np.float64))[0]),
                              ("device", a3.astype(np.float64))):
                d = np.abs(got - q)
                print(f"layer {l} {name}: max LSB {d.max():.0f}, off {np.mean(d > 0):.4%}")
                assert d.max() <= 1 and np.mean(d > 0) <= 0.01, (l, name)
            np.testing.assert_allclose(sc[l, 3], inv, rtol=1e-6)
        else:
            g, u = (a2.astype(np.float64) @ m.astype(np.float64) for m in (w1, wu))
            ref = _silu_gate(g + w["b1"][l], u + w["b_up"][l], np.float64).astype(np.float16)
            d = np.abs(a3.astype(np.float64) - ref.astype(np.float64))
            print(f"layer {l} fp16: off {np.mean(d > 0):.4%}")
            assert (d <= np.spacing(np.abs(ref)).astype(np.float64)).all(), l
            assert np.mean(d > 0) <= 0.01, l
    # fc2 + LM head in float64 from the tapped fc2 input of the last layer
    x = a3.astype(np.float64) * (sc[L - 1, 3][:, None] if i8 else 1.0)
    x = x @ w["w2"][L - 1].astype(np.float64) * (w["sw2"][L - 1] if i8 else 1.0) + w["b2"][L - 1]
    assert rel_err(gl, x @ w["emb"].astype(np.float64).T) < LOGIT_TOL

    # row 0's prompt stepped token by token (16-row form) against its prefill
    dec.set_taps(0, 0)
    dec.begin_synthetic(B, 0, 0, False)
    for t in prompt:
        dec.step([t, 0, 0])
    dec.step(last, logits_ptr=logits.data_ptr())
    torch.cuda.synchronize()
    assert rel_err(logits.cpu().numpy()[0], gl[0]) < LOGIT_TOL


def test_gated_decoder_paths_and_setter_rules(gpu, oracle):
    """set_mlp("plain") is the decoder that never called set_mlp, bit for bit;
    generate_many (serving, packed prefill, the step graph) returns generate's
    ids; and the setter's state rules."""
    import torch
    import llm_capi
    w = _model("i8", oracle)
    logits = [torch.empty((B, V), device="cuda") for _ in range(2)]
    for mlp, lg in zip((None, "plain"), logits):
        dec = _decoder("i8", w, mlp)
        dec.begin_synthetic(B, 0, 0, False)
        for s in range(3):
            dec.step([7 + s, 100, 250], logits_ptr=lg.data_ptr())
        torch.cuda.synchronize()
    assert torch.equal(logits[0].view(torch.int32), logits[1].view(torch.int32))
    with pytest.raises(RuntimeError, match="before the weights"):
        _decoder("i8", w, None).set_mlp("gated_silu")  # weights are loaded

    gated = _decoder("i8", w, "gated_gelu", max_batch=4)
    prompts = [[5, 9, 200], list(range(40, 61)), [17]]
    many = gated.generate_many(prompts, 6)
    assert many == [gated.generate(p, 6)[len(p):] for p in prompts]
    assert gated.weight_bytes() == _decoder("i8", w, None).weight_bytes() + L * HID * INTER
    gated.begin_synthetic(1, 0, 0, False)
    with pytest.raises(RuntimeError, match="rows are active"):
        gated.set_mlp("plain")

    # the up matrix missing: every entry that would start rows is refused
    bare = _decoder("i8", {k: v for k, v in w.items() if k not in ("w_up", "sw_up", "b_up")},
                    "gated_silu")
    for start in (lambda: bare.begin_synthetic(1, 0, 0, False), lambda: bare.generate([1, 2], 2),
                  lambda: bare.serve_begin(), lambda: bare.generate_many([[1]], 1)):
        with pytest.raises(RuntimeError, match="up matrix"):
            start()
    lib = llm_capi.load()
    d = {k: np.ascontiguousarray(v) for k, v in w.items() if k != "cfg"}
    d["emb"] = d["emb"].view(np.uint16)
    with pytest.raises(RuntimeError, match="4-bit weights with a gated MLP"):
        bare.set_weights(d, int4=True)
    assert b"4-bit weights" in lib.llm_last_error()
