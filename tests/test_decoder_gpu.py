"""Decoder-level parity: the HIP INT8Decoder / CUDADecoder (pybind11
`llm_decoder`, over the C ABI) against the restated INT8Decoder oracle.

Every kernel of the step is held to its own bar elsewhere (int32 GEMM
accumulators and epilogues bit-exact, row quantiser bit-exact, attention 1e-7
rel).  A whole step is not bit-exact: LayerNorm / softmax reduce in a different
fp32 order (~1e-7 rel), and once in a while that moves an activation across an
int8 rounding boundary (one LSB = 1/127 of the row's absmax, ~0.5 % of a layer
output; scripts/debug_layer.py).

The parity tests therefore run TEACHER-FORCED at the int8 activations
(llm_decoder_set_taps + OracleDecoder.step_forced): after every GPU step the
four int8 GEMM inputs of every layer are read back; the oracle quantises its own
fp32 values, counts where they differ from the GPU's (one LSB at most, rare),
and continues from the GPU's.  A flip can then not propagate, and the step is
held to the north_star bar:
  * logits within LOGIT_TOL = 1e-3 rel (max-abs error / max-abs logit) at every
    step — measured ~1e-6;
  * tokens exact: a GPU token may differ from the oracle's argmax only where the
    oracle's top two logits are within TIE_TOL = 1e-5 of the logit scale (a tie
    at fp32 noise level);
  * int8 activations: every GPU value within one LSB of the oracle's, flips
    below 1e-3 of all values.
The free-running tests (no forcing: prompts, generate, prefill) let flips
propagate and are held to FREE_RUN_TOL: the measured drift of these tests
(round 6, profiles/r06/free_run_generate.jsonl: 1.75e-2 random tokens at C1
dims, 1.66e-2 lockstep at d 128, 1.2e-2 / 0.94e-2 prefill against token by
token) plus a margin.  That drift is the INT8 decoder's own: the oracle
against itself with only its summation order reversed drifts 2.3e-2 at C1
dims (tests/test_generate_free_run.py); test_generate_free_run_gpu.py holds
free-running generate to that yardstick."""
import numpy as np
import pytest

from _util import assert_parity, decoder_kv_at, decoder_kv_to_oracle, record, rel_err

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-3
TIE_TOL = 1e-5
FREE_RUN_TOL = 2.5e-2


def _torch():
    import torch
    return torch


def _int8_model(oracle, L=2, H=4, D=64, V=1000, S=64, seed=1234):
    from oracle.oracle import synthetic_int8_model
    return synthetic_int8_model(oracle, L=L, H=H, D=D, V=V, max_seq=S, seed=seed)


def _weights_dict(w):
    d = {k: np.ascontiguousarray(v) for k, v in w.items() if k != "cfg"}
    d["emb"] = w["emb"].view(np.uint16)
    return d


def _make_gpu_decoder(w, max_batch, cls="INT8Decoder"):
    import llm_decoder
    c = w["cfg"]
    dec = getattr(llm_decoder, cls)(c["L"], c["H"], c["D"], c["hid"], c["V"], c["max_seq"],
                                    max_batch=max_batch)
    dec.set_weights(_weights_dict(w))
    return dec


def _random_tokens(dec, odec, steps, B, V, seed):
    """Random tokens every step (no feedback), free running: drift bound."""
    torch = _torch()
    dec.begin_synthetic(B, 0, 0, False)
    logits = torch.empty((B, V), device="cuda")
    rng = np.random.default_rng(seed)
    worst = 0.0
    for s in range(steps):
        tok = [int(t) for t in rng.permutation(V)[:B]]
        g_next = dec.step(tok, logits_ptr=logits.data_ptr())
        torch.cuda.synchronize()
        _, o_logits, o_next = odec.step(np.array(tok, np.int32), np.full(B, s, np.int32))
        gl = logits.cpu().numpy()
        worst = max(worst, rel_err(gl, o_logits))
        for b in range(B):
            if g_next[b] != o_next[b]:
                gap = o_logits[b][o_next[b]] - o_logits[b][g_next[b]]
                assert gap <= FREE_RUN_TOL * np.abs(o_logits[b]).max()
    return worst


def _lockstep(dec, odec, prompts, gen, V):
    """Step GPU and oracle together; returns (gpu tokens per row, #near ties, max logit rel err)."""
    torch = _torch()
    B = len(prompts)
    steps = max(len(p) for p in prompts) + gen - 1
    dec.begin_synthetic(B, 0, 0, False)  # fresh rows at position 0
    logits = torch.empty((B, V), device="cuda")
    out = [[] for _ in range(B)]
    nxt = [0] * B
    ties = 0
    worst = 0.0
    for s in range(steps):
        tok = [p[s] if s < len(p) else nxt[b] for b, p in enumerate(prompts)]
        g_next = dec.step(tok, logits_ptr=logits.data_ptr())
        torch.cuda.synchronize()
        _, o_logits, o_next = odec.step(np.array(tok, np.int32), np.full(B, s, np.int32))
        gl = logits.cpu().numpy()
        worst = max(worst, rel_err(gl, o_logits))
        for b in range(B):
            if g_next[b] != o_next[b]:
                top = np.sort(o_logits[b])[-2:]
                scale = np.abs(o_logits[b]).max()
                gap = o_logits[b][o_next[b]] - o_logits[b][g_next[b]]
                assert gap <= FREE_RUN_TOL * scale, (s, b, g_next[b], o_next[b], gap, top)
                ties += 1
            if s >= len(prompts[b]) - 1 and len(out[b]) < gen:
                out[b].append(g_next[b])
        nxt = list(g_next)
    return out, ties, worst


class _Taps:
    """Device buffers of llm_decoder_set_taps and their host unpacking into the
    oracle's forced-activation layout [L][4][B][max(hid, inter)]."""

    def __init__(self, dec, w, max_batch):
        torch = _torch()
        c = w["cfg"]
        self.L, self.hid, self.inter = c["L"], c["hid"], c["inter"]
        self.K = max(self.hid, self.inter)
        self.b16 = (max_batch + 15) // 16 * 16
        self.maxB = max_batch
        self.q = torch.zeros(self.L * 4 * self.b16 * self.K, dtype=torch.int8, device="cuda")
        self.s = torch.zeros(self.L * 4 * max_batch, dtype=torch.float32, device="cuda")
        dec.set_taps(self.q.data_ptr(), self.s.data_ptr())

    def read(self, B):
        from oracle.oracle import unpack_a_i8
        q = self.q.cpu().numpy().reshape(self.L, 4, self.b16 * self.K)
        s = self.s.cpu().numpy().reshape(self.L, 4, self.maxB)
        fq = np.zeros((self.L, 4, B, self.K), np.int8)
        for l in range(self.L):
            for st in range(4):
                Kst = self.inter if st == 3 else self.hid
                fq[l, st, :, :Kst] = unpack_a_i8(q[l, st, :self.b16 * Kst], B, Kst)
        return fq, np.ascontiguousarray(s[:, :, :B])


def _forced_lockstep(dec, odec, taps, prompts, gen, V):
    """Step the GPU (taps on) and the teacher-forced oracle together; prompts
    are fed one token per step, then each row's own (GPU) next token.  Holds
    every step to LOGIT_TOL / TIE_TOL; returns (tokens per row, worst logit
    error, int8 values compared, int8 values that differed)."""
    torch = _torch()
    B = len(prompts)
    steps = max(len(p) for p in prompts) + gen - 1
    dec.begin_synthetic(B, 0, 0, False)
    logits = torch.empty((B, V), device="cuda")
    out = [[] for _ in range(B)]
    nxt = [0] * B
    worst, n_vals, n_flips = 0.0, 0, 0
    for s in range(steps):
        tok = [p[s] if s < len(p) else nxt[b] for b, p in enumerate(prompts)]
        g_next = dec.step(tok, logits_ptr=logits.data_ptr())
        torch.cuda.synchronize()
        fq, fs = taps.read(B)
        o_logits, o_next, stats = odec.step_forced(np.array(tok, np.int32),
                                                   np.full(B, s, np.int32), fq, fs)
        gl = logits.cpu().numpy()
        err = rel_err(gl, o_logits)
        assert err < LOGIT_TOL, (s, err)
        assert_parity(gl, o_logits, LOGIT_TOL, axis=1, what=f"step {s} logits")
        worst = max(worst, err)
        assert stats[:, :, 1].max() <= 1, (s, stats)        # at most one int8 LSB
        assert stats[:, :, 2].max() < 1e-5, (s, stats)      # row scales agree
        n_flips += int(stats[:, :, 0].sum())
        n_vals += B * taps.L * (3 * taps.hid + taps.inter)
        for b in range(B):
            if g_next[b] != o_next[b]:
                gap = o_logits[b][o_next[b]] - o_logits[b][g_next[b]]
                assert gap <= TIE_TOL * np.abs(o_logits[b]).max(), (s, b, gap)
            if s >= len(prompts[b]) - 1 and len(out[b]) < gen:
                out[b].append(g_next[b])
        nxt = list(g_next)
    return out, worst, n_vals, n_flips


def test_int8_decoder_matches_oracle_c1(gpu, oracle):
    """C1 model dims (2 layers, 4 heads, d=64, tile 16), ragged prompts, 46
    teacher-forced steps at the north_star bar (logits 1e-3, exact tokens)."""
    from oracle.oracle import OracleDecoder
    w = _int8_model(oracle, L=2, H=4, D=64, V=1000, S=64)
    dec = _make_gpu_decoder(w, max_batch=3)
    taps = _Taps(dec, w, 3)
    rng = np.random.default_rng(0)
    prompts = [list(rng.integers(0, 1000, n)) for n in (5, 17, 1)]
    out, worst, n_vals, n_flips = _forced_lockstep(dec, OracleDecoder(oracle, w, 3), taps,
                                                   prompts, gen=30, V=1000)
    assert all(len(o) == 30 for o in out)
    assert n_flips < 1e-3 * n_vals, (n_flips, n_vals)
    print(f"C1 forced lockstep: worst logit rel err {worst:.2e}, int8 flips {n_flips}/{n_vals}")
    # free running (no taps): the same decoder, flips allowed to propagate
    dec.set_taps(0, 0)
    drift = _random_tokens(dec, OracleDecoder(oracle, w, 3), 40, 3, 1000, seed=1)
    record("free_run", test="c1_random_tokens", step_drift_worst=drift)
    assert drift < FREE_RUN_TOL, drift


def test_int8_decoder_larger_heads(gpu, oracle):
    """D=128 heads, several pages per row, a row crossing page boundaries;
    teacher forced over 69 steps."""
    from oracle.oracle import OracleDecoder
    w = _int8_model(oracle, L=2, H=2, D=128, V=512, S=96, seed=7)
    dec = _make_gpu_decoder(w, max_batch=2)
    taps = _Taps(dec, w, 2)
    rng = np.random.default_rng(1)
    prompts = [list(rng.integers(0, 512, 40)), list(rng.integers(0, 512, 3))]
    _, worst, n_vals, n_flips = _forced_lockstep(dec, OracleDecoder(oracle, w, 2), taps,
                                                 prompts, gen=30, V=512)
    assert n_flips < 1e-3 * n_vals, (n_flips, n_vals)
    dec.set_taps(0, 0)
    _, ties, worst_free = _lockstep(dec, OracleDecoder(oracle, w, 2), prompts, gen=30, V=512)
    record("free_run", test="d128_lockstep", step_drift_worst=worst_free, id_differences=ties)
    assert worst_free < FREE_RUN_TOL, worst_free


def test_generate_after_set_sampling_is_greedy(gpu, oracle):
    """generate is greedy argmax (sample_from_logits, decoder/cuda_decoder.cu:
    7-14) even after set_sampling; the sampling mode still applies to step."""
    w = _int8_model(oracle, L=1, H=2, D=64, V=300, S=48, seed=3)
    dec = _make_gpu_decoder(w, max_batch=2)
    prompt = [3, 14, 15, 92]
    greedy = dec.generate(prompt, 10, 1.0)
    dec.set_sampling(1.5, 0, 1.0, 123)
    assert dec.generate(prompt, 10, 1.0) == greedy
    assert dec.generate(prompt, 10, 0.5) == greedy
    # step still samples: at temperature 1.5 over 300 tokens, 16 draws are
    # not all the argmax of their own step's logits
    torch = _torch()
    logits = torch.empty((2, 300), device="cuda")
    dec.begin_synthetic(2, 0, 0, False)
    tok, differ = [5, 6], 0
    for _ in range(8):
        tok = dec.step(tok, logits_ptr=logits.data_ptr(), want_next=True)
        torch.cuda.synchronize()
        differ += int((np.asarray(tok) != logits.cpu().numpy().argmax(1)).sum())
    assert differ > 0


def test_generate_call_forms(gpu, oracle):
    w = _int8_model(oracle, L=1, H=2, D=64, V=300, S=48, seed=3)
    dec = _make_gpu_decoder(w, max_batch=4)
    prompt = [3, 14, 15, 92]
    r1 = dec.generate(prompt, 10, 1.0)               # bindings.cpp:8-15 form
    assert r1[:4] == prompt and len(r1) == 14
    out = []
    assert dec.generate(prompt, out, 10, 0.7) is None  # api/router.py:23 form
    assert out == r1                                   # temperature does not move argmax
    out2 = []
    dec.generate(prompt, out2, max_gen_len=10, temperature=1.0)  # cli/chat_cli.py:24 form
    assert out2 == r1
    rb = dec.generate_batch([prompt, [7], prompt], 10)
    assert rb[0] == r1 and rb[2] == r1 and rb[1][:1] == [7] and len(rb[1]) == 11
    with pytest.raises(RuntimeError):
        dec.generate([5000], 3)  # token id out of range
    with pytest.raises(RuntimeError):
        dec.generate(prompt, 100)  # beyond max_seq_len


def test_weight_files_roundtrip(gpu, oracle, tmp_path):
    """fp32 .bin directory (weights/README.md layout) -> quantize_weights ->
    load_quantized_weights gives the same decoder as quantising in-process."""
    import llm_decoder
    rng = np.random.default_rng(5)
    L, H, D, V, S = 2, 2, 64, 200, 40
    hid, inter = H * D, 4 * H * D
    fp = tmp_path / "fp32"
    (fp).mkdir()
    emb = rng.standard_normal((V, hid)).astype(np.float32)
    emb.tofile(fp / "embedding.bin")
    mats = {}
    for l in range(L):
        p = fp / f"layer_{l}"
        p.mkdir()
        g = {}
        for nm, shp in [("attn_wq", (hid, hid)), ("attn_wk", (hid, hid)), ("attn_wv", (hid, hid)),
                        ("attn_wo", (hid, hid)), ("mlp_fc1", (hid, inter)), ("mlp_fc2", (inter, hid))]:
            g[nm] = (0.02 * rng.standard_normal(shp)).astype(np.float32)
            g[nm].tofile(p / f"{nm}.bin")
        for nm in ("ln1", "ln2"):
            g[nm] = np.concatenate([1 + 0.1 * rng.standard_normal(hid),
                                    0.1 * rng.standard_normal(hid)]).astype(np.float32)
            g[nm].tofile(p / f"{nm}.bin")
        g["bias"] = (0.02 * rng.standard_normal(inter + hid)).astype(np.float32)
        g["bias"].tofile(p / "mlp_biases.bin")
        mats[l] = g
    d1 = llm_decoder.INT8Decoder(L, H, D, hid, V, S)
    d1.quantize_weights(str(fp), str(tmp_path / "int8"))
    d1.load_quantized_weights(str(tmp_path / "int8"))
    d2 = llm_decoder.INT8Decoder(L, H, D, hid, V, S)
    d2.load_weights(str(fp))  # quantise-on-load path
    # in-process reference weights through the oracle quantiser
    w = {"cfg": dict(L=L, H=H, D=D, hid=hid, inter=inter, V=V, max_seq=S),
         "emb": emb.astype(np.float16)}
    for key in ("ln1_g", "ln1_b", "ln2_g", "ln2_b"):
        which, part = key[:3], key[-1]
        w[key] = np.stack([mats[l][which][:hid] if part == "g" else mats[l][which][hid:]
                           for l in range(L)]).astype(np.float32)
    def qcols(name_list, K, N):
        qs, ss = [], []
        for l in range(L):
            wf = np.concatenate([mats[l][n] for n in name_list], axis=1)
            q, s = oracle.quantize_cols(wf)
            qs.append(q); ss.append(s)
        return np.stack(qs), np.stack(ss)
    w["wqkv"], w["sw_qkv"] = qcols(["attn_wq", "attn_wk", "attn_wv"], hid, 3 * hid)
    w["wo"], w["sw_o"] = qcols(["attn_wo"], hid, hid)
    w["w1"], w["sw1"] = qcols(["mlp_fc1"], hid, inter)
    w["w2"], w["sw2"] = qcols(["mlp_fc2"], inter, hid)
    w["b1"] = np.stack([mats[l]["bias"][:inter] for l in range(L)])
    w["b2"] = np.stack([mats[l]["bias"][inter:] for l in range(L)])
    d3 = _make_gpu_decoder(w, max_batch=1)
    prompt = [1, 2, 3, 4, 5]
    r1, r2, r3 = d1.generate(prompt, 12), d2.generate(prompt, 12), d3.generate(prompt, 12)
    assert r1 == r3 and r2 == r3


def _f16_model(rng, L, H, D, V, S):
    hid, inter = H * D, 4 * H * D
    w = {"cfg": dict(L=L, H=H, D=D, hid=hid, inter=inter, V=V, max_seq=S)}
    w["emb"] = rng.standard_normal((V, hid)).astype(np.float16)
    for k in ("ln1_g", "ln2_g"):
        w[k] = (1 + 0.1 * rng.standard_normal((L, hid))).astype(np.float32)
    for k in ("ln1_b", "ln2_b"):
        w[k] = (0.1 * rng.standard_normal((L, hid))).astype(np.float32)
    w["wqkv"] = (0.02 * rng.standard_normal((L, hid, 3 * hid))).astype(np.float16)
    w["wo"] = (0.02 * rng.standard_normal((L, hid, hid))).astype(np.float16)
    w["w1"] = (0.02 * rng.standard_normal((L, hid, inter))).astype(np.float16)
    w["w2"] = (0.02 * rng.standard_normal((L, inter, hid))).astype(np.float16)
    w["b1"] = (0.02 * rng.standard_normal((L, inter))).astype(np.float32)
    w["b2"] = (0.02 * rng.standard_normal((L, hid))).astype(np.float32)
    return w


def _f16_reference_logits(w, tokens_per_step, oracle):
    """float64 reference of the CUDADecoder step (fp16 weights, fp16-rounded
    GEMM inputs, fp16 KV), contiguous KV cache."""
    c = w["cfg"]
    L, H, D, hid = c["L"], c["H"], c["D"], c["hid"]
    B = len(tokens_per_step[0])
    kc = [np.zeros((B, H, 0, D)) for _ in range(L)]
    vc = [np.zeros((B, H, 0, D)) for _ in range(L)]
    f16 = lambda a: np.asarray(a, np.float32).astype(np.float16).astype(np.float64)
    all_logits = []
    for tok in tokens_per_step:
        x = w["emb"][np.array(tok)].astype(np.float64)
        for l in range(L):
            a = oracle.layer_norm(x.astype(np.float32), w["ln1_g"][l], w["ln1_b"][l])
            qkv = f16(a) @ w["wqkv"][l].astype(np.float64)
            q = qkv[:, :hid].reshape(B, H, D)
            kc[l] = np.concatenate([kc[l], f16(qkv[:, hid:2 * hid]).reshape(B, H, 1, D)], axis=2)
            vc[l] = np.concatenate([vc[l], f16(qkv[:, 2 * hid:]).reshape(B, H, 1, D)], axis=2)
            s = np.einsum("bhd,bhtd->bht", q, kc[l])
            p = np.exp(s - s.max(-1, keepdims=True))
            p /= p.sum(-1, keepdims=True) + 1e-6
            o = np.einsum("bht,bhtd->bhd", p, vc[l]).reshape(B, hid)
            x = f16(o) @ w["wo"][l].astype(np.float64)
            a2 = oracle.layer_norm(x.astype(np.float32), w["ln2_g"][l], w["ln2_b"][l])
            h = np.maximum(f16(a2) @ w["w1"][l].astype(np.float64) + w["b1"][l], 0)
            x = f16(h) @ w["w2"][l].astype(np.float64) + w["b2"][l]
        all_logits.append(x @ w["emb"].astype(np.float64).T)
    return all_logits


@pytest.mark.parametrize("H,S", [(2, 40), (12, 40), (12, 512)])
def test_cuda_decoder_fp16_vs_oracle(gpu, oracle, H, S):
    """CUDADecoder (fp16 weights, fp16 GEMM inputs, fp16 KV) against the
    oracle's restated CUDADecoder step (oracle.cpp f16_gemm path), 24 steps of
    ragged prompts then fed-back tokens, TEACHER FORCED at the four fp16 GEMM
    inputs (taps) and at the K / V each step appends (read back from the
    pages): an fp32 reduction-order difference can move an activation
    across an fp16 rounding boundary (one ulp, 2^-11 relative), which free
    running lets propagate to ~5e-4 of the logit scale; forced, every step is
    held to the north_star bar -- logits within LOGIT_TOL tensor-normalised
    AND elementwise per row, fp16 inputs within one ulp (< 1e-3 differing),
    tokens exact unless the oracle's top two are within TIE_TOL.  A free-running
    pass (no taps) is then held to LOGIT_TOL tensor-normalised, and a float64
    numpy restatement (_f16_reference_logits) to the same.  H 12 is C2's width
    (hid 768, inter 3072).  S 512 gives the attention 4 splits, so it runs in
    the workgroup-merge form (splits past a short row's tiles empty); S 40 is a
    single-split launch."""
    torch = _torch()
    import llm_decoder
    from oracle.oracle import OracleDecoder, unpack_a_f16
    rng = np.random.default_rng(9)
    L, D, V = 2, 64, 300
    w = _f16_model(rng, L, H, D, V, S)
    c = w["cfg"]
    hid, inter = c["hid"], c["inter"]
    dec = llm_decoder.CUDADecoder(L, H, D, hid, V, S, max_batch=2)
    d = {k: np.ascontiguousarray(v) for k, v in w.items() if k != "cfg"}
    for k in ("emb", "wqkv", "wo", "w1", "w2"):
        d[k] = d[k].view(np.uint16)
    dec.set_weights(d)
    Kmax, b16 = max(hid, inter), 16
    tq = torch.zeros(L * 4 * b16 * Kmax * 2, dtype=torch.int8, device="cuda")
    ts_ = torch.zeros(L * 4 * 2, dtype=torch.float32, device="cuda")
    dec.set_taps(tq.data_ptr(), ts_.data_ptr())

    def read_forced():
        q = tq.cpu().numpy().view(np.uint16).reshape(L, 4, b16 * Kmax)
        fh = np.zeros((L, 4, 2, Kmax), np.float16)
        for l in range(L):
            for st in range(4):
                Kst = inter if st == 3 else hid
                fh[l, st, :, :Kst] = unpack_a_f16(q[l, st, :b16 * Kst], 2, Kst)
        return fh

    prompts = [rng.integers(0, V, 7).tolist(), rng.integers(0, V, 2).tolist()]
    logits = torch.empty((2, V), device="cuda")

    def lockstep(forced):
        odec = OracleDecoder(oracle, w, 2)
        dec.begin_synthetic(2, 0, 0, False)
        nxt, seen, worst, flips = [0, 0], [], 0.0, 0
        for s_ in range(24):
            tok = [p[s_] if s_ < len(p) else nxt[b] for b, p in enumerate(prompts)]
            g_next = dec.step(tok, logits_ptr=logits.data_ptr())
            torch.cuda.synchronize()
            if forced:
                ol, on, stats, _ = odec.step_attn(np.array(tok, np.int32), np.full(2, s_, np.int32),
                                                  read_forced(),
                                                  forced_kv=decoder_kv_at(dec, 2, [s_, s_], L))
                assert stats[:, :, 1].max() <= 1, (s_, stats)
                assert odec.kv_stats[:, 1].max() <= 1, (s_, odec.kv_stats)
                flips += int(stats[:, :, 0].sum())
            else:
                _, ol, on = odec.step(np.array(tok, np.int32), np.full(2, s_, np.int32))
            gl = logits.cpu().numpy()
            worst = max(worst, rel_err(gl, ol))
            assert rel_err(gl, ol) < LOGIT_TOL, (forced, s_, rel_err(gl, ol))
            if forced:
                assert_parity(gl, ol, LOGIT_TOL, axis=1, what=f"step {s_} logits")
            for b in range(2):
                if g_next[b] != on[b]:
                    assert ol[b][on[b]] - ol[b][g_next[b]] <= TIE_TOL * np.abs(ol[b]).max()
            seen.append(tok)
            nxt = list(g_next)
        return seen, worst, flips

    seen, worst, flips = lockstep(True)
    # an fp16 rounding boundary is 2^-11 of the value apart (int8: 1/127 of the
    # row's absmax), so an fp32 reordering of ~1e-6 relative flips ~1e-3 of the
    # values; each flip is held to one ulp above, the rate to < 1e-2
    assert flips < 1e-2 * 24 * 2 * L * (3 * hid + inter), flips
    dec.set_taps(0, 0)
    lockstep(False)
    ref = _f16_reference_logits(w, seen[:6], oracle)
    dec.begin_synthetic(2, 0, 0, False)
    for s_, tok in enumerate(seen[:6]):
        dec.step(tok, logits_ptr=logits.data_ptr())
        torch.cuda.synchronize()
        assert rel_err(logits.cpu().numpy(), ref[s_]) < LOGIT_TOL
    print(f"fp16 decoder H {H} S {S}: forced worst logit rel err {worst:.2e}, fp16 flips {flips}")


def test_synthetic_long_context_step(gpu, oracle):
    """begin_synthetic: shuffled pages, random KV at context 500.  The KV is
    read back from the pool through the page table into the oracle, and two
    steps (the second feeding back the device's own ids, tokens = None) match
    the teacher-forced oracle at the north_star bar."""
    torch = _torch()
    from oracle.oracle import OracleDecoder
    w = _int8_model(oracle, L=1, H=2, D=128, V=256, S=600, seed=11)
    dec = _make_gpu_decoder(w, max_batch=2)
    taps = _Taps(dec, w, 2)
    dec.begin_synthetic(2, 500, 123, True)
    assert dec.context_len(0) == 500
    odec = OracleDecoder(oracle, w, 2)
    decoder_kv_to_oracle(dec, odec, 2, 500)
    logits = torch.empty((2, 256), device="cuda")
    tok = [5, 6]
    for s in range(2):
        nxt = dec.step(tok if s == 0 else None, logits_ptr=logits.data_ptr())
        torch.cuda.synchronize()
        assert dec.context_len(1) == 501 + s
        fq, fs = taps.read(2)
        o_logits, o_next, stats = odec.step_forced(np.array(tok, np.int32),
                                                   np.full(2, 500 + s, np.int32), fq, fs)
        assert stats[:, :, 1].max() <= 1 and stats[:, :, 2].max() < 1e-5, stats
        assert_parity(logits.cpu().numpy(), o_logits, LOGIT_TOL, axis=1, what=f"step {s}")
        for b in range(2):
            if nxt[b] != o_next[b]:
                gap = o_logits[b][o_next[b]] - o_logits[b][nxt[b]]
                assert gap <= TIE_TOL * np.abs(o_logits[b]).max(), (s, b, gap)
        tok = list(nxt)


def test_int8_flip_rate(gpu, oracle):
    """The only divergence source between GPU and oracle steps: int8 rounding
    flips after fp32 reductions.  On 64 rows x 2048 activations they must be
    rare (< 1e-4) and never more than one LSB."""
    import llm_capi
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((64, 2048)) * 1.3 + 0.2).astype(np.float32)
    g = (1 + 0.1 * rng.standard_normal(2048)).astype(np.float32)
    b = (0.1 * rng.standard_normal(2048)).astype(np.float32)
    _, q, _ = llm_capi.layernorm_quant(_torch().from_numpy(x).cuda(), _torch().from_numpy(g).cuda(),
                                       _torch().from_numpy(b).cuda())
    qr, _ = oracle.quantize_rows(oracle.layer_norm(x, g, b))
    d = np.abs(q.cpu().numpy().astype(np.int32) - qr.astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 1e-4


def test_beam_decode_forked_prefix(gpu, oracle):
    """llm_decoder_begin_beams: 2 sequences x 4 beams over one forked prefix
    (beam_len 0, so every beam of a sequence holds the SAME context through
    shared pages).  Fed the same token, the beams of a sequence must produce
    bitwise identical logits (beam-aware attention, copy-on-write append into
    the first private tile), sequences differ, and the page pool holds one
    prefix copy per sequence plus the beams' private append tiles."""
    torch = _torch()
    w = _int8_model(oracle, L=2, H=4, D=64, V=500, S=128, seed=9)
    dec = _make_gpu_decoder(w, max_batch=8)
    seqs, W, prefix = 2, 4, 40  # 2.5 tiles shared: the partial 3rd tile is copied on write
    dec.begin_beams(seqs, W, prefix, 0, 3, True)
    V = w["cfg"]["V"]
    logits = torch.empty((seqs * W, V), device="cuda")
    for step in range(3):
        dec.step([11, 11, 11, 11, 7, 7, 7, 7] if step == 0 else None, logits_ptr=logits.data_ptr())
        torch.cuda.synchronize()
        lg = logits.cpu().numpy()
        assert np.isfinite(lg).all()
        for sq in range(seqs):
            for b in range(1, W):
                np.testing.assert_array_equal(lg[sq * W + b], lg[sq * W])
        assert not np.array_equal(lg[0], lg[W])
    assert dec.context_len(0) == prefix + 3


def test_decoder_device_sampling(gpu, oracle):
    """llm_decoder_set_sampling: the step graph draws with sample_rows at each
    row's position (draw counter) — the next ids equal the oracle sampler on
    the step's own logits; temperature 0 restores greedy argmax."""
    torch = _torch()
    from oracle.oracle import sample_rows
    w = _int8_model(oracle, L=2, H=4, D=64, V=700, S=64, seed=4)
    dec = _make_gpu_decoder(w, max_batch=4)
    V = w["cfg"]["V"]
    dec.set_sampling(0.8, 40, 0.9, 77)
    dec.begin_synthetic(4, 0, 0, False)
    logits = torch.empty((4, V), device="cuda")
    toks = [3, 1, 4, 1]
    for s in range(4):
        nxt = dec.step(toks, logits_ptr=logits.data_ptr(), want_next=True)
        torch.cuda.synchronize()
        ref, margin = sample_rows(logits.cpu().numpy(), 0.8, 40, 0.9, seed=77, counter=s)
        ok = (np.asarray(nxt) == ref) | (margin < 1e-4)
        assert ok.all(), (s, nxt, ref, margin)
        toks = list(map(int, nxt))
    dec.set_sampling(0.0, 0, 1.0, 0)
    nxt = dec.step(toks, logits_ptr=logits.data_ptr(), want_next=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(np.asarray(nxt), logits.cpu().numpy().argmax(1))


def _prefill_vs_stepping(make, prompts, V):
    """(token-by-token logits per row, prefill+step logits, prefill+step ids)
    A: the prompt one token per decode step (rows in their own decoders once
    their prompt ends); B: prefill all but the last token, then one step."""
    torch = _torch()
    lens = [len(p) for p in prompts]
    logits_a = [None] * len(prompts)
    for r, p in enumerate(prompts):
        a = make(1)
        a.begin_synthetic(1, 0, 0, False)
        la = torch.empty((1, V), device="cuda")
        for t in p:
            a.step([t], logits_ptr=la.data_ptr())
        torch.cuda.synchronize()
        logits_a[r] = la[0].cpu().numpy().copy()
    b = make(len(prompts))
    b.begin_synthetic(len(prompts), 0, 0, False)
    for r, p in enumerate(prompts):
        b.prefill(r, p[:-1])
    lb = torch.empty((len(prompts), V), device="cuda")
    nxt = b.step([p[-1] for p in prompts], logits_ptr=lb.data_ptr(), want_next=True)
    torch.cuda.synchronize()
    for r in range(len(prompts)):
        assert b.context_len(r) == lens[r]  # tokens now in the row's KV
    return logits_a, lb.cpu().numpy(), nxt


def test_prefill_matches_token_by_token(gpu, oracle):
    """Chunked prefill (one layer pass per <= 512-token chunk, causal attention
    on the MFMA prefill kernel) leaves the same KV and state as feeding the
    prompt one token per decode step; prompts of 600 (two chunks) and 37
    tokens, ragged.  The prefill kernel's attention agrees with the decode
    kernel to ~1e-6 (tests/test_pa_prefill_gpu.py); through the int8
    activations that is the free-running bar of this file (FREE_RUN_TOL)."""
    w = _int8_model(oracle, L=2, H=4, D=64, V=500, S=1024, seed=12)
    V = w["cfg"]["V"]
    rng = np.random.default_rng(3)
    prompts = [rng.integers(0, V, 600).tolist(), rng.integers(0, V, 37).tolist()]
    la, lb, nxt = _prefill_vs_stepping(lambda n: _make_gpu_decoder(w, max_batch=n), prompts, V)
    errs = [rel_err(lb[r], la[r]) for r in range(2)]
    gaps = [float((la[r].max() - la[r][nxt[r]]) / np.abs(la[r]).max()) for r in range(2)]
    record("free_run", test="prefill_vs_token_by_token_int8", logit_err=errs, id_gap_rel=gaps)
    for r in range(2):
        assert errs[r] < FREE_RUN_TOL, (r, errs[r])
        assert gaps[r] <= FREE_RUN_TOL, (r, gaps[r])


def test_prefill_decode_kernel_fallback(gpu, oracle):
    """Head dims the MFMA prefill kernel does not take (D = 256) prefill
    through the decode kernel, one row per prompt token (beam_ids = the row,
    context_lens = p0 + i + 1).  Against stepping the prompt token by token the
    attention split order and the fp32 order of the GEMM-fused LayerNorm differ
    (~1e-7): the fp16 CUDADecoder (no int8 rounding to amplify it) holds both paths to
    LOGIT_TOL of the oracle's restated step and to each other within twice that
    (fp16 activation roundings flip independently in the two paths); the
    INT8Decoder, where such a difference can flip an int8 activation, to
    FREE_RUN_TOL."""
    import llm_decoder
    rng = np.random.default_rng(4)
    L, H, D, V, S = 2, 2, 256, 400, 700
    wf = _f16_model(rng, L, H, D, V, S)
    d = {k: np.ascontiguousarray(v) for k, v in wf.items() if k != "cfg"}
    for k in ("emb", "wqkv", "wo", "w1", "w2"):
        d[k] = d[k].view(np.uint16)

    def make_f16(n):
        dec = llm_decoder.CUDADecoder(L, H, D, H * D, V, S, max_batch=n)
        dec.set_weights(d)
        return dec

    prompts = [rng.integers(0, V, 530).tolist(), rng.integers(0, V, 9).tolist()]
    la, lb, nxt = _prefill_vs_stepping(make_f16, prompts, V)
    from oracle.oracle import OracleDecoder
    for r in range(2):
        # both paths against the oracle's restated step over the same prompt
        od = OracleDecoder(oracle, wf, 1)
        for i, t in enumerate(prompts[r]):
            _, ol, _ = od.step(np.array([t], np.int32), np.array([i], np.int32))
        # free running (prefill chunks are not tapped): tensor-normalised bound
        assert rel_err(la[r], ol[0]) < LOGIT_TOL, (r, "stepping", rel_err(la[r], ol[0]))
        assert rel_err(lb[r], ol[0]) < LOGIT_TOL, (r, "prefill", rel_err(lb[r], ol[0]))
        assert rel_err(lb[r], la[r]) < 2 * LOGIT_TOL, (r, rel_err(lb[r], la[r]))
        assert la[r].max() - la[r][nxt[r]] <= LOGIT_TOL * np.abs(la[r]).max()
    w = _int8_model(oracle, L=2, H=2, D=256, V=400, S=700, seed=13)
    la, lb, nxt = _prefill_vs_stepping(lambda n: _make_gpu_decoder(w, max_batch=n), prompts, V)
    errs = [rel_err(lb[r], la[r]) for r in range(2)]
    gaps = [float((la[r].max() - la[r][nxt[r]]) / np.abs(la[r]).max()) for r in range(2)]
    record("free_run", test="prefill_decode_kernel_fallback_int8", logit_err=errs, id_gap_rel=gaps)
    for r in range(2):
        assert errs[r] < FREE_RUN_TOL, (r, errs[r])
        assert gaps[r] <= FREE_RUN_TOL, (r, gaps[r])


def test_prefill_mfma_fp16_decoder(gpu, oracle):
    """The FP16 CUDADecoder has no int8 rounding steps, so the MFMA prefill
    stays within 1e-3 rel of token-by-token stepping (fp16 activation
    roundings are 2^-11 and rarely move)."""
    import llm_decoder
    rng = np.random.default_rng(4)
    L, H, D, V, S = 2, 4, 64, 300, 700
    w = _f16_model(rng, L, H, D, V, S)
    c = w["cfg"]
    d = {k: np.ascontiguousarray(v) for k, v in w.items() if k != "cfg"}
    for k in ("emb", "wqkv", "wo", "w1", "w2"):
        d[k] = d[k].view(np.uint16)

    def make(n):
        dec = llm_decoder.CUDADecoder(L, H, D, c["hid"], V, S, max_batch=n)
        dec.set_weights(d)
        return dec

    prompts = [rng.integers(0, V, 530).tolist(), rng.integers(0, V, 20).tolist()]
    la, lb, nxt = _prefill_vs_stepping(make, prompts, V)
    for r in range(2):
        assert rel_err(lb[r], la[r]) < 1e-3, (r, rel_err(lb[r], la[r]))
        gap = la[r].max() - la[r][nxt[r]]
        assert gap <= 1e-3 * np.abs(la[r]).max()


def test_forced_step_48_rows(gpu, oracle):
    """48 rows (three 16-row packed-A tiles) against the oracle, teacher forced
    at the int8 activations, north_star bar."""
    from oracle.oracle import OracleDecoder
    w = _int8_model(oracle, L=2, H=4, D=64, V=600, S=32, seed=31)
    dec = _make_gpu_decoder(w, max_batch=48)
    taps = _Taps(dec, w, 48)
    rng = np.random.default_rng(2)
    prompts = [list(rng.integers(0, 600, 5)) for _ in range(48)]
    _, _, n_vals, n_flips = _forced_lockstep(dec, OracleDecoder(oracle, w, 48), taps, prompts,
                                             gen=3, V=600)
    assert n_flips < 1e-3 * n_vals


@pytest.mark.parametrize("rows", [24, 40, 48])
def test_forced_hidden_2048_tile_forms(gpu, oracle, rows):
    """hid 2048: the LayerNorms are launches (the rows' fp32 image is too big
    for the GEMM prologue).  At 40 / 48 rows o_proj and fc2 run 2-column-tile
    16-row workgroups (three row blocks, the last one partial at 40; round 2
    ran split-K here); at 24 rows the GEMMs take the narrow 16-row tiles (two
    row blocks, 4-wave workgroups for K < 4096).  o_proj quantises the
    attention's fp32 rows in its prologue at every one of these row counts
    (the tapped stage-1 A).  Teacher forced, north_star bar."""
    from oracle.oracle import OracleDecoder
    w = _int8_model(oracle, L=2, H=16, D=128, V=512, S=24, seed=41)
    dec = _make_gpu_decoder(w, max_batch=rows)
    taps = _Taps(dec, w, rows)
    rng = np.random.default_rng(5)
    prompts = [list(rng.integers(0, 512, 3)) for _ in range(rows)]
    _, worst, n_vals, n_flips = _forced_lockstep(dec, OracleDecoder(oracle, w, rows), taps,
                                                 prompts, gen=4, V=512)
    assert n_flips < 1e-3 * n_vals, (n_flips, n_vals)


def _tied_vocab_decoder(oracle, cls, hid_heads, rows):
    """A one-layer decoder whose embedding (and tied LM head) repeats 7 rows:
    emb[v] = base[v % 7], so every logit row holds 7 distinct values, each
    shared bit for bit by ~143 tokens spread over the whole vocabulary."""
    V, D = 1000, 64
    rng = np.random.default_rng(hid_heads + rows)
    if cls == "INT8Decoder":
        from oracle.oracle import synthetic_int8_model
        w = synthetic_int8_model(oracle, L=1, H=hid_heads, D=D, V=V, max_seq=16, seed=3,
                                 fast=hid_heads > 8)
    else:
        w = _f16_model(rng, 1, hid_heads, D, V, 16)
    base = rng.standard_normal((7, hid_heads * D)).astype(np.float16)
    w["emb"] = np.ascontiguousarray(base[np.arange(V) % 7])
    return w, _make_gpu_decoder(w, max_batch=rows, cls=cls)


@pytest.mark.parametrize("cls,heads,rows", [
    ("INT8Decoder", 2, 1), ("INT8Decoder", 2, 17), ("INT8Decoder", 2, 33),
    ("CUDADecoder", 2, 1), ("CUDADecoder", 2, 17), ("CUDADecoder", 2, 33),
    ("INT8Decoder", 36, 1),  # hid 2304 > 2048: lm_head_kernel<1, 16, 1>
])
def test_greedy_ties_through_lm_head(gpu, oracle, cls, heads, rows):
    """Greedy decode takes its token from the LM head's fused partial maxima
    (lm_head_* kernels + argmax_partials_kernel), not from argmax_rows: with
    the step's maximum logit shared bit for bit by ~143 tokens across lanes,
    waves, vocabulary tiles and workgroups, the first of them wins, in the
    1-, 2- and 4-row-tile forms (rows 1 / 17 / 33)."""
    torch = _torch()
    V = 1000
    w, dec = _tied_vocab_decoder(oracle, cls, heads, rows)
    dec.begin_synthetic(rows, 0, 0, False)
    logits = torch.empty((rows, V), device="cuda")
    tok = [(3 * r + 1) % V for r in range(rows)]
    for step in range(2):
        nxt = np.asarray(dec.step(tok, logits_ptr=logits.data_ptr(), want_next=True))
        torch.cuda.synchronize()
        lg = logits.cpu().numpy()
        assert np.isfinite(lg).all()
        bits = lg.view(np.uint32)
        for r in range(rows):
            tied = np.nonzero(bits[r] == bits[r, np.argmax(lg[r])])[0]
            # precondition: the maximum is shared by one whole residue class
            assert len(tied) in (142, 143) and len(set(tied % 7)) == 1, (r, len(tied))
            assert tied[-1] > V - 8  # up to the last vocabulary tile and workgroup
        want = np.argmax(lg, axis=1)  # first maximum
        assert (want < 7).all()
        np.testing.assert_array_equal(nxt, want)
        tok = [int(t) + 7 * (r % 100) for r, t in enumerate(nxt)]  # same embedding, other ids
