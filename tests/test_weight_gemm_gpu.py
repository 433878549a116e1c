"""The decoder's weight_gemm (csrc/gemm.hip) in every fused form, kernel by kernel.

Through weight_gemm_tune of the tuning build (csrc/tune/gemm_tune.hip), which
forwards a plain-C struct to llm::weight_gemm itself: the LayerNorm prologue
(I8 and F16, x rows and embedding rows), the quantising prologue of o_proj, the
two-slice atomic fc2 (ksplit2), the packed fp16 output (C16), the KV append
epilogue (fp16 and FP8 pools, the rows remap, c_cols < N) and the activation
taps, on and off.  Through f16_gemm and f16_gemm_tune: the FP16 GEMM on
integer-valued operands, where fp32 accumulation is exact in any order.

Every comparison is bit for bit (int8 GEMMs against the oracle, the taps
against the LayerNorm / quantisation launches, fused outputs against the same
launch's plain outputs) except the FP16 LayerNorm-prologue product, which is
held to the fp32 dot-product bound derived in test_ln_prologue_f16.  Output
buffers are pre-filled with NaN or a sentinel byte and carry guard margins;
what a launch must not write is compared with the pre-fill.

test_every_launchable_form_is_reached asserts, through gemm_form_tune (the
form function launch_gemm dispatches on), that the shapes of this file reach
every kernel instantiation the product library can launch."""
import ctypes
import functools

import numpy as np
import pytest

from _util import record

pytestmark = pytest.mark.gpu

F16, I8, FP8 = 0, 1, 4  # llm_dtype
EPS = 1e-5
SENTINEL = 0x5A
GUARD = 256  # bytes before and after every output buffer


@pytest.fixture(scope="module")
def tune(gpu):
    import llm_capi
    return llm_capi.load_tune()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pad16(rows):
    return (rows + 15) // 16 * 16


class Buf:
    """A device output buffer holding `prefill` (any dtype / shape) between two
    guard margins of SENTINEL bytes.  read() returns what the device holds now,
    in prefill's dtype and shape, after asserting the margins are intact."""

    def __init__(self, prefill):
        self.before = np.ascontiguousarray(prefill)
        guard = np.full(GUARD, SENTINEL, np.uint8)
        self.t = _dev(np.concatenate([guard, self.before.view(np.uint8).ravel(), guard]))

    def data_ptr(self):
        return self.t.data_ptr() + GUARD

    def read(self):
        h = self.t.cpu().numpy()
        assert (h[:GUARD] == SENTINEL).all() and (h[-GUARD:] == SENTINEL).all(), "guard written"
        return h[GUARD:-GUARD].view(self.before.dtype).reshape(self.before.shape)

    def untouched(self):
        return np.array_equal(self.read().view(np.uint8), self.before.view(np.uint8))


def _nan(*shape):
    return Buf(np.full(shape, np.nan, np.float32))


def _sentinel(nbytes):
    return Buf(np.full(nbytes, SENTINEL, np.uint8))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same_bits(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


def _wg(tune, **fields):
    """One weight_gemm_tune call (device tensors / Bufs / None for pointers);
    returns its status after the stream has drained."""
    import torch
    import llm_capi
    a = llm_capi.WeightGemmTuneArgs()
    a.ln_eps = EPS
    a.kv_k_inv_scale = a.kv_v_inv_scale = 1.0
    names = {n for n, _ in a._fields_}
    for k, v in fields.items():
        assert k in names, k
        setattr(a, k, v.data_ptr() if hasattr(v, "data_ptr") else v)
    st = tune.weight_gemm_tune(ctypes.byref(a), llm_capi.stream_ptr())
    torch.cuda.synchronize()
    return st


def _form(tune, dtype, M, N, K, pro=0, ksplit2=0, nt=0, waves=0, mrows=0):
    """(MT, NT, waves launched, k slices, prologue) launch_gemm picks."""
    out = (ctypes.c_int32 * 5)()
    assert tune.gemm_form_tune(dtype, M, N, K, pro, ksplit2, nt, waves, mrows, out) == 0
    return tuple(out)


def _matmul_exact(A, W):
    """Integer product through float64 BLAS: exact while |sum| < 2^53."""
    return (A.astype(np.float64) @ W.astype(np.float64)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _weights(dtype, K, N):
    """(W, packed W on the device, sw, bias, device sw, device bias), one draw per shape."""
    import llm_capi
    rng = np.random.default_rng(K * 31 + N + dtype)
    if dtype == I8:
        W = rng.integers(-127, 128, (K, N), dtype=np.int8)
    else:
        W = (0.05 * rng.standard_normal((K, N))).astype(np.float16)
    sw = rng.uniform(1e-3, 1e-2, N).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    return W, llm_capi.pack_weights(_dev(W), dtype), sw, bias, _dev(sw), _dev(bias)


def _packed_a(A, dtype):
    """A [M][K] in packed-A order on the device (gemm_pack_weights of A^T)."""
    import llm_capi
    return llm_capi.pack_weights(_dev(np.ascontiguousarray(A.T)), dtype)


def _a_offsets(rows, K, dtype):
    """Element offsets of A[m][k] in packed-A order (csrc/common.hpp a_frag_off_*)."""
    per, sh = (64, 4) if dtype == I8 else (32, 3)  # k per step, log2(k per lane)
    m = np.arange(rows)[:, None]
    k = np.arange(K)[None, :]
    lane = (m & 15) + 16 * ((k & (per - 1)) >> sh)
    return ((((m >> 4) * (K // per) + k // per) * 64 + lane) << sh) + (k & ((1 << sh) - 1))


def _pack_rows(vals, dtype):
    """What a sentinel-filled packed-A buffer holds once rows `vals` [M][K] are
    stored and nothing else: bytes [pad16(M) * K * esize]."""
    M, K = vals.shape
    es = 1 if dtype == I8 else 2
    out = np.full(_pad16(M) * K * es, SENTINEL, np.uint8).view(np.int8 if dtype == I8 else np.uint16)
    out[_a_offsets(M, K, dtype).ravel()] = vals.view(out.dtype).ravel()
    return out.view(np.uint8)


# ---------------------------------------------------------------------------
# Shapes.  test_every_launchable_form_is_reached reads these same lists.
# ---------------------------------------------------------------------------
def _ln_rows(M):
    return 16 if M <= 16 else 32 if M <= 32 else 64


def _ln_fits(M, K):
    """ln_fusable's 64 KB of fp32 rows per workgroup (the LDS image is smaller
    at every K used here)."""
    return _ln_rows(M) * K * 4 <= 64 * 1024


LN_M = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)  # 65: a second, one-row row block
LN_I8_K, LN_F16_K = (256, 512, 1024), (128, 256, 512)
# N = 48 (I8; 64 for F16, whose C16 needs N % 32 == 0), and N = 6144 for two column tiles
LN_I8_CASES = [(M, K, 48) for K in LN_I8_K for M in LN_M if _ln_fits(M, K)] + \
    [(17, 512, 6144), (64, 256, 6144)]
LN_F16_CASES = [(M, K, 64) for K in LN_F16_K for M in LN_M if _ln_fits(M, K)] + \
    [(17, 512, 6144), (64, 256, 6144)]

QP_K = (256, 1792, 2048)  # one, seven and all eight float4 chunks per lane
QP_M = (1, 16, 17, 32, 33, 40, 64)
QP_CASES = [(M, K, 256) for K in QP_K for M in QP_M] + [(40, K, 2048) for K in QP_K]

KSPLIT_KS = (16, 17, 33)
KSPLIT_M = (1, 16, 24, 40, 64)
KSPLIT_N = (64, 2048)

C16_M, C16_N, C16_K = (1, 17, 40, 64), (32, 96, 2048), 256

KV_CASES = [(2, 64, 12), (4, 128, 24), (16, 128, 40), (16, 128, 64)]  # (H, D, M)

# (M, N) of the table in launch_gemm's order of rules -> (MT, NT, waves), at K < 4096
FORM_TABLE = [((16, 64), (1, 1, 8)), ((17, 64), (1, 1, 4)), ((33, 64), (1, 2, 8)),
              ((65, 2048), (2, 1, 8)), ((32, 8192), (2, 2, 8)), ((64, 4096), (4, 1, 8)),
              ((64, 6144), (4, 2, 8))]
PLAIN_I8_K = 128

F16_EXACT_M = (1, 16, 17, 24, 32, 33, 64, 65, 130)
F16_EXACT_NK = [(2048, 64), (8192, 64), (4096, 64), (6144, 64), (2048, 4096), (64, 8192)]
F16_FORCED = [(1, 8, 16), (1, 4, 16), (2, 8, 16), (2, 8, 32), (1, 8, 64), (2, 8, 64), (4, 4, 32),
              (3, 8, 64)]

PLAIN_FORMS = [(1, 1, 8), (1, 1, 4), (1, 2, 8), (2, 1, 8), (2, 2, 8), (4, 1, 8), (4, 2, 8)]


# ---------------------------------------------------------------------------
# 2.0 coverage
# ---------------------------------------------------------------------------
def test_every_launchable_form_is_reached(gpu, tune):
    plain = {I8: set(), F16: set()}

    def add_plain(dtype, M, N, K):
        f = _form(tune, dtype, M, N, K)
        assert f[3:] == (1, 0), f
        plain[dtype].add(f[:3])

    for (M, N), want in FORM_TABLE:
        for dtype in (I8, F16):
            assert _form(tune, dtype, M, N, PLAIN_I8_K)[:3] == want, (dtype, M, N)
        add_plain(I8, M, N, PLAIN_I8_K)  # test_plain_forms_i8
    for dtype in (I8, F16):
        for M in C16_M:
            for N in C16_N:
                add_plain(dtype, M, N, C16_K)
        for H, D, M in KV_CASES:
            add_plain(dtype, M, 3 * H * D, H * D)
    for N, K in F16_EXACT_NK:
        for M in F16_EXACT_M:
            add_plain(F16, M, N, K)
    for dtype in (I8, F16):
        assert plain[dtype] >= set(PLAIN_FORMS), (dtype, set(PLAIN_FORMS) - plain[dtype])
    # 17..32 rows at K >= 4096: 8 waves on 16 rows (narrow_tile_for)
    assert _form(tune, F16, 24, 2048, 4096) == (1, 1, 8, 1, 0)
    # LayerNorm prologue: always 8 waves, (MT, NT)
    for dtype, cases in ((I8, LN_I8_CASES), (F16, LN_F16_CASES)):
        got = set()
        for M, K, N in cases:
            f = _form(tune, dtype, M, N, K, pro=1)
            assert f[2:] == (8, 1, 1), f
            got.add(f[:2])
        assert got >= {(1, 1), (2, 1), (2, 2), (4, 1), (4, 2)}, (dtype, got)
    # quantising prologue: 16-row workgroups only
    got = set()
    for M, K, N in QP_CASES:
        f = _form(tune, I8, M, N, K, pro=2)
        assert f[2:] == (8, 1, 1) and f[0] == 1, f
        got.add(f[:2])
    assert got == {(1, 1), (1, 2)}, got
    # ksplit2
    for KS in KSPLIT_KS:
        for N in KSPLIT_N:
            for M in KSPLIT_M:
                f = _form(tune, I8, M, N, 64 * KS, ksplit2=1)
                assert f[3:] == (2, 0), f
                if M <= 16:
                    assert f[:3] == (1, 1, 8), (M, f)
                elif M > 32:
                    assert f[:3] == (4, 2, 8), (M, f)
    # the forced forms of test_f16_gemm_forced_forms_exact, as launched
    assert _form(tune, F16, 64, 2048, 4096, nt=3, waves=8, mrows=64)[:3] == (4, 3, 4)
    assert _form(tune, F16, 64, 2048, 4096, nt=4, waves=4, mrows=32)[:3] == (2, 4, 4)
    assert _form(tune, F16, 64, 2048, 4096, nt=2, waves=8, mrows=64)[:3] == (4, 2, 8)


def test_prologue_predicates(gpu, tune):
    """gemm_ln_fusable_tune agrees with the rule the case lists were built by
    (64 KB of fp32 rows per workgroup); the quantising prologue takes 16-row
    forms only."""
    for dtype, ks in ((I8, LN_I8_K), (F16, LN_F16_K)):
        for K in ks:
            for M in LN_M:
                assert bool(tune.gemm_ln_fusable_tune(dtype, M, K)) == _ln_fits(M, K), (dtype, M, K)
    assert not tune.gemm_ln_fusable_tune(I8, 16, 2304) and not tune.gemm_ln_fusable_tune(I8, 1, 200)
    assert not tune.gemm_ln_fusable_tune(F16, 1, 64)  # K * 2 bytes not a multiple of 256
    for M, K, N in QP_CASES:
        assert tune.gemm_quant_prologue_ok_tune(M, N, K), (M, N, K)
    assert not tune.gemm_quant_prologue_ok_tune(64, 4096, 256)  # 33..64 rows, 256 column tiles
    assert not tune.gemm_quant_prologue_ok_tune(32, 8192, 256)


# ---------------------------------------------------------------------------
# Plain I8 launches at every form of the table (row-major and packed A)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [mn for mn, _ in FORM_TABLE])
def test_plain_forms_i8(gpu, tune, oracle, M, N):
    K = PLAIN_I8_K
    W, Wp, sw, bias, dsw, dbias = _weights(I8, K, N)
    rng = np.random.default_rng(M + N)
    A = rng.integers(-128, 128, (M, K), dtype=np.int8)
    sa = rng.uniform(1e-3, 1e-2, M).astype(np.float32)
    dsa, dA, dAp = _dev(sa), _dev(A), _packed_a(A, I8)
    ref = oracle.i8_gemm(A, W, sa, sw, bias, 1)[1]
    for packed in (0, 1):
        C = _nan(M, N)
        assert _wg(tune, dtype=I8, A=dAp if packed else dA, lda=K, a_packed=packed, W_packed=Wp,
                   M=M, N=N, K=K, sa=dsa, sw=dsw, bias=dbias, act=1, C=C) == 0
        _same_bits(C.read(), ref, f"packed={packed}")


# ---------------------------------------------------------------------------
# 2.1 / 2.2 LayerNorm prologue
# ---------------------------------------------------------------------------
def _ln_inputs(M, K):
    """x [M][K] with the adversarial rows of test_row_ops_gpu.py in the last
    rows (so that they fall into the partial row block), gamma, beta."""
    rng = np.random.default_rng(M * 100003 + K)
    x = (rng.standard_normal((M, K)) * 2 + 0.5).astype(np.float32)
    x[M - 1] = rng.uniform(-1, 1, K).astype(np.float32)
    x[M - 1, K - 1] = -40.0  # |max| in the last element
    if M >= 3:
        x[M - 2] = (1e3 + 1e-3 * rng.standard_normal(K)).astype(np.float32)
        x[M - 3] = 1.5  # all equal: the output is beta
    g = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    b = (0.1 * rng.standard_normal(K)).astype(np.float32)
    return x, g, b


def _emb_inputs(M, K):
    V = 50
    rng = np.random.default_rng(M + K)
    E = rng.standard_normal((V, K)).astype(np.float16)
    tok = np.resize(np.array([-3, V + 5, 0, V - 1, V, 7, 23], np.int32), M)
    return E, tok, V, E[np.clip(tok, 0, V - 1)].astype(np.float32)


def _ln_launch(tune, dtype, dx, dg, db, M, K):
    """The LayerNorm launch's packed outputs: (A bytes [pad16(M) K esize] over
    a sentinel fill, row scales or None)."""
    import torch
    import llm_capi
    es = 1 if dtype == I8 else 2
    a = torch.full((_pad16(M) * K * es,), SENTINEL, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    if dtype == I8:
        s = torch.full((M,), -1.0, device="cuda")
        st = tune.layernorm_quant_tune(p(dx), M, K, p(dg), p(db), EPS, None, p(a), p(s), 1, None,
                                       None, 0, None, llm_capi.stream_ptr())
    else:
        s = None
        st = tune.layernorm_f16_tune(p(dx), M, K, p(dg), p(db), EPS, p(a), 1, None, None, 0, None,
                                     llm_capi.stream_ptr())
    torch.cuda.synchronize()
    assert st == 0, tune.llm_last_error()
    return a.cpu().numpy(), None if s is None else s.cpu().numpy()


def _ln_call(tune, dtype, M, K, N, dg, db, *, x=None, emb=None, taps=True, want_c=True,
             want_c16=False, kv=None, c_cols=0):
    """One LayerNorm-prologue weight_gemm as fc1 runs it (bias, ReLU); returns
    (C, act_out bytes, sa_out, C16 bytes), None where not asked for."""
    _, Wp, _, _, dsw, dbias = _weights(dtype, K, N)
    es = 1 if dtype == I8 else 2
    C = _nan(M, N) if want_c else None
    C16 = _sentinel(_pad16(M) * N * 2) if want_c16 else None
    act = _sentinel(_pad16(M) * K * es) if taps else None
    sa = Buf(np.full(M, -1.0, np.float32)) if taps and dtype == I8 else None
    f = dict(dtype=dtype, a_packed=1, W_packed=Wp, M=M, N=N, K=K, bias=dbias, act=1, C=C,
             C16=C16, ln_g=dg, ln_b=db, act_out=act, sa_out=sa, c_cols=c_cols)
    if dtype == I8:
        f["sw"] = dsw
    if emb is None:
        f["ln_x"] = x
    else:  # ln_x must be set (it selects the prologue) and must not be read
        dE, dtok, V = emb
        f.update(ln_x=_dev(np.full((M, K), np.nan, np.float32)), ln_emb=dE, ln_tok=dtok, ln_V=V)
    if kv:
        f.update(kv)
    assert _wg(tune, **f) == 0, tune.llm_last_error()
    r = lambda b: None if b is None else b.read()
    return r(C), r(act), r(sa), r(C16)


@pytest.mark.parametrize("M,K,N", LN_I8_CASES)
def test_ln_prologue_i8(gpu, tune, oracle, M, K, N):
    from oracle.oracle import unpack_a_i8
    assert tune.gemm_ln_fusable_tune(I8, M, K)
    W, _, sw, bias, _, _ = _weights(I8, K, N)
    x, g, b = _ln_inputs(M, K)
    dx, dg, db = _dev(x), _dev(g), _dev(b)
    q_ref, s_ref = _ln_launch(tune, I8, dx, dg, db, M, K)
    C, act, sa, _ = _ln_call(tune, I8, M, K, N, dg, db, x=dx)
    # (a) the taps are the LayerNorm launch's outputs; padding rows keep the fill
    _same_bits(act, q_ref, "act_out")
    _same_bits(sa, s_ref, "sa_out")
    q = unpack_a_i8(act.view(np.int8), M, K)
    _same_bits(q, unpack_a_i8(q_ref.view(np.int8), M, K))
    assert (q[M - 1, K - 1] == -127) and np.isfinite(sa).all()
    # (b) C is the oracle's GEMM of the tapped A
    _same_bits(C, oracle.i8_gemm(q, W, sa, sw, bias, 1)[1], "C")
    # (c) the production launch (taps off) computes the same C
    C2, _, _, _ = _ln_call(tune, I8, M, K, N, dg, db, x=dx, taps=False)
    _same_bits(C2, C, "C without taps")
    # (d) embedding rows E[clamp(tok)] equal the x-row call on the widened rows
    E, tok, V, xe = _emb_inputs(M, K)
    want = _ln_call(tune, I8, M, K, N, dg, db, x=_dev(xe))
    got = _ln_call(tune, I8, M, K, N, dg, db, emb=(_dev(E), _dev(tok), V))
    for w_, g_, what in zip(want[:3], got[:3], ("C", "act_out", "sa_out")):
        _same_bits(g_, w_, "embedding source " + what)


@pytest.mark.parametrize("M,K,N", LN_F16_CASES)
def test_ln_prologue_f16(gpu, tune, M, K, N):
    """C against the float64 product of the tapped A with W, element by
    element, within 2 (K + 2) 2^-24 (|A| @ |W| + |bias|): K products (each
    exact in fp32: 11 x 11 bits) summed in fp32 in any order and one bias add
    make at most K rounding errors of 2^-24 relative to the running sums, each
    bounded by sum |a w| + |bias|, so (K + 1) 2^-24 of it to first order (K + 2
    covers the higher-order terms at K <= 512); doubled because the rounding
    inside the MFMA's own adder tree is not documented.  ReLU is 1-Lipschitz.
    The worst observed ratio to that bound is recorded (profiles/)."""
    from oracle.oracle import unpack_a_f16
    assert tune.gemm_ln_fusable_tune(F16, M, K)
    W, _, _, bias, _, _ = _weights(F16, K, N)
    x, g, b = _ln_inputs(M, K)
    dx, dg, db = _dev(x), _dev(g), _dev(b)
    h_ref, _ = _ln_launch(tune, F16, dx, dg, db, M, K)
    C, act, _, C16 = _ln_call(tune, F16, M, K, N, dg, db, x=dx, want_c16=True)
    _same_bits(act, h_ref, "act_out")
    A = unpack_a_f16(act, M, K).astype(np.float64)
    assert np.isfinite(A).all()
    W64 = W.astype(np.float64)
    ref = np.maximum(A @ W64 + bias, 0)
    bound = 2 * (K + 2) * 2.0 ** -24 * (np.abs(A) @ np.abs(W64) + np.abs(bias))
    err = np.abs(C.astype(np.float64) - ref)
    ratio = float(np.max(err / np.maximum(bound, 1e-300)))
    record("weight_gemm_f16_prologue", M=M, K=K, N=N, worst_ratio_to_bound=ratio,
           max_abs_err=float(err.max()))
    print(f"f16 prologue M={M} K={K} N={N}: worst err / bound = {ratio:.4f}")
    assert ratio <= 1.0, (ratio, float(err.max()))
    # the packed fp16 copy is the same launch's C, rounded; padding rows keep the fill
    _same_bits(C16, _pack_rows(C.astype(np.float16), F16), "C16")
    # the fp16 decoder's fc1: C16 only, taps off
    _, _, _, only = _ln_call(tune, F16, M, K, N, dg, db, x=dx, taps=False, want_c=False,
                             want_c16=True)
    _same_bits(only, C16, "C16 alone")
    # embedding source
    E, tok, V, xe = _emb_inputs(M, K)
    want = _ln_call(tune, F16, M, K, N, dg, db, x=_dev(xe))
    got = _ln_call(tune, F16, M, K, N, dg, db, emb=(_dev(E), _dev(tok), V))
    _same_bits(got[0], want[0], "embedding source C")
    _same_bits(got[1], want[1], "embedding source act_out")


# ---------------------------------------------------------------------------
# 2.3 quantising prologue
# ---------------------------------------------------------------------------
def _quant_inputs(M, K):
    rng = np.random.default_rng(M * 7919 + K)
    x = (rng.standard_normal((M, K)) * 3).astype(np.float32)
    # .5 boundaries of x * scale: |max| 127 makes scale = 127 / (127 + 1e-6) = 1 in fp32
    x[M - 1] = (rng.integers(-127, 127, K) + 0.5).astype(np.float32)
    x[M - 1, :5] = [127.0, 0.5, -0.5, 1.5, -1.5]
    if M >= 3:
        x[M - 2] = rng.uniform(-1, 1, K).astype(np.float32)
        x[M - 2, K - 1] = 40.0  # |max| in the last element
        x[M - 3] = 0.0
    return x


@pytest.mark.parametrize("M,K,N", QP_CASES)
def test_quant_prologue(gpu, tune, oracle, M, K, N):
    assert tune.gemm_quant_prologue_ok_tune(M, N, K)
    W, Wp, sw, _, dsw, _ = _weights(I8, K, N)
    x = _quant_inputs(M, K)
    dx = _dev(x)
    q_ref, s_ref = oracle.quantize_rows(x)
    assert list(q_ref[M - 1, :5]) == [127, 1, -1, 2, -2]  # round half away from zero
    ref = oracle.i8_gemm(q_ref, W, s_ref, sw, None, 0)[1]
    f = dict(dtype=I8, a_packed=1, W_packed=Wp, M=M, N=N, K=K, sw=dsw, ln_x=dx, ln_quant_only=1)
    C, act, sa = _nan(M, N), _sentinel(_pad16(M) * K), Buf(np.full(M, -1.0, np.float32))
    assert _wg(tune, C=C, act_out=act, sa_out=sa, **f) == 0, tune.llm_last_error()
    _same_bits(C.read(), ref, "C")
    _same_bits(act.read(), _pack_rows(q_ref, I8), "act_out")
    _same_bits(sa.read(), s_ref, "sa_out")
    C2 = _nan(M, N)
    assert _wg(tune, C=C2, **f) == 0
    _same_bits(C2.read(), ref, "C without taps")


@pytest.mark.parametrize("M,K", [(65, 256), (16, 2304), (16, 320)])
def test_quant_prologue_refused(gpu, tune, M, K):
    N = 256
    assert not tune.gemm_quant_prologue_ok_tune(M, N, K)
    _, Wp, _, _, dsw, _ = _weights(I8, K, N)
    C = _nan(M, N)
    st = _wg(tune, dtype=I8, a_packed=1, W_packed=Wp, M=M, N=N, K=K, sw=dsw, C=C,
             ln_x=_dev(np.ones((M, K), np.float32)), ln_quant_only=1)
    assert st != 0 and b"prologue" in tune.llm_last_error()
    assert C.untouched()


# ---------------------------------------------------------------------------
# 2.4 ksplit2
# ---------------------------------------------------------------------------
def _ksplit_ref(acc0, acc1, sa, sw, bias):
    """The kernel's own float32 operation order (every numpy op rounds once)."""
    f = np.float32
    scale = (f(1) * sa)[:, None] * sw[None, :]
    y0 = acc0.astype(np.int32).astype(f) * scale
    if bias is not None:
        y0 = y0 + bias[None, :]
    y1 = acc1.astype(np.int32).astype(f) * scale
    if bias is not None:
        y1 = y1 + f(0)  # slice 1 adds a zero bias
    assert scale.dtype == f and y0.dtype == f and y1.dtype == f
    return y0 + y1


@pytest.mark.parametrize("N", KSPLIT_N)
@pytest.mark.parametrize("KS", KSPLIT_KS)
def test_ksplit2(gpu, tune, KS, N):
    K = 64 * KS
    W, Wp, sw, bias, dsw, dbias = _weights(I8, K, N)
    rng = np.random.default_rng(KS * 131 + N)
    A_all = rng.integers(-128, 128, (max(KSPLIT_M), K), dtype=np.int8)
    sa_all = rng.uniform(1e-3, 1e-2, max(KSPLIT_M)).astype(np.float32)
    half = 64 * (KS // 2)  # slice z sums k-steps [z KS / 2, (z + 1) KS / 2)
    acc0_all = _matmul_exact(A_all[:, :half], W[:half])
    acc1_all = _matmul_exact(A_all[:, half:], W[half:])
    for M in KSPLIT_M:
        A, sa = A_all[:M], sa_all[:M]
        dA, dsa = _packed_a(A, I8), _dev(sa)
        for with_bias in (False, True):
            ref = _ksplit_ref(acc0_all[:M], acc1_all[:M], sa, sw, bias if with_bias else None)
            for c_ld in (N, N + 16):
                pre = np.full((M, c_ld), np.nan, np.float32)
                pre[:, :N] = 0.0
                runs = []
                for _ in range(2):
                    C = Buf(pre)
                    assert _wg(tune, dtype=I8, A=dA, a_packed=1, W_packed=Wp, M=M, N=N, K=K,
                               sa=dsa, sw=dsw, bias=dbias if with_bias else None, C=C,
                               c_ld=0 if c_ld == N else c_ld, ksplit2=1) == 0, tune.llm_last_error()
                    runs.append(C.read())
                what = f"M={M} bias={with_bias} c_ld={c_ld}"
                _same_bits(runs[0][:, :N], ref, what)
                _same_bits(runs[1], runs[0], what + " second run")
                _same_bits(runs[0][:, N:], pre[:, N:], what + " row padding")


@pytest.mark.parametrize("why", ["relu", "15 k-steps", "C16", "c_cols < N"])
def test_ksplit2_refused(gpu, tune, why):
    M, N = 16, 64
    K = 64 * (15 if why == "15 k-steps" else 16)
    _, Wp, _, _, dsw, _ = _weights(I8, K, N)
    rng = np.random.default_rng(1)
    A = rng.integers(-128, 128, (M, K), dtype=np.int8)
    C, C16 = _nan(M, N), _sentinel(M * N * 2)
    f = dict(dtype=I8, A=_packed_a(A, I8), a_packed=1, W_packed=Wp, M=M, N=N, K=K, sw=dsw, C=C,
             ksplit2=1)
    assert _form(tune, I8, M, N, 1024, ksplit2=1) == (1, 1, 8, 2, 0)
    if why == "relu":
        f["act"] = 1
    elif why == "C16":
        f["C16"] = C16
    elif why == "c_cols < N":
        f["c_cols"] = N - 16
    assert _wg(tune, **f) != 0 and b"ksplit2" in tune.llm_last_error()
    assert C.untouched() and C16.untouched()


# ---------------------------------------------------------------------------
# 2.5 packed fp16 output
# ---------------------------------------------------------------------------
def _plain_operands(dtype, M, K, seed):
    """(A, device packed A, sa or None, device sa or None) of a plain launch."""
    rng = np.random.default_rng(seed)
    if dtype == I8:
        A = rng.integers(-128, 128, (M, K), dtype=np.int8)
        sa = rng.uniform(1e-3, 1e-2, M).astype(np.float32)
        return A, _packed_a(A, I8), sa, _dev(sa)
    A = rng.standard_normal((M, K)).astype(np.float16)
    return A, _packed_a(A, F16), None, None


@pytest.mark.parametrize("dtype", [I8, F16])
@pytest.mark.parametrize("N", C16_N)
@pytest.mark.parametrize("M", C16_M)
def test_c16(gpu, tune, oracle, dtype, M, N):
    K = C16_K
    W, Wp, sw, bias, dsw, dbias = _weights(dtype, K, N)
    A, dA, sa, dsa = _plain_operands(dtype, M, K, M * 13 + N)
    f = dict(dtype=dtype, A=dA, a_packed=1, W_packed=Wp, M=M, N=N, K=K, bias=dbias)
    if dtype == I8:
        f.update(sa=dsa, sw=dsw)
    for act in (0, 1, 2):
        C, C16 = _nan(M, N), _sentinel(_pad16(M) * N * 2)
        assert _wg(tune, C=C, C16=C16, act=act, **f) == 0, tune.llm_last_error()
        c = C.read()
        assert np.isfinite(c).all()
        if dtype == I8 and act < 2:
            _same_bits(c, oracle.i8_gemm(A, W, sa, sw, bias, act)[1], f"C act={act}")
        # unpack_a_f16(C16, M, N) == C.astype(float16), and the padding rows keep the fill
        _same_bits(C16.read(), _pack_rows(c.astype(np.float16), F16), f"C16 act={act}")
        only = _sentinel(_pad16(M) * N * 2)
        assert _wg(tune, C16=only, act=act, **f) == 0
        _same_bits(only.read(), C16.read(), f"C16 alone act={act}")


@pytest.mark.parametrize("dtype", [I8, F16])
def test_c16_refused_unless_n_multiple_of_32(gpu, tune, dtype):
    M, N, K = 16, 48, C16_K
    _, Wp, _, _, dsw, dbias = _weights(dtype, K, N)
    _, dA, _, dsa = _plain_operands(dtype, M, K, 5)
    C, C16 = _nan(M, N), _sentinel(M * 64 * 2)
    st = _wg(tune, dtype=dtype, A=dA, a_packed=1, W_packed=Wp, M=M, N=N, K=K, bias=dbias, C=C,
             C16=C16)
    assert st != 0 and b"N % 32" in tune.llm_last_error()
    assert C.untouched() and C16.untouched()


# ---------------------------------------------------------------------------
# 2.6 KV append
# ---------------------------------------------------------------------------
TS, MAX_TILES = 16, 3
K_SCALE, V_SCALE = 0.25, 3.0  # the inverse of 3 is not a power of two


def _kv_tables(rng, M, H, use_rows):
    """pos, rows (or None), page table and the row of the table each GEMM row
    writes through, with one skip of every kind."""
    from oracle.oracle import shuffled_page_table
    num_beams = M + 3
    num_pages = num_beams * H * MAX_TILES + 5
    pt = shuffled_page_table(rng, num_beams, H, MAX_TILES, MAX_TILES, num_pages)
    pos = rng.integers(0, TS * MAX_TILES, M).astype(np.int32)
    pos[:4] = [0, TS - 1, TS * MAX_TILES - 1, TS * (MAX_TILES - 1)]  # p % TS in {0, TS - 1}, last tile
    pos[4] = -1                 # skipped: no position
    pos[5] = TS * MAX_TILES     # skipped: past the page table
    rows = None
    br = np.arange(M)
    if use_rows:
        rows = rng.permutation(num_beams)[:M].astype(np.int32)
        rows[8] = num_beams + 1  # skipped: no such table row
        rows[9] = -1             # skipped
        br = rows
    pt[br[6], 0, pos[6] // TS] = num_pages + 3  # skipped for head 0: no such page
    pt[br[7], H - 1, pos[7] // TS] = -1         # skipped for the last head
    return pos, rows, pt, br, num_beams, num_pages


def _kv_expected(pool0, y, which, pos, br, pt, H, D, num_beams, num_pages, stride, enc):
    """pool0 with row m's K (which = 0) or V (1) columns of the full-width
    result y stored at position pos[m] of its pages; the number of (row, head)
    slots stored."""
    hid = H * D
    pool = pool0.copy()
    vals = enc(y[:, hid * (1 + which): hid * (2 + which)], which)
    stored = 0
    for m in range(len(pos)):
        p, r = int(pos[m]), int(br[m])
        if p < 0 or r < 0 or r >= num_beams or p // TS >= MAX_TILES:
            continue
        for h in range(H):
            page = int(pt[r, h, p // TS])
            if page < 0 or page >= num_pages:
                continue
            off = page * stride + (p % TS) * D
            pool[off:off + D] = vals[m, h * D:(h + 1) * D]
            stored += 1
    return pool, stored


def _kv_check(tune, run, y, M, N, H, D, fp8, seed):
    """run(**extra fields) -> status launches the GEMM under test; y is its
    full-width result without the append.  Checks C, both pools and every
    untouched byte, with rows NULL and with a permuted rows."""
    from _fp8 import ref_encode
    hid = H * D
    stride = TS * D + 32  # elements from page to page: more than one page
    if fp8:
        enc = lambda v, which: ref_encode(v, V_SCALE if which else K_SCALE)
    else:
        enc = lambda v, which: v.astype(np.float16).view(np.uint16)
    for use_rows in (False, True):
        rng = np.random.default_rng(seed + use_rows)
        pos, rows, pt, br, num_beams, num_pages = _kv_tables(rng, M, H, use_rows)
        garbage = lambda: rng.integers(0, 256 if fp8 else 65536, num_pages * stride).astype(
            np.uint8 if fp8 else np.uint16)
        kp, vp, C = Buf(garbage()), Buf(garbage()), _nan(M, N)
        dpos, dpt = _dev(pos), _dev(pt)
        drows = None if rows is None else _dev(rows)
        st = run(C=C, c_cols=hid, c_ld=N, has_kv=1, kv_pos=dpos, kv_page_table=dpt, kv_rows=drows,
                 kv_k_pool=kp, kv_v_pool=vp, kv_num_beams=num_beams, kv_max_tiles=MAX_TILES,
                 kv_page_size=TS, kv_num_pages=num_pages, kv_H=H, kv_D=D, kv_page_stride=stride,
                 kv_dtype=FP8 if fp8 else F16,
                 kv_k_inv_scale=float(np.float32(1) / np.float32(K_SCALE)),
                 kv_v_inv_scale=float(np.float32(1) / np.float32(V_SCALE)))
        assert st == 0, tune.llm_last_error()
        c = C.read()
        what = f"rows={'permuted' if use_rows else 'NULL'}"
        _same_bits(c[:, :hid], y[:, :hid], what + " q columns")
        _same_bits(c[:, hid:], C.before[:, hid:], what + " C beyond c_cols")
        want_stored = (M - (4 if use_rows else 2)) * H - 2
        for which, pool in ((0, kp), (1, vp)):
            want, stored = _kv_expected(pool.before, y, which, pos, br, pt, H, D, num_beams,
                                        num_pages, stride, enc)
            assert stored == want_stored, (stored, want_stored)
            _same_bits(pool.read(), want, what + (" V pool" if which else " K pool"))


@functools.lru_cache(maxsize=None)
def _kv_operands(dtype, H, D, M):
    return _plain_operands(dtype, M, H * D, H * 1000 + D + M)


@pytest.mark.parametrize("pool", ["f16", "fp8"])
@pytest.mark.parametrize("dtype", [I8, F16])
@pytest.mark.parametrize("H,D,M", KV_CASES)
def test_kv_append(gpu, tune, oracle, H, D, M, dtype, pool):
    hid = H * D
    N, K = 3 * hid, hid
    W, Wp, sw, _, dsw, _ = _weights(dtype, K, N)
    A, dA, sa, dsa = _kv_operands(dtype, H, D, M)
    f = dict(dtype=dtype, A=dA, a_packed=1, W_packed=Wp, M=M, N=N, K=K)
    if dtype == I8:
        f.update(sa=dsa, sw=dsw)
    full = _nan(M, N)
    assert _wg(tune, C=full, **f) == 0, tune.llm_last_error()
    y = full.read()
    assert np.isfinite(y).all()
    if dtype == I8:
        _same_bits(y, _kv_oracle(oracle, H, D, M), "full-width C")
    _kv_check(tune, lambda **kv: _wg(tune, **f, **kv), y, M, N, H, D, pool == "fp8",
              seed=H + D + M)


_kv_oracle_cache = {}


def _kv_oracle(oracle, H, D, M):
    key = (H, D, M)
    if key not in _kv_oracle_cache:
        W, _, sw, _, _, _ = _weights(I8, H * D, 3 * H * D)
        A, _, sa, _ = _kv_operands(I8, H, D, M)
        _kv_oracle_cache[key] = oracle.i8_gemm(A, W, sa, sw, None, 0)[1]
    return _kv_oracle_cache[key]


@pytest.mark.parametrize("pool", ["f16", "fp8"])
@pytest.mark.parametrize("dtype", [I8, F16])
def test_kv_append_with_ln_prologue(gpu, tune, dtype, pool):
    """The decode step's qkv launch: LayerNorm prologue and KV append in one
    (hid 256, 16 rows; no bias, no activation)."""
    H, D, M = 4, 64, 16
    hid = H * D
    N, K = 3 * hid, hid
    _, Wp, _, _, dsw, _ = _weights(dtype, K, N)
    x, g, b = _ln_inputs(M, K)
    f = dict(dtype=dtype, a_packed=1, W_packed=Wp, M=M, N=N, K=K, ln_x=_dev(x), ln_g=_dev(g),
             ln_b=_dev(b))
    if dtype == I8:
        f["sw"] = dsw
    assert _form(tune, dtype, M, N, K, pro=1) == (1, 1, 8, 1, 1)
    full = _nan(M, N)
    assert _wg(tune, C=full, **f) == 0, tune.llm_last_error()
    y = full.read()
    assert np.isfinite(y).all()
    _kv_check(tune, lambda **kv: _wg(tune, **f, **kv), y, M, N, H, D, pool == "fp8", seed=77)


# ---------------------------------------------------------------------------
# 2.7 FP16 GEMM on integer-valued operands: exact in any summation order
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _int_operands(M, K, N):
    """A, W, bias with integer values in [-4, 4]: every partial sum is an
    integer of magnitude <= 16 K + 4 < 2^24 (K <= 8192), so fp32 accumulation
    is exact whatever the order and the result is the integer product."""
    import llm_capi
    assert 16 * K + 4 < 2 ** 24
    rng = np.random.default_rng(M + K * 3 + N)
    A = rng.integers(-4, 5, (M, K)).astype(np.float16)
    W = rng.integers(-4, 5, (K, N)).astype(np.float16)
    bias = rng.integers(-4, 5, N).astype(np.float32)
    ref = _matmul_exact(A, W)
    return A, W, bias, ref, llm_capi.pack_weights(_dev(W), F16)


@pytest.mark.parametrize("N,K", F16_EXACT_NK)
def test_f16_gemm_exact(gpu, N, K):
    import llm_capi
    A_all, _, bias, ref_all, Wp = _int_operands(max(F16_EXACT_M), K, N)
    dA, dbias = _dev(A_all), _dev(bias)
    for M in F16_EXACT_M:
        for act, b in ((0, None), (0, bias), (1, bias)):
            C = llm_capi.f16_gemm(dA[:M], Wp, N, bias=None if b is None else dbias, act=act)
            ref = ref_all[:M] + (0 if b is None else b.astype(np.int64))
            if act:
                ref = np.maximum(ref, 0)
            _same_bits(C.cpu().numpy(), ref.astype(np.float32), f"M={M} act={act} bias={b is not None}")


@pytest.mark.parametrize("M,K,N", [(37, 512, 96), (64, 4096, 2048), (48, 2048, 6144)])
def test_f16_gemm_forced_forms_exact(gpu, tune, M, K, N):
    import llm_capi
    A, _, _, ref, Wp = _int_operands(M, K, N)
    ref = ref.astype(np.float32)
    dA, dAp = _dev(A), _packed_a(A, F16)
    for nt, waves, mrows in F16_FORCED:
        for packed in (1, 0):
            C = _nan(M, N)
            llm_capi.check(tune.f16_gemm_tune(nt, waves, mrows, packed,
                                              (dAp if packed else dA).data_ptr(), K, Wp.data_ptr(),
                                              C.data_ptr(), M, N, K, llm_capi.stream_ptr()), tune)
            _same_bits(C.read(), ref, f"nt={nt} waves={waves} mrows={mrows} packed={packed}")
