"""The row kernels of csrc/row_ops.hip at every form.

Through the C ABI: layernorm_quant and quantize_rows one width below and above
every float4-chunks-per-thread boundary (1, 2, 4, 8, 16), the scalar kernels
(cols % 4 != 0, and quantize_rows past 16384), the three output modes and
adversarial rows.  Through the tuning build's entries over the internal
launchers (csrc/tune/row_ops_tune.hip): the forms only the decoder runs --
packed-A outputs, the embedding source, the zeroing source, fp16 outputs.

References: `out` against a float64 LayerNorm (rtol = atol = 1e-5; a row beyond
that is held to 4x the error a numpy float32 LayerNorm of the same row makes
against float64, the reduction order being the only difference); `q` and
`inv_scale` bit for bit equal to the oracle's quantisation of the GPU's own
`out` (the kernel quantises exactly the values it stores)."""
import ctypes

import numpy as np
import pytest

from _util import record

pytestmark = pytest.mark.gpu

EPS = 1e-5
VECTOR_COLS = [4, 64, 1020, 1024, 1028, 2048, 2052, 4096, 4100, 8192, 8196, 16384]
SCALAR_COLS = [1, 3, 30, 1023, 2050, 16383]
SENTINEL = 0x5A


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    import llm_capi
    return llm_capi.stream_ptr()


def _ln64(x, g, b):
    x = x.astype(np.float64)
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    return (x - mean) / np.sqrt(var + EPS) * g.astype(np.float64) + b.astype(np.float64)


def _ln32(x, g, b):
    f = np.float32
    mean = x.mean(axis=1, keepdims=True, dtype=f)
    d = (x - mean).astype(f)
    var = (d * d).mean(axis=1, keepdims=True, dtype=f)
    inv = (f(1) / np.sqrt(var + f(EPS))).astype(f)
    return ((d * inv).astype(f) * g + b).astype(f)


def _layernorm(lib, x, g, b, want_out=True, want_q=True, dx=None):
    """(status, out, q, inv_scale) of one layernorm_quant call (numpy or None)."""
    import torch
    R, C = x.shape
    dx = _dev(x) if dx is None else dx
    dg, db = _dev(g), _dev(b)  # named: a temporary's memory would be reused before the launch
    out = torch.full((R, C), 7.0, device="cuda") if want_out else None
    q = torch.full((R, C), 99, dtype=torch.int8, device="cuda") if want_q else None
    s = torch.full((R,), -1.0, device="cuda") if want_q else None
    st = lib.layernorm_quant(_p(dx), R, C, _p(dg), _p(db), EPS, _p(out), _p(q), _p(s),
                             _stream())
    torch.cuda.synchronize()
    n = lambda t: None if t is None else t.cpu().numpy()
    return st, n(out), n(q), n(s)


def _check_out(name, out, x, g, b):
    """out vs float64: 1e-5, else 4x the float32 numpy LayerNorm's own error."""
    ref = _ln64(x, g, b)
    err = np.abs(out - ref)
    within = err <= 1e-5 + 1e-5 * np.abs(ref)
    row_err = err.max(axis=1)
    e32 = np.abs(_ln32(x, g, b).astype(np.float64) - ref).max(axis=1)
    record("row_ops_layernorm", case=name, rows=int(x.shape[0]), cols=int(x.shape[1]),
           max_err=float(row_err.max()), f32_numpy_err=float(e32.max()),
           rows_beyond_1e5=int((~within.all(axis=1)).sum()),
           worst_ratio_to_f32=float((row_err / np.maximum(e32, 1e-300))[~within.all(axis=1)].max(initial=0)))
    print(f"{name} {x.shape}: max err {row_err.max():.3e}, numpy f32 err {e32.max():.3e}, "
          f"rows beyond 1e-5: {int((~within.all(axis=1)).sum())}")
    for r in range(x.shape[0]):
        if not within[r].all():
            assert row_err[r] <= 4 * e32[r], (name, r, row_err[r], e32[r])


def _check_modes(lib, oracle, name, x, g, b):
    """The three output modes of one input: `out` against float64, q / inv_scale
    bit for bit against the oracle's quantisation of that `out`."""
    st, out, q, s = _layernorm(lib, x, g, b)
    assert st == 0, (name, st, lib.llm_last_error())
    _check_out(name, out, x, g, b)
    qr, sr = oracle.quantize_rows(out)
    np.testing.assert_array_equal(q, qr)
    np.testing.assert_array_equal(s.view(np.uint32), sr.view(np.uint32))
    st, out1, _, _ = _layernorm(lib, x, g, b, want_q=False)
    assert st == 0
    np.testing.assert_array_equal(out1.view(np.uint32), out.view(np.uint32))
    st, _, q2, s2 = _layernorm(lib, x, g, b, want_out=False)
    assert st == 0
    np.testing.assert_array_equal(q2, qr)
    np.testing.assert_array_equal(s2.view(np.uint32), sr.view(np.uint32))
    return out, q, s


def _random_case(rows, cols):
    rng = np.random.default_rng(rows * 100003 + cols)
    x = (rng.standard_normal((rows, cols)) * 2 + 0.5).astype(np.float32)
    g = (1 + 0.1 * rng.standard_normal(cols)).astype(np.float32)
    b = (0.1 * rng.standard_normal(cols)).astype(np.float32)
    return x, g, b


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("cols", VECTOR_COLS + SCALAR_COLS)
def test_layernorm_quant_widths(gpu, oracle, rows, cols):
    x, g, b = _random_case(rows, cols)
    _check_modes(gpu, oracle, f"random_r{rows}", x, g, b)


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("cols", VECTOR_COLS + SCALAR_COLS + [16388, 20000])
def test_quantize_rows_widths(gpu, oracle, rows, cols):
    import llm_capi
    x, _, _ = _random_case(rows, cols)
    x *= 3
    q, s = llm_capi.quantize_rows(_dev(x))
    qr, sr = oracle.quantize_rows(x)
    np.testing.assert_array_equal(q.cpu().numpy(), qr)
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), sr.view(np.uint32))


def test_layernorm_quant_refuses_wide_rows(gpu):
    x, g, b = _random_case(1, 16385)
    st, out, q, s = _layernorm(gpu, x, g, b)
    assert st == 1 and b"16384" in gpu.llm_last_error()
    assert (out == 7.0).all() and (q == 99).all() and (s == -1.0).all()


def _adversarial_rows(cols, rng):
    """[7][cols] rows on which row kernels go wrong."""
    x = np.zeros((7, cols), np.float32)  # 0: all zero
    x[1] = 1.5  # constant (var = 0); 1.5 * n is exact in fp32, so is any order's mean
    x[2] = (1e3 + 1e-3 * rng.standard_normal(cols)).astype(np.float32)
    x[3] = rng.standard_normal(cols).astype(np.float32)
    x[3, cols // 3] = 1e4  # one outlier
    x[4] = rng.uniform(-1, 1, cols).astype(np.float32)
    x[4, cols - 1] = -40.0  # absmax in the last column, negative
    # .5 rounding boundaries of x * scale: absmax 127 makes scale 127 / (127 + 1e-6) = 1 in fp32
    x[5] = (rng.integers(-127, 127, cols) + 0.5).astype(np.float32)
    x[5, 0] = 127.0
    x[5, cols - 1] = -126.5
    x[6] = (rng.integers(-4000, 4000, cols) * 1e-42).astype(np.float32)  # denormals
    return x


ADV_COLS = [30, 256, 2048, 2050, 4096, 8192, 16384]  # scalar, VPT 1, 2, scalar (9 passes), 4, 8, 16


@pytest.mark.parametrize("cols", ADV_COLS)
def test_quantize_rows_adversarial(gpu, oracle, cols):
    import llm_capi
    x = _adversarial_rows(cols, np.random.default_rng(cols))
    assert np.float32(127.0) / (np.float32(127.0) + np.float32(1e-6)) == 1.0
    assert (x[6] != 0).any() and np.abs(x[6]).max() < np.finfo(np.float32).tiny
    q, s = llm_capi.quantize_rows(_dev(x))
    q, s = q.cpu().numpy(), s.cpu().numpy()
    qr, sr = oracle.quantize_rows(x)
    np.testing.assert_array_equal(q, qr)
    np.testing.assert_array_equal(s.view(np.uint32), sr.view(np.uint32))
    # what the oracle's answers must themselves be on these rows
    assert (q[0] == 0).all() and (q[1] == 127).all() and (q[6] == 0).all()
    assert q[4, cols - 1] == -127 and np.abs(q[4, :cols - 1].astype(int)).max() <= 4
    half = np.sign(x[5]) * np.floor(np.abs(x[5]) + 0.5)  # round half away from zero
    np.testing.assert_array_equal(q[5].astype(np.float32), half)


@pytest.mark.parametrize("cols", ADV_COLS)
def test_layernorm_quant_adversarial(gpu, oracle, cols):
    rng = np.random.default_rng(cols + 1)
    x = _adversarial_rows(cols, rng)
    g = (1 + 0.1 * rng.standard_normal(cols)).astype(np.float32)
    b = (0.1 * rng.standard_normal(cols)).astype(np.float32)
    out, q, s = _check_modes(gpu, oracle, "adversarial", x, g, b)
    assert np.isfinite(out).all()
    # zero and constant rows: (x - mean) is exactly 0, the output is beta
    np.testing.assert_array_equal(out[0], b)
    np.testing.assert_array_equal(out[1], b)
    assert np.argmax(np.abs(out[4])) == cols - 1 and out[4, cols - 1] < 0 and q[4, cols - 1] == -127
    # gamma 0: out = beta exactly, here on .5 rounding boundaries of out * scale
    beta = x[5].copy()
    out, q, s = _check_modes(gpu, oracle, "half_boundaries", x[[2, 3, 4]], np.zeros(cols, np.float32), beta)
    np.testing.assert_array_equal(out, np.tile(beta, (3, 1)))
    half = np.sign(beta) * np.floor(np.abs(beta) + 0.5)
    np.testing.assert_array_equal(q.astype(np.float32), np.tile(half, (3, 1)))


# ---------------------------------------------------------------------------
# The forms the decoder runs, through the tuning build's entries
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tune(gpu):
    import llm_capi
    return llm_capi.load_tune()


def _pad16(rows):
    return (rows + 15) // 16 * 16


def _i8_offsets(rows, K):
    m = np.arange(rows)[:, None]
    k = np.arange(K)[None, :]
    KS = K // 64
    return ((((m >> 4) * KS + (k >> 6)) * 64 + (m & 15) + 16 * ((k & 63) >> 4)) * 16 + (k & 15))


def _f16_offsets(rows, K):
    m = np.arange(rows)[:, None]
    k = np.arange(K)[None, :]
    KS = K // 32
    return ((((m >> 4) * KS + (k >> 5)) * 64 + (m & 15) + 16 * ((k & 31) >> 3)) * 8 + (k & 7))


def _padding_untouched(packed_bytes, rows, cols, elem):
    """Every element of the padded 16-row group that belongs to a row >= rows
    still holds the sentinel (and the rows' own elements cover the rest)."""
    off = (_i8_offsets if elem == 1 else _f16_offsets)(_pad16(rows), cols)
    assert np.array_equal(np.sort(off.ravel()), np.arange(_pad16(rows) * cols))  # a bijection
    el = packed_bytes.view(np.uint8).reshape(-1, elem)
    assert (el[off[rows:].ravel()] == SENTINEL).all()


def _ln_tune(tune, x, g, b, rows, cols, *, out=False, q=False, f16=False, pack=0, emb=None,
             tok=None, V=0, zero_x=None):
    """One layernorm_quant_tune (out / q) or layernorm_f16_tune (f16) call on
    device tensors; returns (status, out, q bytes, inv_scale, out16 bytes)."""
    import torch
    pr = _pad16(rows) if pack else rows
    o = torch.full((rows, cols), 7.0, device="cuda") if out else None
    qq = torch.full((pr * cols,), SENTINEL, dtype=torch.uint8, device="cuda") if q else None
    s = torch.full((rows,), -1.0, device="cuda") if q else None
    h = torch.full((pr * cols * 2,), SENTINEL, dtype=torch.uint8, device="cuda") if f16 else None
    if f16:
        st = tune.layernorm_f16_tune(_p(x), rows, cols, _p(g), _p(b), EPS, _p(h), pack, _p(emb),
                                     _p(tok), V, _p(zero_x), _stream())
    else:
        st = tune.layernorm_quant_tune(_p(x), rows, cols, _p(g), _p(b), EPS, _p(o), _p(qq), _p(s),
                                       pack, _p(emb), _p(tok), V, _p(zero_x), _stream())
    torch.cuda.synchronize()
    n = lambda t: None if t is None else t.cpu().numpy()
    return st, n(o), n(qq), n(s), n(h)


@pytest.mark.parametrize("rows", [1, 17, 33])
@pytest.mark.parametrize("cols", [256, 768, 2048, 4096])
def test_layernorm_packed_outputs(gpu, tune, oracle, rows, cols):
    """pack = 1: q and out16 in packed-A order equal, unpacked, the row-major
    outputs; the padding rows of the last 16-row group are not written."""
    from oracle.oracle import unpack_a_f16, unpack_a_i8
    x, g, b = _random_case(rows, cols)
    dx, dg, db = _dev(x), _dev(g), _dev(b)
    st, out, qp, sp, _ = _ln_tune(tune, dx, dg, db, rows, cols, out=True, q=True, pack=1)
    assert st == 0, tune.llm_last_error()
    st, out_rm, q_rm, s_rm, _ = _ln_tune(tune, dx, dg, db, rows, cols, out=True, q=True)
    assert st == 0
    # the row-major tuning call is the C ABI's call
    st, out_c, q_c, s_c = _layernorm(gpu, x, g, b)
    np.testing.assert_array_equal(out_rm.view(np.uint32), out_c.view(np.uint32))
    np.testing.assert_array_equal(q_rm.view(np.int8).reshape(rows, cols), q_c)
    np.testing.assert_array_equal(out.view(np.uint32), out_rm.view(np.uint32))
    qr, sr = oracle.quantize_rows(out)
    np.testing.assert_array_equal(unpack_a_i8(qp.view(np.int8), rows, cols), qr)
    np.testing.assert_array_equal(unpack_a_i8(qp.view(np.int8), rows, cols),
                                  q_rm.view(np.int8).reshape(rows, cols))
    np.testing.assert_array_equal(sp.view(np.uint32), sr.view(np.uint32))
    np.testing.assert_array_equal(sp.view(np.uint32), s_rm.view(np.uint32))
    _padding_untouched(qp, rows, cols, 1)
    # fp16 output: np.float16(out), row-major and packed
    st, _, _, _, h_rm = _ln_tune(tune, dx, dg, db, rows, cols, f16=True)
    assert st == 0
    np.testing.assert_array_equal(h_rm.view(np.uint16).reshape(rows, cols),
                                  out.astype(np.float16).view(np.uint16))
    st, _, _, _, hp = _ln_tune(tune, dx, dg, db, rows, cols, f16=True, pack=1)
    assert st == 0
    np.testing.assert_array_equal(unpack_a_f16(hp, rows, cols).view(np.uint16),
                                  out.astype(np.float16).view(np.uint16))
    _padding_untouched(hp, rows, cols, 2)


@pytest.mark.parametrize("rows", [1, 17, 33])
@pytest.mark.parametrize("cols", [256, 768, 2048, 4096, 16384])
def test_quantize_rows_packed(gpu, tune, oracle, rows, cols):
    import torch
    from oracle.oracle import unpack_a_i8
    x, _, _ = _random_case(rows, cols)
    dx = _dev(x)
    qp = torch.full((_pad16(rows) * cols,), SENTINEL, dtype=torch.uint8, device="cuda")
    s = torch.full((rows,), -1.0, device="cuda")
    assert tune.quantize_rows_tune(_p(dx), rows, cols, _p(qp), _p(s), 1, _stream()) == 0
    q_rm = torch.full((rows, cols), 99, dtype=torch.int8, device="cuda")
    s_rm = torch.full((rows,), -1.0, device="cuda")
    assert tune.quantize_rows_tune(_p(dx), rows, cols, _p(q_rm), _p(s_rm), 0, _stream()) == 0
    torch.cuda.synchronize()
    qr, sr = oracle.quantize_rows(x)
    qp = qp.cpu().numpy()
    np.testing.assert_array_equal(q_rm.cpu().numpy(), qr)
    np.testing.assert_array_equal(unpack_a_i8(qp.view(np.int8), rows, cols), qr)
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), sr.view(np.uint32))
    np.testing.assert_array_equal(s_rm.cpu().numpy().view(np.uint32), sr.view(np.uint32))
    _padding_untouched(qp, rows, cols, 1)


@pytest.mark.parametrize("cols", [32, 96, 1000, 2080])
def test_pack_refused_unless_cols_multiple_of_64(gpu, tune, cols):
    import torch
    x, g, b = _random_case(3, cols)
    dx, dg, db = _dev(x), _dev(g), _dev(b)
    st, _, qp, sp, _ = _ln_tune(tune, dx, dg, db, 3, cols, q=True, pack=1)
    assert st != 0 and (qp == SENTINEL).all() and (sp == -1.0).all()
    st, _, _, _, hp = _ln_tune(tune, dx, dg, db, 3, cols, f16=True, pack=1)
    assert st != 0 and (hp == SENTINEL).all()
    qq = torch.full((16 * cols,), SENTINEL, dtype=torch.uint8, device="cuda")
    s = torch.full((3,), -1.0, device="cuda")
    assert tune.quantize_rows_tune(_p(dx), 3, cols, _p(qq), _p(s), 1, _stream()) != 0
    torch.cuda.synchronize()
    assert (qq.cpu().numpy() == SENTINEL).all() and (s.cpu().numpy() == -1.0).all()


@pytest.mark.parametrize("rows", [1, 17, 33])
@pytest.mark.parametrize("cols", [256, 768, 2048, 4096])
def test_layernorm_embedding_source(gpu, tune, rows, cols):
    """LnSource::emb: rows read as E[clamp(tok[r])] equal, bit for bit, the x
    source fed float(E[clamp(tok)]); tokens below 0 and past V - 1 are clamped."""
    V = 50
    rng = np.random.default_rng(rows + cols)
    E = rng.standard_normal((V, cols)).astype(np.float16)
    tok = np.resize(np.array([-1, 0, V - 1, V, V + 5, 7, 23], np.int32), rows)
    x = E[np.clip(tok, 0, V - 1)].astype(np.float32)
    _, g, b = _random_case(rows, cols)
    dx, dg, db, dE, dtok = _dev(x), _dev(g), _dev(b), _dev(E), _dev(tok)
    for pack in (0, 1):
        ref = _ln_tune(tune, dx, dg, db, rows, cols, out=True, q=True, pack=pack)
        got = _ln_tune(tune, None, dg, db, rows, cols, out=True, q=True, pack=pack, emb=dE,
                       tok=dtok, V=V)
        assert ref[0] == 0 and got[0] == 0, tune.llm_last_error()
        np.testing.assert_array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
        np.testing.assert_array_equal(got[2], ref[2])
        np.testing.assert_array_equal(got[3].view(np.uint32), ref[3].view(np.uint32))
        ref = _ln_tune(tune, dx, dg, db, rows, cols, f16=True, pack=pack)
        got = _ln_tune(tune, None, dg, db, rows, cols, f16=True, pack=pack, emb=dE, tok=dtok, V=V)
        assert ref[0] == 0 and got[0] == 0
        np.testing.assert_array_equal(got[4], ref[4])
    # and the x-source reference is itself right
    out = _ln_tune(tune, dx, dg, db, rows, cols, out=True)[1]
    _check_out("emb_source", out, x, g, b)


@pytest.mark.parametrize("rows", [1, 17, 33])
@pytest.mark.parametrize("cols", [256, 768, 2048, 4096])
def test_layernorm_zero_x(gpu, tune, rows, cols):
    """LnSource::zero_x (what fc2's split-K accumulation relies on): the
    outputs are those of the plain call, exactly the rows x cols floats read
    are zero afterwards, and the floats after them are untouched."""
    import torch
    x, g, b = _random_case(rows, cols)
    tail = np.full(64, 3.25, np.float32)
    dg, db = _dev(g), _dev(b)
    ref = _ln_tune(tune, _dev(x), dg, db, rows, cols, out=True, q=True, pack=1)
    ref16 = _ln_tune(tune, _dev(x), dg, db, rows, cols, f16=True, pack=1)
    for f16 in (False, True):
        buf = _dev(np.concatenate([x.ravel(), tail]))  # x and its own zero target
        got = _ln_tune(tune, buf, dg, db, rows, cols, out=not f16, q=not f16, f16=f16, pack=1,
                       zero_x=buf)
        assert got[0] == 0, tune.llm_last_error()
        want = ref16 if f16 else ref
        for a, w in zip(got[1:], want[1:]):
            assert (a is None) == (w is None)
            if a is not None:
                np.testing.assert_array_equal(a.view(np.uint8), w.view(np.uint8))
        after = buf.cpu().numpy()
        assert (after[:rows * cols].view(np.uint32) == 0).all()
        np.testing.assert_array_equal(after[rows * cols:], tail)
    # a zero target other than x: x is left as it was
    dx = _dev(x)
    other = torch.full((rows * cols + 64,), 3.25, device="cuda")
    got = _ln_tune(tune, dx, dg, db, rows, cols, out=True, q=True, pack=1, zero_x=other)
    assert got[0] == 0
    np.testing.assert_array_equal(got[2], ref[2])
    np.testing.assert_array_equal(dx.cpu().numpy(), x)
    other = other.cpu().numpy()
    assert (other[:rows * cols] == 0).all() and (other[rows * cols:] == 3.25).all()


@pytest.mark.parametrize("rows", [1, 17, 33])
@pytest.mark.parametrize("cols", [256, 768, 2048, 4096])
def test_to_f16_packed(gpu, tune, rows, cols):
    import torch
    from oracle.oracle import unpack_a_f16
    rng = np.random.default_rng(rows * 7 + cols)
    x = (rng.standard_normal((rows, cols)) * 4).astype(np.float32)
    x[0, :4] = [65504.0, -1e-7, 2049.0, 1e-5]  # fp16 max, underflow, a tie to even, a subnormal
    dx = _dev(x)
    want = x.astype(np.float16).view(np.uint16)
    plain = torch.full((rows * cols * 2,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert tune.to_f16_tune(_p(dx), rows * cols, _p(plain), 0, _stream()) == 0
    packed = torch.full((_pad16(rows) * cols * 2,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert tune.to_f16_tune(_p(dx), rows * cols, _p(packed), cols, _stream()) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(plain.cpu().numpy().view(np.uint16).reshape(rows, cols), want)
    packed = packed.cpu().numpy()
    np.testing.assert_array_equal(unpack_a_f16(packed, rows, cols).view(np.uint16), want)
    _padding_untouched(packed, rows, cols, 2)
    # pack_cols must be a multiple of 32
    bad = torch.full((64 * 2,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert tune.to_f16_tune(_p(dx), 48, _p(bad), 48, _stream()) != 0
    torch.cuda.synchronize()
    assert (bad.cpu().numpy() == SENTINEL).all()
