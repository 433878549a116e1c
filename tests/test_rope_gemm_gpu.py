"""The rotary epilogue of the fused qkv projection (csrc/gemm_impl.hpp, ROPE)
and rope_rows (csrc/row_ops.hip), kernel by kernel, bit for bit.

Through weight_gemm_tune of the tuning build (llm::weight_gemm itself behind a
plain-C struct), for every shape: one launch without a KV append gives the
plain fp32 result y [M][3 hid]; one KV-append launch with a rotary table, into
NaN / garbage pre-filled buffers between guard margins, must then hold

    C[:, :hid]  == rope_ref(y_q)
    K pages     == fp16(rope_ref(y_k))   (FP8 pools: the host codec of it at k_scale)
    V pages     == fp16(y_v)             (not rotated)

and nothing else; rope_rows over y's q and K columns must equal rope_ref too.
rope_ref (tests/_rope.py) is the numpy float32 statement of the rotation.

Shapes: hid 256 (4 x 64), 512 (4 x 128) and 2048 (16 x 128), int8 and fp16
weights, and M chosen from gemm_form's rules so that the set reaches every
kernel form a KV-append launch can take at these sizes
(test_every_rope_form_is_reached asserts it through gemm_form_tune), with the
LayerNorm-prologue launch (the decode step's qkv) where the rows fit it.
Positions are ragged per row: 0, a page's last and first slot, the table's
last position, one position past the table (stored, not rotated), -1 and one
past the page table (neither stored nor rotated), and one row whose pages are
missing (q rotated, nothing stored)."""
import ctypes
import functools

import numpy as np
import pytest

from _rope import rope_ref

pytestmark = pytest.mark.gpu

F16, I8, FP8 = 0, 1, 4  # llm_dtype
EPS = 1e-5
SENTINEL = 0x5A
GUARD = 256
TS, MAX_TILES = 16, 3
NUM_POS = 40          # table rows: positions 40..47 have pages but no table row
K_SCALE, V_SCALE = 0.25, 3.0

SHAPES = [(4, 64), (4, 128), (16, 128)]  # (H, D): hid 256, 512, 2048
PLAIN_M = (1, 16, 17, 32, 33, 64, 100, 512)
LN_M = (1, 16, 17, 32, 33, 64)  # where ln_fusable: 64 KB of fp32 rows per workgroup
# forms (MT, NT, waves) gemm_form gives N = 3 hid, K = hid at these sizes
PLAIN_FORMS = {(1, 1, 8), (1, 1, 4), (1, 2, 8), (2, 1, 8), (4, 2, 8)}
LN_FORMS = {(1, 1, 8), (2, 1, 8), (4, 1, 8)}


def _ln_fits(M, K):
    return (16 if M <= 16 else 32 if M <= 32 else 64) * K * 4 <= 64 * 1024


CASES = [(H, D, M, 0) for H, D in SHAPES for M in PLAIN_M] + \
        [(H, D, M, 1) for H, D in SHAPES for M in LN_M if _ln_fits(M, H * D)]


@pytest.fixture(scope="module")
def tune(gpu):
    import llm_capi
    return llm_capi.load_tune()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Buf:
    """A device output buffer holding `prefill` between two guard margins of
    SENTINEL bytes; read() asserts the margins are intact."""

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


def _nan(*shape):
    return Buf(np.full(shape, np.nan, np.float32))


def _same_bits(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8),
                                  np.ascontiguousarray(b).view(np.uint8), err_msg=what)


def _wg(tune, **fields):
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


def _form(tune, dtype, M, N, K, pro=0):
    out = (ctypes.c_int32 * 5)()
    assert tune.gemm_form_tune(dtype, M, N, K, pro, 0, 0, 0, 0, out) == 0
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _table(D):
    import llm_capi
    t = llm_capi.rope_table(10000.0, D, NUM_POS)
    return t, _dev(t)


@functools.lru_cache(maxsize=None)
def _weights(dtype, hid):
    import llm_capi
    rng = np.random.default_rng(hid * 7 + dtype)
    if dtype == I8:
        W = rng.integers(-127, 128, (hid, 3 * hid), dtype=np.int8)
    else:
        W = (0.05 * rng.standard_normal((hid, 3 * hid))).astype(np.float16)
    sw = rng.uniform(1e-3, 1e-2, 3 * hid).astype(np.float32)
    return llm_capi.pack_weights(_dev(W), dtype), _dev(sw)


@functools.lru_cache(maxsize=None)
def _plain(dtype, H, D, M, pro):
    """(launch fields, y): the operands of one case and the full-width result
    of the launch without a KV append, computed once and shared by its tests."""
    import llm_capi
    tune = llm_capi.load_tune()
    hid = H * D
    Wp, dsw = _weights(dtype, hid)
    rng = np.random.default_rng(hid * 1009 + M * 3 + dtype + 17 * pro)
    f = dict(dtype=dtype, a_packed=1, W_packed=Wp, M=M, N=3 * hid, K=hid)
    if dtype == I8:
        f["sw"] = dsw
    if pro:
        x = (rng.standard_normal((M, hid)) * 2 + 0.5).astype(np.float32)
        g = (1 + 0.1 * rng.standard_normal(hid)).astype(np.float32)
        b = (0.1 * rng.standard_normal(hid)).astype(np.float32)
        f.update(ln_x=_dev(x), ln_g=_dev(g), ln_b=_dev(b))
    elif dtype == I8:
        A = rng.integers(-128, 128, (M, hid), dtype=np.int8)
        f.update(A=llm_capi.pack_weights(_dev(np.ascontiguousarray(A.T)), I8),
                 sa=_dev(rng.uniform(1e-3, 1e-2, M).astype(np.float32)))
    else:
        A = rng.standard_normal((M, hid)).astype(np.float16)
        f.update(A=llm_capi.pack_weights(_dev(np.ascontiguousarray(A.T)), F16))
    full = _nan(M, 3 * hid)
    assert _wg(tune, C=full, **f) == 0, tune.llm_last_error()
    y = full.read().copy()
    assert np.isfinite(y).all()
    return f, y


def _positions(M, seed):
    """pos [M] and the rows whose pages are missing."""
    rng = np.random.default_rng(seed)
    pos = rng.integers(1, NUM_POS, M).astype(np.int32)
    special = [NUM_POS - 1, 0, TS - 1, TS, NUM_POS, 7, -1, TS * MAX_TILES + 3]
    n = min(M, len(special))
    pos[:n] = special[:n]
    missing = {5} if M > 5 else set()
    return pos, missing


def _tables(M, H, use_rows, seed):
    """pos, rows (or None), page table [num_beams][H][MAX_TILES] holding a page
    only for each row's own tile, the table row of each GEMM row, sizes."""
    rng = np.random.default_rng(seed)
    pos, missing = _positions(M, seed)
    num_beams = M + 3
    num_pages = M * H + 5
    pt = np.full((num_beams, H, MAX_TILES), -1, np.int32)
    br = rng.permutation(num_beams)[:M].astype(np.int32) if use_rows else np.arange(M, dtype=np.int32)
    perm = rng.permutation(num_pages)
    for m in range(M):
        p = int(pos[m])
        if m in missing or p < 0 or p // TS >= MAX_TILES:
            continue
        pt[br[m], :, p // TS] = perm[m * H:(m + 1) * H]
    return pos, (br if use_rows else None), pt, br, missing, num_beams, num_pages


def _expected_pool(pool0, vals, pos, br, pt, H, D, stride):
    pool = pool0.copy()
    stored = 0
    for m in range(len(pos)):
        p = int(pos[m])
        if p < 0 or p // TS >= MAX_TILES:
            continue
        for h in range(H):
            page = int(pt[br[m], h, p // TS])
            if page < 0:
                continue
            off = page * stride + (p % TS) * D
            pool[off:off + D] = vals[m, h * D:(h + 1) * D]
            stored += 1
    return pool, stored


def test_every_rope_form_is_reached(gpu, tune):
    for dtype in (I8, F16):
        plain, ln = set(), set()
        for H, D, M, pro in CASES:
            hid = H * D
            f = _form(tune, dtype, M, 3 * hid, hid, pro)
            assert f[3:] == (1, pro), f
            (ln if pro else plain).add(f[:3])
            if pro:
                assert tune.gemm_ln_fusable_tune(dtype, M, hid)
        assert plain == PLAIN_FORMS, (dtype, plain)
        assert ln == LN_FORMS, (dtype, ln)
    # no LayerNorm-prologue launch exists at hid 2048 (its rows do not fit)
    assert not tune.gemm_ln_fusable_tune(I8, 1, 2048)


@pytest.mark.parametrize("pool", ["f16", "fp8"])
@pytest.mark.parametrize("dtype", [I8, F16])
@pytest.mark.parametrize("H,D,M,pro", CASES)
def test_rope_kv_append(gpu, tune, H, D, M, pro, dtype, pool):
    import llm_capi
    fp8 = pool == "fp8"
    hid = H * D
    N = 3 * hid
    f, y = _plain(dtype, H, D, M, pro)
    table, dtable = _table(D)
    stride = TS * D + 32
    for use_rows in (False, True):
        seed = hid + M + 2 * use_rows
        pos, rows, pt, br, missing, num_beams, num_pages = _tables(M, H, use_rows, seed)
        rng = np.random.default_rng(seed)
        garbage = lambda: rng.integers(0, 256 if fp8 else 65536, num_pages * stride).astype(
            np.uint8 if fp8 else np.uint16)
        kp, vp = Buf(garbage()), Buf(garbage())
        # the decoder's form (c_ld = hid) with the rows remap, else a full-width C
        c_ld = hid if use_rows else N
        C = _nan(M, c_ld)
        dpos, dpt = _dev(pos), _dev(pt)
        st = _wg(tune, C=C, c_cols=hid, c_ld=c_ld, has_kv=1, kv_pos=dpos, kv_page_table=dpt,
                 kv_rows=None if rows is None else _dev(rows), kv_k_pool=kp, kv_v_pool=vp,
                 kv_num_beams=num_beams, kv_max_tiles=MAX_TILES, kv_page_size=TS,
                 kv_num_pages=num_pages, kv_H=H, kv_D=D, kv_page_stride=stride,
                 kv_dtype=FP8 if fp8 else F16,
                 kv_k_inv_scale=float(np.float32(1) / np.float32(K_SCALE)),
                 kv_v_inv_scale=float(np.float32(1) / np.float32(V_SCALE)),
                 kv_rope=dtable, kv_rope_len=NUM_POS, **f)
        assert st == 0, tune.llm_last_error()
        what = f"rows={'permuted' if use_rows else 'NULL'}"
        q_ref = rope_ref(y[:, :hid], pos, table)
        k_ref = rope_ref(y[:, hid:2 * hid], pos, table)
        v_ref = y[:, 2 * hid:]
        # the cases bite: rotated rows differ, the row past the table does not
        assert pos[0] == NUM_POS - 1 and not np.array_equal(q_ref[0], y[0, :hid])
        if M > 4:
            assert pos[4] == NUM_POS and np.array_equal(q_ref[4], y[4, :hid])
        c = C.read()
        _same_bits(c[:, :hid], q_ref, what + " q columns")
        _same_bits(c[:, hid:], C.before[:, hid:], what + " C beyond c_cols")
        if fp8:
            k_vals = llm_capi.fp8_encode(k_ref, K_SCALE)
            v_vals = llm_capi.fp8_encode(v_ref, V_SCALE)
        else:
            k_vals = k_ref.astype(np.float16).view(np.uint16)
            v_vals = v_ref.astype(np.float16).view(np.uint16)
        skipped = len(missing) + int(np.count_nonzero((pos < 0) | (pos // TS >= MAX_TILES)))
        for vals, buf, name in ((k_vals, kp, " K pool"), (v_vals, vp, " V pool")):
            want, stored = _expected_pool(buf.before, vals, pos, br, pt, H, D, stride)
            assert stored == (M - skipped) * H, (stored, M, skipped)
            _same_bits(buf.read(), want, what + name)


@pytest.mark.parametrize("H,D,M", [(4, 64, 1), (4, 64, 33), (4, 128, 100), (16, 128, 512)])
def test_rope_rows(gpu, H, D, M):
    """rope_rows over the q and K columns of y (as 2 H heads at row stride
    3 hid) equals rope_ref; the V columns keep their bits."""
    import torch
    import llm_capi
    lib = llm_capi.load()
    hid = H * D
    _, y = _plain(I8, H, D, M, 0)
    table, dtable = _table(D)
    pos, _ = _positions(M, M + 1)
    x = Buf(y)
    dpos = _dev(pos)
    llm_capi.check(lib.rope_rows(x.data_ptr(), 3 * hid, dpos.data_ptr(), M, 2 * H, D,
                                 dtable.data_ptr(), NUM_POS, llm_capi.stream_ptr()))
    torch.cuda.synchronize()
    want = y.copy()
    want[:, :2 * hid] = rope_ref(y[:, :2 * hid], pos, table)
    _same_bits(x.read(), want)


@pytest.mark.parametrize("why", ["no kv", "odd head_dim", "activation"])
def test_rope_refused(gpu, tune, why):
    H, D, M = (2, 64, 16) if why != "odd head_dim" else (128, 1, 16)
    hid = H * D
    f, _ = _plain(I8, 2, 64, M, 0)
    table, dtable = _table(64)
    C = _nan(M, 3 * hid)
    kw = dict(f, C=C, kv_rope=dtable, kv_rope_len=NUM_POS)
    if why != "no kv":
        pos, _, pt, _, _, num_beams, num_pages = _tables(M, H, False, 3)
        pool = Buf(np.zeros(num_pages * TS * D, np.uint16))
        kw.update(has_kv=1, kv_pos=_dev(pos), kv_page_table=_dev(pt), kv_k_pool=pool,
                  kv_v_pool=pool, kv_num_beams=num_beams, kv_max_tiles=MAX_TILES, kv_page_size=TS,
                  kv_num_pages=num_pages, kv_H=H, kv_D=D, c_cols=hid)
    if why == "activation":
        kw["act"] = 1
    assert _wg(tune, **kw) != 0
    assert b"rotary" in tune.llm_last_error()
    assert np.array_equal(C.read().view(np.uint32), C.before.view(np.uint32))
