"""Helpers of the FP8 (OCP e4m3fn) KV-cache tests: the torch reference of the
format, the boundary rule for append bytes, and readback of an FP8 decoder's
pages.

Reference (include/llm_decoder.h, llm_dtype): byte = e4m3_rne(clamp(y * (1 /
scale), -448, 448)), with 1 / scale computed in fp32.  torch's cast rounds to
nearest even but does not saturate (500 -> NaN), so the clamp is part of the
reference."""
from __future__ import annotations

import ctypes

import numpy as np

FORM_DIRECT, FORM_SPLIT_MERGE, FORM_SPLIT_MERGE_ROW, FORM_WG_MERGE, FORM_BEAM = 0, 1, 2, 3, 16
NAN_CODES = (0x7F, 0xFF)


def ref_encode(y, scale=1.0):
    """uint8 bytes of fp32 `y` at `scale` by the torch reference."""
    import torch
    inv = np.float32(1.0) / np.float32(scale)
    t = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)) * float(inv)
    return torch.clamp(t, -448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def ref_decode(b, scale=1.0):
    """fp32 values of uint8 bytes `b` at `scale` by torch's decode."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(b, dtype=np.uint8)).view(torch.float8_e4m3fn)
    return t.to(torch.float32).numpy() * np.float32(scale)


def boundary_sensitive(pre, scale=1.0):
    """Mask of pre-images whose reference byte changes when the pre-image moves
    one fp32 ulp up or down: the only places where an append byte may differ
    from the reference (the pre-image itself is compared elsewhere)."""
    pre = np.ascontiguousarray(pre, dtype=np.float32)
    b = ref_encode(pre, scale)
    up = ref_encode(np.nextafter(pre, np.float32(np.inf)), scale)
    dn = ref_encode(np.nextafter(pre, np.float32(-np.inf)), scale)
    return (up != b) | (dn != b)


class DecoderConfig(ctypes.Structure):
    """llm_decoder_config (include/llm_decoder.h)."""
    _fields_ = [("num_layers", ctypes.c_int), ("num_heads", ctypes.c_int),
                ("head_dim", ctypes.c_int), ("hidden_dim", ctypes.c_int),
                ("vocab_size", ctypes.c_int), ("max_seq_len", ctypes.c_int),
                ("inter_dim", ctypes.c_int), ("page_size", ctypes.c_int),
                ("weight_dtype", ctypes.c_int), ("max_batch", ctypes.c_int),
                ("attn_scale", ctypes.c_float), ("num_pages", ctypes.c_longlong)]


def fp8_pools(rng, shape, k_std, v_std=1.0):
    """Random K / V pools as FP8 bytes (encoded by the library's host codec) and
    the exact fp32 values they decode to: (k_bytes, v_bytes, k_f32, v_f32)."""
    import llm_capi
    kb = llm_capi.fp8_encode((rng.standard_normal(shape) * k_std).astype(np.float32))
    vb = llm_capi.fp8_encode((rng.standard_normal(shape) * v_std).astype(np.float32))
    return kb, vb, ref_decode(kb), ref_decode(vb)


def dev_fp8(b):
    """Device torch.float8_e4m3fn tensor over uint8 bytes."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(b)).cuda().view(torch.float8_e4m3fn)


def f16_model(rng, L, H, D, V, S):
    """Random fp16 CUDADecoder weights (the oracle's fp16 restatement reads them)."""
    hid, inter = H * D, 4 * H * D
    w = {"cfg": dict(L=L, H=H, D=D, hid=hid, inter=inter, V=V, max_seq=S)}
    w["emb"] = rng.standard_normal((V, hid)).astype(np.float16)
    for k in ("ln1_g", "ln2_g"):
        w[k] = (1 + 0.1 * rng.standard_normal((L, hid))).astype(np.float32)
    for k in ("ln1_b", "ln2_b"):
        w[k] = (0.1 * rng.standard_normal((L, hid))).astype(np.float32)
    for k, shp in (("wqkv", (L, hid, 3 * hid)), ("wo", (L, hid, hid)), ("w1", (L, hid, inter)),
                   ("w2", (L, inter, hid))):
        w[k] = (0.02 * rng.standard_normal(shp)).astype(np.float16)
    w["b1"] = (0.02 * rng.standard_normal((L, inter))).astype(np.float32)
    w["b2"] = (0.02 * rng.standard_normal((L, hid))).astype(np.float32)
    return w


class F16Taps:
    """llm_decoder_set_taps buffers of an FP16 decoder: the four fp16 GEMM inputs
    of every layer as [L][4][B][max(hid, inter)] fp16 (stage 1 = attention rows)."""

    def __init__(self, dec, c, max_batch):
        import torch
        self.L, self.hid, self.inter = c["L"], c["hid"], c["inter"]
        self.K = max(self.hid, self.inter)
        self.b16 = (max_batch + 15) // 16 * 16
        self.q = torch.zeros(self.L * 4 * self.b16 * self.K * 2, dtype=torch.int8, device="cuda")
        self.s = torch.zeros(self.L * 4 * max_batch, dtype=torch.float32, device="cuda")
        dec.set_taps(self.q.data_ptr(), self.s.data_ptr())

    def read(self, B):
        from oracle.oracle import unpack_a_f16
        q = self.q.cpu().numpy().view(np.uint16).reshape(self.L, 4, self.b16 * self.K)
        fh = np.zeros((self.L, 4, B, self.K), np.float16)
        for l in range(self.L):
            for st in range(4):
                Kst = self.inter if st == 3 else self.hid
                fh[l, st, :, :Kst] = unpack_a_f16(q[l, st, :self.b16 * Kst], B, Kst)
        return fh


def make_decoder(w, max_batch, kv_dtype="fp8", cls="INT8Decoder", **kw):
    import llm_decoder
    c = w["cfg"]
    dec = getattr(llm_decoder, cls)(c["L"], c["H"], c["D"], c["hid"], c["V"], c["max_seq"],
                                    max_batch=max_batch, kv_dtype=kv_dtype, **kw)
    d = {k: np.ascontiguousarray(v) for k, v in w.items() if k != "cfg"}
    for k in ("emb", "wqkv", "wo", "w1", "w2"):
        if d[k].dtype == np.float16:
            d[k] = d[k].view(np.uint16)
    dec.set_weights(d)
    return dec


class Pages:
    """Readback of a decoder's KV pages as bytes: pool uint8 [num_pages][2 (K,
    V)][page_size][D * es] and the page table of each layer."""

    def __init__(self, dec, es=1):
        import llm_capi
        from _util import hip_copy_to_host
        self._copy = hip_copy_to_host
        self.lib = llm_capi.load()
        self.kvh = ctypes.c_void_p(dec.kv_handle)
        view = llm_capi.PaKvView()
        llm_capi.check(self.lib.kv_cache_view(self.kvh, 0, ctypes.byref(view)))
        self.view = view
        self.ts, self.D, self.H, self.mt = (view.page_size, view.head_dim, view.num_heads,
                                            view.max_tiles)
        self.beams = view.num_beams
        self.es = es
        self.n_pages = self.lib.kv_cache_num_pages(self.kvh)
        self.stride = self.lib.kv_cache_page_stride(self.kvh)
        assert self.stride == 2 * self.ts * self.D * es, self.stride

    def pool(self):
        p = np.empty((self.n_pages, 2, self.ts, self.D * self.es), np.uint8)
        self._copy(p, self.lib.kv_cache_k_pool(self.kvh))
        return p

    def table(self, layer):
        pt = np.empty((self.beams, self.H, self.mt), np.int32)
        self._copy(pt, self.lib.kv_cache_page_table(self.kvh, layer))
        return pt

    def at(self, pool, rows, pos, L):
        """Bytes at position pos[r] of each row: uint8 [L][rows][2][H][D]."""
        out = np.empty((L, rows, 2, self.H, self.D * self.es), np.uint8)
        for layer in range(L):
            pt = self.table(layer)
            for r in range(rows):
                p = int(pos[r])
                ids = pt[r, :, p // self.ts]
                assert (ids >= 0).all()
                out[layer, r] = pool[ids, :, p % self.ts].transpose(1, 0, 2)
        return out

    def context(self, pool, layer, rows, T, row0=0):
        """Bytes of positions [0, T) of rows row0 .. row0 + rows - 1: uint8
        [2][rows][H][T][D]."""
        nt = (T + self.ts - 1) // self.ts
        ids = self.table(layer)[row0:row0 + rows, :, :nt]
        assert (ids >= 0).all() and (ids < self.n_pages).all()
        out = []
        for which in (0, 1):
            pages = pool[ids, which]  # [rows][H][nt][ts][D]
            out.append(pages.reshape(rows, self.H, nt * self.ts, -1)[:, :, :T])
        return np.stack(out)


def fp8_kv_to_oracle(pages, odec, rows, T, k_scale, v_scale, exact=True):
    """decoder_kv_to_oracle for an FP8 decoder: decode positions [0, T) of every
    row and layer with the layer's scales into the oracle's fp16 KV (exact for
    power-of-two scales in [2^-4, 2^2]: 448 * 4 < 65504, 2^-13 is an fp16 value;
    exact=False for other scales: each element then rounds to fp16, 2^-11 relative)."""
    pool = pages.pool()
    for layer in range(odec.cfg["L"]):
        ctx = pages.context(pool, layer, rows, T)
        for which, sc in ((0, k_scale[layer]), (1, v_scale[layer])):
            val = ref_decode(ctx[which], sc)
            h = val.astype(np.float16)
            assert not exact or np.array_equal(h.astype(np.float32), val), "scale not exact in fp16"
            odec.kv(layer, which)[:rows, :, :T] = h
