"""Helpers of tests/test_pa_rows_gpu.py: page pools of every KV element type
with the exact fp32 values the kernels read, and the exact (stage 2) check of
an attention launch's row outputs against its own fp32 rows.

Host-only and numpy-only, so tests/test_pa_rows.py checks them on the CPU."""
from __future__ import annotations

import numpy as np

SENTINEL = 0x5A  # llm_capi.PA_ROWS_SENTINEL: every byte of a row buffer before the launch


def pad16(rows: int) -> int:
    return (rows + 15) // 16 * 16


def rows_ref(ref, out_scale=1.0):
    """The oracle's [B][H][D] heads as float64 rows [B][H*D], times the V scale."""
    ref = np.asarray(ref)
    return ref.astype(np.float64).reshape(ref.shape[0], -1) * float(out_scale)


def pack_a(rows2d: np.ndarray, fill) -> np.ndarray:
    """[rows][K] (int8, or uint16 fp16 bits) in packed-A order, rows padded to
    a multiple of 16 with `fill`: the inverse of oracle.unpack_a_i8 /
    unpack_a_f16 (csrc/common.hpp a_frag_off_i8 / a_frag_off_f16)."""
    rows, K = rows2d.shape
    i8 = rows2d.dtype == np.int8
    step, per = (64, 16) if i8 else (32, 8)
    assert K % step == 0
    r16 = pad16(rows)
    full = np.full((r16, K), fill, rows2d.dtype)
    full[:rows] = rows2d
    m = np.arange(r16)[:, None]
    k = np.arange(K)[None, :]
    off = ((((m >> 4) * (K // step) + k // step) * 64 + (m & 15) + 16 * ((k % step) // per)) * per
           + k % per)
    flat = np.empty(r16 * K, rows2d.dtype)
    flat[off] = full
    return flat


def unpacked_rows(raw: np.ndarray, rows: int, hid: int, pack: int, what="") -> np.ndarray:
    """The [rows][hid] rows of a row buffer as the launch left it (int8, or
    int16 / uint16 fp16 bits -> uint16).  Packed buffers hold pad16(rows) rows:
    all are unpacked and the padding rows must still hold the sentinel."""
    from oracle.oracle import unpack_a_f16, unpack_a_i8
    raw = np.ascontiguousarray(raw)
    i8 = raw.dtype == np.int8
    if not pack:
        assert raw.size == rows * hid, (what, raw.size)
        return (raw if i8 else raw.view(np.uint16)).reshape(rows, hid)
    r16 = pad16(rows)
    assert raw.size == r16 * hid, (what, raw.size)
    full = unpack_a_i8(raw, r16, hid) if i8 else unpack_a_f16(raw, r16, hid).view(np.uint16)
    fill = SENTINEL if i8 else SENTINEL * 0x0101
    assert (full[rows:] == fill).all(), f"{what}: padding rows of a packed output written"
    return full[:rows]


def check_conversions(quantize_rows, out, *, q8=None, inv_scale=None, out16=None, pack=0, what=""):
    """Stage 2, no tolerance: q8 / inv_scale are quantize_rows(out) (the oracle's
    int8_quant.cpp restatement) and out16 is out rounded to fp16, bit for bit.
    out: the launch's own fp32 rows [rows][hid]; q8 / out16: the raw buffers."""
    out = np.ascontiguousarray(out, np.float32)
    rows, hid = out.shape
    if q8 is not None:
        wq, ws = quantize_rows(out)
        got = unpacked_rows(q8, rows, hid, pack, what)
        bad = np.argwhere(got != wq)
        assert bad.size == 0, (f"{what}: {len(bad)} int8 elements differ, first (row, k) "
                               f"{tuple(bad[0])}: {got[tuple(bad[0])]} vs {wq[tuple(bad[0])]}")
        np.testing.assert_array_equal(np.ascontiguousarray(inv_scale, np.float32).view(np.uint32),
                                      np.asarray(ws, np.float32).view(np.uint32),
                                      err_msg=f"{what}: inv_scale bits")
    if out16 is not None:
        got = unpacked_rows(out16, rows, hid, pack, what)
        want = out.astype(np.float16).view(np.uint16)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (f"{what}: {len(bad)} fp16 elements differ, first (row, k) "
                               f"{tuple(bad[0])}: {got[tuple(bad[0])]:#06x} vs "
                               f"{want[tuple(bad[0])]:#06x}")


def page_table(rng, num_beams, H, T, ts, *, shared_groups=False, extra_pages=5):
    """Shuffled page table int32 [num_beams][H][tiles + 2] (the two trailing
    tiles unmapped) over num_beams * H * tiles + extra_pages pages.
    shared_groups: rows 4g+1 .. 4g+3 share the first half of row 4g's pages (a
    forked prefix).  Returns (pt, num_pages, unused page ids)."""
    nt = (T + ts - 1) // ts
    num_pages = num_beams * H * nt + extra_pages
    perm = rng.permutation(num_pages)[: num_beams * H * nt].astype(np.int32)
    pt = np.full((num_beams, H, nt + 2), -1, np.int32)
    pt[:, :, :nt] = perm.reshape(num_beams, H, nt)
    if shared_groups:
        for g in range(0, num_beams - 3, 4):
            pt[g + 1:g + 4, :, :nt // 2] = pt[g, :, :nt // 2]
    unused = np.setdiff1d(np.arange(num_pages), pt[pt >= 0])
    return pt, num_pages, unused


def pool_values(rng, kv, shape, std, unused):
    """One pool of element type kv ("f16", "bf16", "i8", "fp8") as (host array
    to upload, exact fp32 values): N(0, std) values (int8: integers in
    [-4, 4]), the `unused` pages holding garbage 50 times as large (int8: 127,
    fp8: the code of 448), so a wrong page lookup cannot pass."""
    if kv == "i8":
        a = rng.integers(-4, 5, size=shape).astype(np.int8)
        a[unused] = 127
        return a, a.astype(np.float32)
    x = (rng.standard_normal(shape) * std).astype(np.float32)
    if kv == "fp8":
        import llm_capi
        from _fp8 import ref_decode
        b = llm_capi.fp8_encode(x)
        b[unused] = 0x7E
        return b, ref_decode(b)
    x[unused] *= 50
    if kv == "f16":
        h = x.astype(np.float16)
        return h, h.astype(np.float32)
    assert kv == "bf16", kv
    import torch
    t = torch.from_numpy(x).to(torch.bfloat16)
    return t, t.float().numpy()
