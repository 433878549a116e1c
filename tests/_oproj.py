"""Helpers of tests/test_oproj_rows_gpu.py: the fused o_proj of the attention's
workgroup merge (csrc/pa_split.hpp, PaOut::OPROJ) restated on the host -- the
W_o head-slice layout, the counted fixed-point accumulator of csrc/common.hpp
(oacc_term / oacc_count / oacc_value) in Python integers, the float64 product
with its derived error bound, and the builder of the exact cases.

Host-only and numpy-only, so tests/test_oproj.py checks them on the CPU."""
from __future__ import annotations

import math
import types

import numpy as np

SCALE_BITS = 32          # kOAccScale = 2^32
COUNT = 1 << 56          # kOAccCount: one arrival
RANGE = (1 << 23) - 1    # |sum| the 56 bits below the count hold, in units of 1


def slices_ref(wo, H, D):
    """[H*D][o_n] -> [H][D/8][o_n][8]: out[h][kg][n][j] = wo[h D + 8 kg + j][n]."""
    wo = np.asarray(wo)
    assert wo.ndim == 2 and wo.shape[0] == H * D and D % 8 == 0
    return np.ascontiguousarray(wo.reshape(H, D // 8, 8, wo.shape[1]).transpose(0, 1, 3, 2))


def oacc_limit(H):
    """oacc_limit: (2^23 - 1) / H in fp32."""
    return np.float32(RANGE) / np.float32(H)


def term_ref(p, H):
    """oacc_term of one head's fp32 product p: (the int64 term, clamped).  A
    value past the limit goes to the limit of its sign; NaN (which is neither
    <= lim nor < 0) to the positive one."""
    p = float(np.float32(p))
    lim = float(oacc_limit(H))
    ok = abs(p) <= lim  # False for NaN and +-inf
    c = p if ok else (-lim if p < 0 else lim)
    # c * 2^32 is exact in fp32 (a power of two); __float2ll_rn rounds half to even
    return int(np.rint(np.float64(c) * 2.0 ** SCALE_BITS)) + COUNT, not ok


def count_ref(v):
    """oacc_count: arrivals in a column value (Python's >> floors, as the device's)."""
    return (v + (COUNT >> 1)) >> 56


def _round_f32(num, shift):
    """num / 2^shift (Python int) rounded once to fp32, half to even."""
    if num == 0:
        return np.float32(0.0)
    a = abs(num)
    drop = a.bit_length() - 24
    if drop > 0:
        q, rem, half = a >> drop, a & ((1 << drop) - 1), 1 << (drop - 1)
        if rem > half or (rem == half and (q & 1)):
            q += 1
        a, shift = q, shift - drop
    return np.float32(math.copysign(math.ldexp(a, -shift), num))


def value_ref(v):
    """oacc_value: the signed sum below the count, in units of 2^-32, as fp32.
    (The device converts through double first: the same value whenever the sum
    has at most 53 significant bits, |sum| < 2^21 at the latest.)"""
    return _round_f32(v - count_ref(v) * COUNT, SCALE_BITS)


def fixed_point_ref(terms, H=None):
    """The column value H heads leave: terms = their fp32 products, in any
    order.  Returns (x fp32, clamped flag, count, the raw int sum)."""
    terms = list(terms)
    H = len(terms) if H is None else H
    v, flag = 0, False
    for p in terms:
        t, c = term_ref(p, H)
        v += t
        flag |= c
    assert -(1 << 63) <= v < (1 << 63)
    return value_ref(v), flag, count_ref(v), v


def head_terms(o16, wo, H, D):
    """Each head's product [B][H][o_n] in float64 (exact wherever the fp32 sums
    are: exact cases), NaN / inf propagated as IEEE does."""
    B, o_n = o16.shape[0], wo.shape[1]
    o = np.asarray(o16, np.float64).reshape(B, H, D)
    w = np.asarray(wo, np.float64).reshape(H, D, o_n)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.einsum("bhd,hdn->bhn", o, w)


def x_fixed_ref(terms, H):
    """fixed_point_ref of every [b][:, n] of head_terms' result rounded to
    fp32: (x fp32 [B][o_n], clamped [B][o_n])."""
    with np.errstate(over="ignore"):
        t32 = np.asarray(terms).astype(np.float32)
    B, _, o_n = t32.shape
    x = np.empty((B, o_n), np.float32)
    cl = np.zeros((B, o_n), bool)
    for b in range(B):
        for n in range(o_n):
            x[b, n], cl[b, n], cnt, _ = fixed_point_ref(t32[b, :, n], H)
            assert cnt == H
    return x, cl


def x_ref64(o16, wo):
    """The o_proj in float64: fp16 rows [B][H*D] times fp16 W_o [H*D][o_n]."""
    return np.asarray(o16, np.float64) @ np.asarray(wo, np.float64)


def x_bound(o16, wo, H, D):
    """Elementwise bound of |x - x_ref64|, derived (not measured):
      sum_h D 2^-24 S_h   S_h = sum_k |o16[hD+k] wo[hD+k][n]|: fp16 products are
                          exact in fp32; a two-element dot rounds at most twice
                          (after each addition), D roundings per head, each at
                          most 2^-24 of a partial sum that S_h bounds;
      + H 2^-33           each head's term rounded to a multiple of 2^-32;
      + 2^-24 |ref|       the completed sum rounded to fp32."""
    S = np.abs(np.asarray(o16, np.float64)) @ np.abs(np.asarray(wo, np.float64))
    return D * 2.0 ** -24 * S + H * 2.0 ** -33 + 2.0 ** -24 * np.abs(x_ref64(o16, wo))


def assert_fp32_exact(v, wo, H, D):
    """Every product of v (integers) and wo (multiples of 2^-6) is a multiple
    of 2^-6, so every sum of any subset of a head's products, in any order and
    grouping, and of the heads' totals, is one too; below 2^18 in magnitude it
    has at most 24 significant bits: exact in fp32, whatever the dot
    instruction rounds, and exact in the 2^-32 fixed point."""
    v = np.asarray(v, np.float64)
    w = np.asarray(wo, np.float64)
    assert (v == np.rint(v)).all() and (w * 64 == np.rint(w * 64)).all()
    S = np.einsum("rhd,hdn->rhn", np.abs(v).reshape(v.shape[0], H, D),
                  np.abs(w).reshape(H, D, w.shape[1]))
    assert S.max() <= 2048 and S.sum(axis=1).max() < 2.0 ** 18, (S.max(), S.sum(axis=1).max())
    assert S.max() <= float(oacc_limit(H))  # no term clamps


def exact_case(rng, rows, H, D, o_n, r0=0):
    """V vectors int [rows][H][D] in [-8, 8] (one per page-table row and head:
    every token of that row holds it, so the merged head is v L / (L + 1e-6)
    and rounds to v in fp16) and W_o fp16 [H*D][o_n] of multiples of 2^-6 in
    [-2, 2].  Row r0 is shaped so that, with m_k in 1 .. 8 and s_k = sign(v):
      column 1 (o_n >= 2): W_o = -m s / 64 in every head, so every head's term
          and the total are negative (v[r0] is nowhere zero);
      column 0 (H >= 2): head 1 holds head 0's V, W_o = m s / 64 in head 0, its
          negative in head 1 and 0 in the others: two non-zero terms, total 0.
    Returns v, wo and x = v @ wo exactly (fp32 [rows][o_n])."""
    v = rng.integers(-8, 9, size=(rows, H, D)).astype(np.int32)
    v[r0][v[r0] == 0] = 3
    if H >= 2:
        v[r0, 1] = v[r0, 0]
    wq = rng.integers(-128, 129, size=(H, D, o_n)).astype(np.int32)  # 64 W_o
    m = rng.integers(1, 9, size=(H, D)).astype(np.int32)
    s = np.sign(v[r0])
    if o_n >= 2:
        wq[:, :, 1] = -m * s
    if H >= 2:
        wq[:, :, 0] = 0
        wq[0, :, 0] = m[0] * s[0]
        wq[1, :, 0] = -wq[0, :, 0]
    wo = (wq.reshape(H * D, o_n) / 64.0).astype(np.float16)
    assert (wo.astype(np.float64) * 64 == wq.reshape(H * D, o_n)).all()
    x64 = v.reshape(rows, H * D).astype(np.float64) @ wo.astype(np.float64)
    x = x64.astype(np.float32)
    assert (x.astype(np.float64) == x64).all()
    if o_n >= 2:
        assert x[r0, 1] < 0
    if H >= 2:
        assert x[r0, 0] == 0 and float(v[r0, 0] @ wq[0, :, 0]) > 0
    return types.SimpleNamespace(v=v, wo=wo, x=x)
