"""Rotary position embedding: the numpy float32 statement of the semantics
(include/llm_decoder.h, rope_rows / llm_decoder_set_rope) and the helpers the
rotary tests share.

The table is float32 [num_pos][D]; for position t and even d, c = table[t][d]
and s = table[t][d + 1], and a head vector x at position t becomes

    x'[d]     = x[d] * c - x[d + 1] * s
    x'[d + 1] = x[d] * s + x[d + 1] * c

with every product rounded to float32 on its own and then one float32 add or
subtract (no fma): numpy float32 arithmetic, which rounds after every
operation, reproduces the device's bits.  A position outside [0, num_pos)
leaves the vector as it is."""
from __future__ import annotations

import numpy as np


def table_f64(theta, D, num_pos):
    """The standard table in float64: angle(t, i) = t * theta^(-2 i / D)."""
    i = np.arange(D // 2, dtype=np.float64)
    ang = np.arange(num_pos, dtype=np.float64)[:, None] * np.power(float(theta), -2.0 * i / D)
    out = np.empty((num_pos, D), np.float64)
    out[:, 0::2] = np.cos(ang)
    out[:, 1::2] = np.sin(ang)
    return out


def identity_table(num_pos, D):
    t = np.zeros((num_pos, D), np.float32)
    t[:, 0::2] = 1.0
    return t


def rope_ref(x, pos, table):
    """x float32 [rows][..., D] (any number of head axes, or [rows][H * D] with
    H * D a multiple of D), pos int [rows], table float32 [num_pos][D]."""
    x = np.asarray(x)
    table = np.asarray(table)
    assert x.dtype == np.float32 and table.dtype == np.float32
    num_pos, D = table.shape
    assert D % 2 == 0 and x.shape[-1] % D == 0
    rows = x.shape[0]
    v = x.reshape(rows, -1, D)
    out = v.copy()
    pos = np.asarray(pos).reshape(rows)
    for r in range(rows):
        p = int(pos[r])
        if p < 0 or p >= num_pos:
            continue
        c, s = table[p, 0::2], table[p, 1::2]
        x0, x1 = v[r, :, 0::2], v[r, :, 1::2]
        out[r, :, 0::2] = x0 * c - x1 * s
        out[r, :, 1::2] = x0 * s + x1 * c
    assert out.dtype == np.float32
    return out.reshape(x.shape)


class KvHistory:
    """The K / V a stepping decoder appended, kept on the host as one page per
    (layer, row, head, tile) so that Oracle.paged_attention can run over
    them: pools float32 [L][pages][ts][D] holding the fp16 values."""

    def __init__(self, L, B, H, D, max_seq, ts=16):
        self.L, self.B, self.H, self.D, self.ts = L, B, H, D, ts
        self.nt = (max_seq + ts - 1) // ts
        self.k = np.zeros((L, B * H * self.nt, ts, D), np.float32)
        self.v = np.zeros_like(self.k)
        self.pt = np.arange(B * H * self.nt, dtype=np.int32).reshape(B, H, self.nt)

    def append(self, kv, pos):
        """kv fp16 [L][B][2][H][D] (decoder_kv_at), pos [B]."""
        for b in range(self.B):
            p = int(pos[b])
            for h in range(self.H):
                page = self.pt[b, h, p // self.ts]
                self.k[:, page, p % self.ts] = kv[:, b, 0, h].astype(np.float32)
                self.v[:, page, p % self.ts] = kv[:, b, 1, h].astype(np.float32)


def stage1_stats(oracle, w, fq, fs, hist, pos, table=None, layers=None):
    """What the decoder's o_proj must have been fed, from the step's own stage-0
    tap: per layer, qkv = i8_gemm(tapped A, wqkv) (exact), q rotated by `table`
    (None: not), attention over the history (which already holds this step's
    K / V) and the row quantiser, compared with the stage-1 tap.

    Returns (qkv [L][B][3 hid], stats [L][3]) with stats as OracleDecoder's:
    int8 values that differ, their max |difference|, max relative difference of
    the row scales.  Every row is at the same position pos; layers: the layers
    to compute (default all)."""
    c = w["cfg"]
    L, H, D, hid = c["L"], c["H"], c["D"], c["hid"]
    B = fq.shape[2]
    qkv = np.empty((L, B, 3 * hid), np.float32)
    stats = np.zeros((L, 3), np.float32)
    for l in range(L) if layers is None else layers:
        qkv[l] = oracle.i8_gemm(fq[l, 0, :, :hid], w["wqkv"][l], fs[l, 0], w["sw_qkv"][l])[1]
        q = qkv[l, :, :hid]
        if table is not None:
            q = rope_ref(q, np.full(B, pos), table)
        o = oracle.paged_attention(q.reshape(B, H, D), hist.k[l], hist.v[l], hist.pt, T=pos + 1)
        q1, s1 = oracle.quantize_rows(o.reshape(B, hid))
        d = np.abs(q1.astype(np.int32) - fq[l, 1, :, :hid].astype(np.int32))
        stats[l] = (np.count_nonzero(d), d.max(),
                    np.max(np.abs(fs[l, 1] - s1) / np.maximum(np.abs(s1), 1e-30)))
    return qkv, stats
