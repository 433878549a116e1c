"""Sliding-window test helpers.

The oracle knows no window, and stays that way: the reference for a windowed
row is the oracle's plain paged attention over a SHIFTED COPY of the row --
tokens [t_lo, T_b) written to a fresh pool at positions [0, T_b - t_lo), with
context T_b - t_lo."""
from __future__ import annotations

import numpy as np


def t_lo_of(T_b: int, W: int) -> int:
    return max(0, T_b - W) if W > 0 else 0


def shifted_copy(kf, vf, pt, lens, W, beam_ids=None):
    """(k_pool, v_pool, page_table, context_lens) of the shifted copy: row b of
    the new table holds tokens [t_lo, T_b) of page-table row beam_ids[b] (b) at
    positions 0 .. .  kf / vf: float pools [num_pages][ts][D], pt int32
    [beams][H][max_tiles], lens [B].  A missing page (-1) inside a window is
    carried over as a missing tile, which needs t_lo on a page edge (the copy
    moves whole tokens, the table marks whole tiles)."""
    kf = np.asarray(kf, np.float32)
    vf = np.asarray(vf, np.float32)
    lens = np.asarray(lens, np.int64)
    B = len(lens)
    _, ts, D = kf.shape
    H = pt.shape[1]
    rows = np.arange(B) if beam_ids is None else np.asarray(beam_ids)
    n = [int(T - t_lo_of(int(T), W)) for T in lens]
    nt = max(1, max((x + ts - 1) // ts for x in n))
    kp = np.zeros((B * H * nt, ts, D), np.float32)
    vp = np.zeros_like(kp)
    npt = np.full((B, H, nt), -1, np.int32)
    for b in range(B):
        T, lo = int(lens[b]), t_lo_of(int(lens[b]), W)
        if T <= 0:
            continue
        for h in range(H):
            t0 = lo // ts  # the row's first live tile; its tokens start at t0 * ts
            old = pt[rows[b], h, t0: (T + ts - 1) // ts]
            present = np.repeat(old >= 0, ts)[lo - t0 * ts: T - t0 * ts]
            if not present.all():
                assert lo % ts == 0, "a missing page inside the window needs t_lo on a page edge"
            safe = np.where(old >= 0, old, 0)
            ktok = kf[safe].reshape(-1, D)[lo - t0 * ts: T - t0 * ts]
            vtok = vf[safe].reshape(-1, D)[lo - t0 * ts: T - t0 * ts]
            for j in range((n[b] + ts - 1) // ts):
                seg = slice(j * ts, min((j + 1) * ts, n[b]))
                if not present[seg].all():
                    continue
                page = (b * H + h) * nt + j
                npt[b, h, j] = page
                kp[page, : seg.stop - seg.start] = ktok[seg]
                vp[page, : seg.stop - seg.start] = vtok[seg]
    return kp, vp, npt, np.asarray(n, np.int32)


def window_reference(oracle, q, kf, vf, pt, lens, W, beam_ids=None, temperature=1.0):
    """Oracle.paged_attention over the shifted copy: fp32 [B][H][D]."""
    kp, vp, npt, n = shifted_copy(kf, vf, pt, lens, W, beam_ids)
    return oracle.paged_attention(q, kp, vp, npt, T=max(1, int(n.max())), context_lens=n,
                                  temperature=temperature)


def stage1_stats(oracle, w, fq, fs, hist, pos, W, table=None, attn_scale=1.0):
    """tests/_rope.py::stage1_stats for a windowed INT8 decoder (q rotated by
    `table` as there; None: no rotation): what the o_proj must have been fed,
    from the step's own stage-0 tap -- per layer qkv = i8_gemm(tapped A, wqkv) (exact), attention over the last W
    tokens of the history (_rope.KvHistory, which already holds this step's
    K / V) and the row quantiser, compared with the stage-1 tap.  W = 0: the
    whole history, which is the oracle's own stage 1 (the anchor).  attn_scale:
    the decoder's score multiplier (the oracle's temperature^-2).
    Returns (qkv [L][B][3 hid], stats [L][3]) as that helper does."""
    c = w["cfg"]
    L, H, D, hid = c["L"], c["H"], c["D"], c["hid"]
    B = fq.shape[2]
    qkv = np.empty((L, B, 3 * hid), np.float32)
    stats = np.zeros((L, 3), np.float32)
    lens = np.full(B, pos + 1, np.int32)
    for l in range(L):
        qkv[l] = oracle.i8_gemm(fq[l, 0, :, :hid], w["wqkv"][l], fs[l, 0], w["sw_qkv"][l])[1]
        q = qkv[l, :, :hid]
        if table is not None:
            from _rope import rope_ref
            q = rope_ref(q, np.full(B, pos), table)
        q = q.reshape(B, H, D)
        if W > 0:
            o = window_reference(oracle, q, hist.k[l], hist.v[l], hist.pt, lens, W,
                                 temperature=attn_scale ** -0.5)
        else:
            o = oracle.paged_attention(q, hist.k[l], hist.v[l], hist.pt, T=pos + 1,
                                       temperature=attn_scale ** -0.5)
        q1, s1 = oracle.quantize_rows(o.reshape(B, hid))
        d = np.abs(q1.astype(np.int32) - fq[l, 1, :, :hid].astype(np.int32))
        stats[l] = (np.count_nonzero(d), d.max(),
                    np.max(np.abs(fs[l, 1] - s1) / np.maximum(np.abs(s1), 1e-30)))
    return qkv, stats


def t_prime(T: int, W: int, ts: int) -> int:
    """The context whose plan a window-W launch of context T takes: a window
    touches at most ceil(W / ts) + 1 tiles."""
    return min(T, ((W + ts - 1) // ts + 1) * ts) if W > 0 else T
