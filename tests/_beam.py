"""Beam search restated in plain Python (include/llm_decoder.h,
llm_decoder_beam_search): the float64 candidate selection of one step and the
host bookkeeping, for the tests of the device kernel and of the search."""
from __future__ import annotations

import numpy as np


def select_ref(logits, score_in, W):
    """float64 restatement of beam_select_rows.  logits [num_seqs * W][V], score_in
    [num_seqs * W] (-inf: the beam is not live).  Per row the 2W largest raw
    logits (ties: lower token id); candidate score = score_in + (x - m) -
    log(sum exp(x - m) + 1e-6); per sequence the W * 2W candidates ranked by
    (score desc, parent asc, token asc).  Returns (score float64, parent, token),
    each [num_seqs][W * 2W] -- the FULL ranking, the first 2W being the result."""
    logits = np.asarray(logits, np.float64)
    score_in = np.asarray(score_in, np.float64)
    R, V = logits.shape
    S, K = R // W, 2 * W
    out_s = np.full((S, W * K), -np.inf)
    out_p = np.zeros((S, W * K), np.int64)
    out_t = np.zeros((S, W * K), np.int64)
    for s in range(S):
        cands = []
        for b in range(W):
            r = s * W + b
            if score_in[r] == -np.inf:
                cands += [(-np.inf, b, j) for j in range(K)]
                continue
            x = logits[r]
            m = x.max()
            lse = np.log(np.exp(x - m).sum() + 1e-6)
            top = np.lexsort((np.arange(V), -x))[:K]  # by -x, then by token id
            cands += [(score_in[r] + ((x[t] - m) - lse), b, int(t)) for t in top]
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        for j, (sc, b, t) in enumerate(cands):
            out_s[s, j], out_p[s, j], out_t[s, j] = sc, b, t
    return out_s, out_p, out_t


def final_score(sum_logprob, length, alpha):
    """sum_logprob / length^alpha, in double, stored as float32 (the library's rounding)."""
    return np.float32(np.float64(np.float32(sum_logprob)) / np.float64(length) ** np.float64(alpha))


def bookkeeping(cand_score, cand_parent, cand_token, W, max_new, eos_token, length_penalty):
    """The host side of the search, fed the candidates the device reported
    (arrays [steps][num_seqs][2W]).  Per sequence and step, candidates in rank
    order: EOS joins the finished set if rank < W (ignored otherwise, and
    always once the sequence is done), anything else becomes the next live
    beam until W are live.  A sequence with >= W finished hypotheses is done.
    The search ends when all are done or after max_new steps; a sequence that
    is not done adds its live beams (beam order).  Best W by final score
    (stable) are returned.

    Returns dict(live_parent, live_token [steps][S][W], ids (lists), length,
    sum_logprob, score [S][W], steps)."""
    cand_score = np.asarray(cand_score, np.float32)
    steps_avail, S, K = cand_score.shape
    assert K == 2 * W
    hist = [[[] for _ in range(W)] for _ in range(S)]
    score = np.zeros((S, W), np.float32)
    finished = [[] for _ in range(S)]
    done = [False] * S
    live_parent, live_token = [], []
    steps = 0
    for st in range(min(max_new, steps_avail)):
        lp = np.zeros((S, W), np.int32)
        lt = np.zeros((S, W), np.int32)
        for s in range(S):
            nxt, nsc = [], []
            for j in range(K):
                sc = cand_score[st, s, j]
                p, t = int(cand_parent[st, s, j]), int(cand_token[st, s, j])
                if t == eos_token:
                    if j < W and not done[s]:
                        ids = hist[s][p] + [t]
                        finished[s].append((ids, sc, final_score(sc, len(ids), length_penalty)))
                elif len(nxt) < W:
                    lp[s, len(nxt)], lt[s, len(nxt)] = p, t
                    nxt.append(hist[s][p] + [t])
                    nsc.append(sc)
            assert len(nxt) == W
            hist[s] = nxt
            score[s] = nsc
            if len(finished[s]) >= W:
                done[s] = True
        live_parent.append(lp)
        live_token.append(lt)
        steps = st + 1
        if all(done):
            break
    ids, length = [], np.zeros((S, W), np.int32)
    sums, finals = np.zeros((S, W), np.float32), np.zeros((S, W), np.float32)
    for s in range(S):
        pool = list(finished[s])
        if not done[s]:
            pool += [(hist[s][w], score[s, w],
                      final_score(score[s, w], len(hist[s][w]), length_penalty)) for w in range(W)]
        pool.sort(key=lambda h: -float(h[2]))  # stable: equal scores keep their order
        ids.append([list(h[0]) for h in pool[:W]])
        for w, h in enumerate(pool[:W]):
            length[s, w], sums[s, w], finals[s, w] = len(h[0]), h[1], h[2]
    return dict(live_parent=np.array(live_parent), live_token=np.array(live_token), ids=ids,
                length=length, sum_logprob=sums, score=finals, steps=steps, done=done)
