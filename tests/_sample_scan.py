"""Host model of the sampler's kept-mass scan (csrc/sample.hip) for rows whose
probabilities are bit-determined, used only to CHOOSE test inputs.

Rows: every logit 0.0 or -inf, temperature 1, no filter.  Then on any IEEE
device expf(0) = 1, the softmax sum s is an exact integer, every kept
probability is the one fp32 constant 1 / (s + 1e-6), and the per-thread sums
and the Hillis-Steele scan are reproducible in numpy float32.

claim_gaps() lists the 24-bit uniforms u whose target u * Z falls between the
claims `lo <= target < lo + part` of two neighbouring threads, as the kernel
formed them before the claims were made to tile [0, Z): `lo + part` is one
fp32 add, the next thread's `lo` is the scan's association of the same terms,
and where the former is smaller a target in between belongs to no thread.
find_draws() searches the draw hash for (row, counter) pairs that land there.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
THREADS = 512  # kSampleThreads
_U = np.uint64


def sample_vpt(V: int) -> int:
    """Tokens per thread of the instantiation launch_sample_rows picks."""
    need = (V + THREADS - 1) // THREADS
    for v in (16, 32, 64, 128):
        if need <= v:
            return v
    raise ValueError("V > 65536")


def banned_row(V: int, banned) -> np.ndarray:
    lg = np.zeros(V, f32)
    lg[np.asarray(banned, np.int64)] = -np.inf
    return lg


def scan_model(logits: np.ndarray):
    """(part, scan, Z) in float32 as the kernel computes them for a 0 / -inf row
    at temperature 1 without filters; thread t owns tokens [t*VPT, (t+1)*VPT)."""
    V = len(logits)
    assert np.all((logits == 0) | np.isneginf(logits)) and np.any(logits == 0)
    vpt = sample_vpt(V)
    kept = np.zeros(THREADS * vpt, bool)
    kept[:V] = logits == 0
    s = f32(int(kept.sum()))  # a sum of ones: exact in any order
    p = f32(1.0) * (f32(1.0) / (s + f32(1e-6)))
    pt = np.where(kept, p, f32(0)).astype(f32).reshape(THREADS, vpt)
    part = np.zeros(THREADS, f32)
    for i in range(vpt):  # sequential, ascending token index
        part = (part + pt[:, i]).astype(f32)
    scan = part.copy()
    off = 1
    while off < THREADS:  # Hillis-Steele inclusive scan
        sh = np.zeros(THREADS, f32)
        sh[off:] = scan[:-off]
        scan = (scan + sh).astype(f32)
        off *= 2
    return part, scan, scan[-1]


def claim_gaps(logits: np.ndarray) -> np.ndarray:
    """Indices i (u = i / 2^24) of the uniforms no thread claims under the rule
    `part > 0 && target >= lo && (target < lo + part || last thread || scan >= Z)`."""
    part, scan, Z = scan_model(logits)
    lo = np.concatenate([[f32(0)], scan[:-1]]).astype(f32)
    hi = (lo + part).astype(np.float64)
    hi[(np.arange(THREADS) == THREADS - 1) | (scan >= Z)] = np.inf
    act = part > 0
    lo_a = lo[act]
    hi_a = np.maximum.accumulate(hi[act])  # any earlier thread's claim counts too
    u = (np.arange(1 << 24, dtype=np.float64) / (1 << 24)).astype(f32)
    tgt = (u * Z).astype(f32)
    idx = np.searchsorted(lo_a, tgt, side="right") - 1  # last active thread with lo <= target
    claimed = (idx >= 0) & (tgt < hi_a[np.maximum(idx, 0)])
    return np.nonzero(~claimed)[0]


def uniform_index(seed: int, row: int, counters: np.ndarray) -> np.ndarray:
    """i with sample_uniform(seed, row, counter) = i / 2^24 (csrc/sample.hip)."""
    z = _U(seed) ^ (_U(row & 0xFFFFFFFF) << _U(32)) ^ counters.astype(_U)
    with np.errstate(over="ignore"):
        z = z + _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
    z ^= z >> _U(31)
    return (z >> _U(40)).astype(np.int64)


def find_draws(seed: int, wanted: np.ndarray, rows=4, counters=1 << 22):
    """[(row, counter, i)] in (row, counter) order whose uniform index i is in `wanted`."""
    mask = np.zeros(1 << 24, bool)
    mask[wanted] = True
    c = np.arange(counters, dtype=_U)
    hits = []
    for row in range(rows):
        ui = uniform_index(seed, row, c)
        for ctr in np.nonzero(mask[ui])[0]:
            hits.append((row, int(ctr), int(ui[ctr])))
    return hits
