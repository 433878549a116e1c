"""The prefill pass packer (csrc/prefill_pack.hpp) through the tuning library's
prefill_passes_tune: the passes the decoder's prefill and prefill_rows run.

Rows go in the given order, a length of 0 adds nothing, a row that does not
fit continues in the next pass at its new position (so a row is in a pass at
most once), and every pass but the last holds exactly `cap` tokens.  The first
two exact cases are test_prefill_packed_decoder_gpu.py's RAGGED and SHORT
prompt lengths minus one (generate prefills prompt[:-1]).
"""
import ctypes
import random

import pytest

import llm_capi


def passes(lens, starts, cap):
    """[[(row index, p0, len), ...] per pass] for rows of lens[i] tokens from starts[i]."""
    tune = llm_capi.load_tune()
    n = len(lens)
    arr = ctypes.c_int32 * max(n, 1)
    st, ln = arr(*starts), arr(*lens)
    room = sum(lens) + 1  # a segment holds >= 1 token
    out = (ctypes.c_int32 * (4 * room))()
    nseg = tune.prefill_passes_tune(st, ln, n, cap, out, room)
    assert 0 <= nseg < room
    res = []
    for i in range(nseg):
        p, row, p0, m = out[4 * i:4 * i + 4]
        assert p in (len(res) - 1, len(res)), "passes are numbered in order from 0"
        if p == len(res):
            res.append([])
        res[p].append((row, p0, m))
    return res


def test_ragged():
    assert passes((599, 36, 0, 512, 199), [0] * 5, 512) == [
        [(0, 0, 512)],
        [(0, 512, 87), (1, 0, 36), (3, 0, 389)],
        [(3, 389, 123), (4, 0, 199)]]


def test_short_rows_share_one_pass():
    lens = (1, 16, 32, 63, 64, 8)
    assert passes(lens, [0] * 6, 184) == [[(i, 0, n) for i, n in enumerate(lens)]]


def test_many_equal_rows():
    ps = passes([127] * 64, [0] * 64, 512)
    assert len(ps) == 16
    assert [sum(s[2] for s in p) for p in ps] == [512] * 15 + [448]
    assert all(len(p) <= 6 for p in ps)


def test_one_long_row():
    assert passes((8191,), (0,), 512) == [[(0, 512 * i, min(512, 8191 - 512 * i))]
                                          for i in range(16)]


def test_start_position():
    assert passes((5,), (100,), 5) == [[(0, 100, 5)]]


@pytest.mark.parametrize("lens,starts,cap", [((0, 0, 0), (0, 7, 3), 512), ((0,), (5,), 1),
                                             ((), (), 512), ((), (), 1)])
def test_nothing_to_do(lens, starts, cap):
    assert passes(lens, starts, cap) == []


def test_output_capacity_is_respected():
    tune = llm_capi.load_tune()
    st, ln = (ctypes.c_int32 * 3)(0, 0, 0), (ctypes.c_int32 * 3)(4, 4, 4)
    out = (ctypes.c_int32 * 12)(*([-7] * 12))
    assert tune.prefill_passes_tune(st, ln, 3, 3, out, 2) == 6  # 3 + 1, 2 + 2, 1 + 3
    assert list(out) == [0, 0, 0, 3, 1, 0, 3, 1] + [-7] * 4
    assert tune.prefill_passes_tune(st, ln, 3, 3, None, 0) == 6
    assert tune.prefill_passes_tune(st, ln, 3, 0, out, 2) == -1  # no capacity per pass


def test_properties_random():
    rng = random.Random(20251)
    for _ in range(300):
        cap = rng.choice([1, 2, 5, 16, 64, 512])
        n = rng.randrange(0, 12)
        lens = [rng.choice([0, 0, 1, rng.randrange(1, cap + 1), rng.randrange(cap, 2 * cap + 1),
                            rng.randrange(2 * cap + 1, 5 * cap + 2)]) for _ in range(n)]
        starts = [rng.choice([0, rng.randrange(0, 1000)]) for _ in range(n)]
        ps = passes(lens, starts, cap)
        sizes = [sum(s[2] for s in p) for p in ps]
        assert all(0 < z <= cap for z in sizes), (lens, cap)
        assert all(z == cap for z in sizes[:-1]), (lens, cap)
        assert sum(sizes) == sum(lens)
        for p in ps:
            rows = [s[0] for s in p]
            assert len(set(rows)) == len(rows), "a row twice in a pass"
        flat = [s for p in ps for s in p]
        assert all(s[2] >= 1 for s in flat)
        order = [s[0] for s in flat]
        assert order == sorted(order), "rows out of input order"
        nxt = list(starts)  # per row: the segments tile [start, start + len) in order
        for row, p0, m in flat:
            assert p0 == nxt[row], (lens, starts, cap)
            nxt[row] += m
        assert nxt == [s + l for s, l in zip(starts, lens)]
