"""CPU checks of tests/_pa_rows.py, the host side of tests/test_pa_rows_gpu.py:
each helper against one the suite already trusts."""
import numpy as np
import pytest

import _pa_rows as pr
from oracle.oracle import quantize_rows_np, unpack_a_f16, unpack_a_i8


def test_pack_a_inverts_the_oracle_unpack():
    rng = np.random.default_rng(1)
    for rows, K in ((1, 64), (16, 128), (37, 192), (130, 384)):
        a = rng.integers(-128, 128, (rows, K)).astype(np.int8)
        np.testing.assert_array_equal(unpack_a_i8(pr.pack_a(a, 0), rows, K), a)
        h = rng.integers(0, 1 << 16, (rows, K)).astype(np.uint16)
        np.testing.assert_array_equal(unpack_a_f16(pr.pack_a(h, 0), rows, K).view(np.uint16), h)


def test_rows_ref_and_quantiser_against_the_oracle(oracle):
    """rows_ref reshapes heads to rows in the o_proj's k order (h * D + d) and
    scales in float64; its rows through quantize_rows_np equal
    oracle.quantize_rows, the reference check_conversions is given."""
    rng = np.random.default_rng(2)
    heads = rng.standard_normal((5, 3, 32)).astype(np.float32)
    rows = pr.rows_ref(heads, 0.37)
    assert rows.dtype == np.float64 and rows.shape == (5, 96)
    assert rows[2, 1 * 32 + 7] == np.float64(heads[2, 1, 7]) * 0.37
    x = rows.astype(np.float32)
    x[4] = 0.0  # an empty context's row
    q, s = oracle.quantize_rows(x)
    qn, sn = quantize_rows_np(x)
    np.testing.assert_array_equal(q, qn)
    np.testing.assert_array_equal(s.view(np.uint32), sn.view(np.uint32))


@pytest.mark.parametrize("pack", [0, 1])
def test_check_conversions_accepts_exact_and_rejects_one_bit(oracle, pack):
    rng = np.random.default_rng(3)
    rows, hid = 21, 128
    out = rng.standard_normal((rows, hid)).astype(np.float32)
    q, s = oracle.quantize_rows(out)
    h = out.astype(np.float16).view(np.uint16)
    fill16 = np.uint16(pr.SENTINEL * 0x0101)
    q8 = pr.pack_a(q, pr.SENTINEL) if pack else q.ravel().copy()
    o16 = (pr.pack_a(h, fill16) if pack else h.ravel().copy()).view(np.int16)
    pr.check_conversions(oracle.quantize_rows, out, q8=q8, inv_scale=s, out16=o16, pack=pack)
    one = q8.copy()
    one[5] ^= 1
    with pytest.raises(AssertionError):
        pr.check_conversions(oracle.quantize_rows, out, q8=one, inv_scale=s, pack=pack)
    with pytest.raises(AssertionError):
        pr.check_conversions(oracle.quantize_rows, out, q8=q8, pack=pack,
                             inv_scale=np.nextafter(s, np.float32(1)))
    one = o16.copy()
    one[7] ^= 1
    with pytest.raises(AssertionError):
        pr.check_conversions(oracle.quantize_rows, out, out16=one, pack=pack)
    if pack:  # a padding row written: rows 21 .. 31 of the second 16-row tile
        full = np.full((pr.pad16(rows), hid), pr.SENTINEL, np.int8)
        full[:rows] = q
        full[rows + 2, 9] = 0
        with pytest.raises(AssertionError, match="padding"):
            pr.check_conversions(oracle.quantize_rows, out, q8=pr.pack_a(full, 0), inv_scale=s,
                                 pack=1)


def test_pools_hold_the_values_they_report():
    rng = np.random.default_rng(4)
    pt, num_pages, unused = pr.page_table(rng, 8, 2, 100, 16, shared_groups=True)
    assert pt.shape == (8, 2, 9) and (pt[:, :, 7:] == -1).all() and len(unused) >= 5
    assert (pt[1:4, :, :3] == pt[0, :, :3]).all() and (pt[1, :, 3:7] != pt[0, :, 3:7]).all()
    for kv in ("f16", "bf16", "i8"):
        host, f32 = pr.pool_values(rng, kv, (num_pages, 16, 32), 0.5, unused)
        back = host.float().numpy() if kv == "bf16" else np.asarray(host).astype(np.float32)
        np.testing.assert_array_equal(back, f32)
        assert np.abs(f32[unused]).mean() > 5 * np.abs(np.delete(f32, unused, axis=0)).mean()
