"""The attention launch planner (csrc/pa_plan.hpp) against recorded plans.

tests/golden/pa_plan_grid.txt holds the return code, split count and form that
the code before the planner was split out gave, in plan-only mode, for an even
thinning (every 211th point) of B {1, 3, 4, 8, 16, 64} x H {1, 12, 16, 32} x
D {32, 64, 128, 256} x page {16, 32} x T {1, 16, 17, 2048, 8192, 16384 page}
x the five KV types x pages_per_split {0, 8, 128} x row_group {1, 4} x every
output kind, with the resident-wave counts it falls back to without a device
(3072 for the split kernel, 0 for the beam form).  pa_plan_device.txt holds the
same for the decoder's own launches (bench.py's C2 .. C5 shapes, fp16 and fp8
pools, both row groups, every kind) with the counts an MI355X reports.

The row kinds are not reachable through the product ABI: the tuning library's
pa_plan_tune takes the request fields and the resident counts (< 0: query the
device; 0 is a count: the beam form's where the plain schedule runs).  Every
row must match exactly.
"""
import ctypes
from pathlib import Path

import pytest

try:
    import llm_capi
except ImportError:  # run as a script (test_planner_replays_device_plans' child)
    import sys
    sys.path.insert(0, str(next(Path(__file__).resolve().parents[1].glob("*_amd"))))
    import llm_capi

GOLDEN = Path(__file__).resolve().parent / "golden"
# kind -> (PaOut value, rows16)
KINDS = {"f32": (0, 0), "row_q": (1, 0), "row_f16": (2, 0), "f32_rows": (3, 0), "oproj": (4, 0),
         "oproj16": (4, 1)}
CPU_RESIDENT, CPU_BEAM_RESIDENT = 3072, 0


def _rows(name):
    rows = []
    for line in (GOLDEN / name).read_text().splitlines():
        if line.startswith("#"):
            continue
        f = line.split()
        rows.append((tuple(int(x) for x in f[:8]), f[8], tuple(int(x) for x in f[9:12])))
    return rows


def _plan_tune(tune, shape, kind, resident, beam_resident):
    B, H, D, page, T, kvt, pps, rg = shape
    out, rows16 = KINDS[kind]
    ns, form = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = tune.pa_plan_tune(B, H, D, T, page, (T + page - 1) // page, kvt, pps, rg, out, rows16,
                           resident, beam_resident, 0, ctypes.byref(ns), ctypes.byref(form))
    return rc, ns.value, form.value


def _plan_product(lib, shape):
    B, H, D, page, T, kvt, pps, rg = shape
    view = llm_capi.PaKvView(k_pool=1, v_pool=1, page_table=1, num_pages=1 << 20, page_size=page,
                             head_dim=D, num_beams=B, num_heads=H,
                             max_tiles=(T + page - 1) // page, kv_dtype=kvt)
    ns, form = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = lib.pa_decode_plan(ctypes.byref(view), B, H, D, T, pps, rg, ctypes.byref(ns),
                            ctypes.byref(form))
    return rc, ns.value, form.value


def test_grid_is_whole():
    rows = _rows("pa_plan_grid.txt")
    assert len(rows) == 983
    assert {k for _, k, _ in rows} == set(KINDS)
    assert {s[5] for s, _, _ in rows} == {0, 1, 2, 3, 4}
    assert {s[6] for s, _, _ in rows} == {0, 8, 128} and {s[7] for s, _, _ in rows} == {1, 4}


def test_planner_replays_recorded_plans():
    tune = llm_capi.load_tune()
    bad = []
    for shape, kind, want in _rows("pa_plan_grid.txt"):
        got = _plan_tune(tune, shape, kind, CPU_RESIDENT, CPU_BEAM_RESIDENT)
        if got != want:
            bad.append((shape, kind, want, got))
    assert not bad, f"{len(bad)} rows differ, first: {bad[:5]}"


def test_product_plan_matches_recorded_plans():
    """pa_decode_plan (fp32 output) against the table's fp32 rows.  With a
    device the product library plans with that device's counts, so there the
    rows that read no count (fixed pages_per_split, refused requests) are
    compared; the others are test_planner_replays_device_plans' business."""
    import torch
    lib = llm_capi.load()
    no_device = not torch.cuda.is_available()
    n = 0
    for shape, kind, want in _rows("pa_plan_grid.txt"):
        if kind == "f32" and (no_device or shape[6] > 0 or want[0] != 0):
            n += 1
            assert _plan_product(lib, shape) == want, shape
    assert n == (164 if no_device else 114)


def _replay_device_plans():
    """Mismatches of the device table: every row through the tuning library's
    planner with queried counts, the fp32 rows through pa_decode_plan too."""
    lib, tune = llm_capi.load(), llm_capi.load_tune()
    rows = _rows("pa_plan_device.txt")
    bad = [] if len(rows) == 144 else [("rows", len(rows))]
    for shape, kind, want in rows:
        got = _plan_tune(tune, shape, kind, -1, -1)
        if got != want:
            bad.append(("tuning", shape, kind, want, got))
        if kind == "f32" and _plan_product(lib, shape) != want:
            bad.append(("product", shape, kind, want, _plan_product(lib, shape)))
    return bad


@pytest.mark.gpu
def test_planner_replays_device_plans():
    """Launches nothing.  In a process of its own: the tuning library caches a
    kernel's occupancy the first time it is asked, under whatever switches
    (LLM_BEAM_MFMA) another test of this process had set at that moment."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, __file__], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


if __name__ == "__main__":
    import sys
    bad = _replay_device_plans()
    for b in bad[:10]:
        print(b)
    print(f"{len(bad)} rows differ")
    sys.exit(1 if bad else 0)
