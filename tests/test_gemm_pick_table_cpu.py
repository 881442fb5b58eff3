"""The GEMM route decision is pinned: tests/golden/gemm_pick_table.json lists descriptors (scalar fields, pointers as set / null) with the
`ud_gemm_pick` value and the kernel class label `ud_gemm_kernel_name` gives them (tools/gemm_pick_table.py).  Both are host code: nothing
runs on a device.  A change that is meant to leave the dispatch alone must pass with the golden file untouched; one that changes the
decision on purpose regenerates it (`python tools/gemm_pick_table.py --write`) and shows the row diff."""
import ctypes as C
import importlib.util
import json
import os

import pytest
import torch

_spec = importlib.util.spec_from_file_location("gemm_pick_table", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                                                                               "gemm_pick_table.py"))
gpt = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gpt)


@pytest.fixture(scope="module")
def rows():
    with open(gpt.GOLDEN) as f:
        return list(gpt.table_rows(json.load(f)))


def test_library_answers_every_row_as_pinned(rows):
    from unidepth_amd import _lib
    bad = []
    for row, pick, label in rows:
        got = gpt.answer(_lib.lib, gpt.desc(row))
        if got != (pick, label):
            bad.append((row, (pick, label), got))
    assert not bad, (len(bad), bad[:5])


def test_table_covers_the_decision(rows):
    """The table cannot quietly shrink: every schedule, hint, epilogue, A mode and flag field stays in it."""
    assert 2000 <= len(rows) and os.path.getsize(gpt.GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(gpt.GOLDEN), "plan_fingerprints.json"))
    assert len({gpt.key(r) for r, _, _ in rows}) == len(rows)
    assert {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 19, 20, 24, 36} <= {p for _, p, _ in rows}
    assert {r.get("tile_hint", 0) for r, _, _ in rows} >= set(range(16))
    assert {r.get("epi", 0) for r, _, _ in rows} == set(range(5))
    assert {r.get("amode", 0) for r, _, _ in rows} == set(range(4))
    for field in ("groups", "row_stats_in", "row_stats_out", "row_stats_final", "max_out", "a_wrap", "w_wrap", "accumulate", "splitk_ws", "splitk_ws_bytes"):
        assert {bool(r.get(field, 0)) for r, _, _ in rows} == {False, True}, field
    assert any(r.get("splitk_ws") and not r.get("splitk_ws_bytes") for r, _, _ in rows)          # the small split-K scratch alone
    # the pick-12 schedule (two workgroups per CU) carries its own kernel's name
    assert {label for _, p, label in rows if p == 12} == {"gemm_pp_f32_kernel<3, 4>"}


def test_table_holds_every_gemm_of_the_dry_run_plans(rows):
    if torch.cuda.is_available():
        pytest.skip("host-only dry run")
    have = {gpt.key(r) for r, _, _ in rows}
    recorded = gpt.plan_rows()
    assert len(recorded) > 3 * 60
    missing = [r for r in recorded if gpt.key(r) not in have]
    assert not missing, (len(missing), missing[:3])


def test_kernel_name_reports_a_short_buffer():
    from unidepth_amd import _lib
    d = gpt.desc(dict(M=4096, N=1024, K=1024))
    buf = C.create_string_buffer(8)
    assert _lib.lib.ud_gemm_kernel_name(C.byref(d), buf, len(buf)) == -1
    assert _lib.lib.ud_gemm_kernel_name(C.byref(d), None, 0) == -1
