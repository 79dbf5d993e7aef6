"""tools/attention_window_timing.py without a GPU: the row format, the routing rule and the sanity gate on canned rows - a head size
is routed to the windowed entry up to the longest measured length at which it was at least as fast as torch's attention with the
window mask, with padding and without, there and at every shorter measured one - and the recorded rows
(profiles/attention_window_timing.jsonl) against fused_forward's tables and the gate: from 1,024 tokens on the windowed entry is
faster than its unwindowed parent by more than the spread between the alternating rounds."""
import importlib.util
import json
import os

import pytest

from conftest import ROOT
from theoremsearch_amd import fused_forward as ff


def tool():
    spec = importlib.util.spec_from_file_location("attention_window_timing", os.path.join(ROOT, "tools", "attention_window_timing.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def row(dtype, tokens, window, torch_, parent=None, window_nomask=None, torch_nomask=None, spread=1.0):
    parent = 2.0 * window if parent is None else parent
    us = {"window_us": window, "parent_us": parent, "torch_us": torch_, "window_nomask_us": window if window_nomask is None else window_nomask,
          "parent_nomask_us": parent, "torch_nomask_us": torch_ if torch_nomask is None else torch_nomask, "mask_fill_us": 1.0}
    return {"pair": "window vs parent vs torch", "dtype": dtype, "head_dim": 256, "batch": 256, "tokens": tokens, "window": 257, "heads": "3/1 x 256",
            "max_abs_diff": 0.0, **us, "spread_us": {k: spread for k in us}, "rounds": 5, "calls": 30, "chunks_walked": 1, "chunks_total": 2}


def test_the_routing_rule_and_the_gate_on_canned_rows():
    t = tool()
    # wins up to 384, loses at 512, wins again at 1,024: the later win does not count
    rows = [row("bf16", 1024, 90.0, 100.0), row("bf16", 258, 10.0, 11.0), row("bf16", 512, 51.0, 50.0), row("bf16", 384, 20.0, 20.0)]
    assert t.routed_max_seq(rows, "bf16") == 384
    assert t.routed_max_seq(rows, "fp32") == 0 and t.routed_max_seq(rows, "bf16", 128) == 0          # nothing measured: not routed
    assert t.routed_max_seq([row("fp32", 258, 2.0, 1.0), row("fp32", 384, 1.0, 2.0)], "fp32") == 0    # loses at the shortest: wins nowhere
    # one table: a length counts only if the entry is at least as fast with padding AND without
    assert not t.at_least_as_fast(row("bf16", 258, 1.0, 2.0, window_nomask=3.0, torch_nomask=2.0))
    assert t.at_least_as_fast(row("bf16", 258, 2.0, 2.0))
    # the gate: against the parent, by more than the spread
    assert t.faster_than_parent(row("bf16", 1024, 10.0, 50.0, parent=20.0, spread=5.0))
    assert not t.faster_than_parent(row("bf16", 1024, 10.0, 50.0, parent=12.0, spread=5.0))
    assert not t.faster_than_parent(row("bf16", 1024, 10.0, 50.0, parent=10.0, spread=0.0))


def test_the_row_format_and_the_chunk_counts(tmp_path):
    t = tool()
    path = tmp_path / "rows.jsonl"
    path.write_text(json.dumps(row("bf16", 258, 1.0, 2.0)) + "\n\n" + json.dumps(row("fp32", 384, 1.0, 2.0)) + "\n")
    rows = t.read_rows(str(path))
    assert [r["tokens"] for r in rows] == [258, 384] and all(set(t.ROW_KEYS) <= set(r) for r in rows)
    bad = row("bf16", 258, 1.0, 2.0)
    del bad["parent_us"]
    path.write_text(json.dumps(bad) + "\n")
    with pytest.raises(AssertionError, match="parent_us"):
        t.read_rows(str(path))
    assert t.batch_of(512) == 256 and t.batch_of(1024) == 64 and t.LENGTHS == (258, 384, 512, 1024, 2048)
    assert (t.HQ, t.HKV, t.HD, t.WINDOW, t.CHUNK) == (3, 1, 256, 257, ff._BF16_TILED_CHUNK[256])
    # 258 tokens: every chunk; 2,048 tokens: 18 of 64 chunks per block away from the ends, fewer at them
    assert t.chunks_walked(258) == (45, 45) and t.chunks_walked(2048) == (536, 2048)


def test_the_routing_tables_and_the_gate_follow_from_the_recorded_rows():
    t = tool()
    rows = t.read_rows(os.path.join(ROOT, "profiles", "attention_window_timing.jsonl"))
    for dtype, table in (("bf16", ff._WINDOW_ROUTED_MAX_SEQ_BF16), ("fp32", ff._WINDOW_ROUTED_MAX_SEQ_F32)):
        mine = [r for r in rows if r["dtype"] == dtype]
        assert tuple(r["tokens"] for r in sorted(mine, key=lambda r: r["tokens"])) == t.LENGTHS, dtype
        assert all(r["batch"] == t.batch_of(r["tokens"]) and r["head_dim"] == 256 and r["window"] == 257 and r["rounds"] >= 5 for r in mine)
        assert set(table) == {256} and table[256] == t.routed_max_seq(rows, dtype), (dtype, t.routed_max_seq(rows, dtype))
        assert table[256] <= (ff._BF16_TILED_MAX_SEQ if dtype == "bf16" else ff._TILED_MAX_SEQ)
        for r in mine:
            assert (r["chunks_walked"], r["chunks_total"]) == t.chunks_walked(r["tokens"])
            if r["tokens"] >= 1024:
                assert t.faster_than_parent(r), (dtype, r["tokens"], "the windowed entry is not clearly faster than its parent: chunks are not skipped")
