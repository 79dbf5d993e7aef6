"""tools/attention_bf16_timing.py without a GPU: the row format, and the routing rule on canned rows - a head size is routed up to
the longest measured length at which the new entry was at least as fast there and at every shorter measured one, separately for
batches with and without padding - and the recorded rows (profiles/attention_bf16_timing.jsonl) against fused_forward's tables."""
import importlib.util
import json
import os

import pytest

from conftest import ROOT
from theoremsearch_amd import fused_forward as ff


def tool():
    spec = importlib.util.spec_from_file_location("attention_bf16_timing", os.path.join(ROOT, "tools", "attention_bf16_timing.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def row(hd, tokens, ts, before, ts_nomask=None, before_nomask=None):
    return {"pair": "flash vs torch", "family": "x", "head_dim": hd, "batch": 256, "tokens": tokens, "heads": f"1/1 x {hd}", "causal": False,
            "max_abs_diff": 0.0, "ts_us": ts, "before_us": before, "ts_nomask_us": ts if ts_nomask is None else ts_nomask,
            "before_nomask_us": before if before_nomask is None else before_nomask, "mask_fill_us": 1.0, "spread_us": {}, "rounds": 5}


def test_the_routing_rule_on_canned_rows():
    t = tool()
    # wins up to 256, loses at 384, wins again at 512: the later win does not count
    rows = [row(64, 512, 90.0, 100.0), row(64, 192, 10.0, 11.0), row(64, 384, 51.0, 50.0), row(64, 256, 20.0, 20.0)]
    assert t.routed_max_seq(rows, 64) == 256
    assert t.routed_max_seq(rows, 128) == 0                                          # nothing measured: not routed
    assert t.routed_max_seq([row(256, 32, 2.0, 1.0), row(256, 64, 1.0, 2.0)], 256) == 0     # loses at the shortest: wins nowhere
    assert t.routed_max_seq([row(128, 129, 1.0, 1.0), row(128, 2048, 5.0, 9.0)], 128) == 2048
    # with and without padding are ruled separately
    both = [row(256, 32, 1.0, 9.0, 1.0, 2.0), row(256, 64, 2.0, 9.0, 3.0, 2.0), row(256, 128, 3.0, 9.0, 1.0, 2.0)]
    assert t.routed_max_seq(both, 256, padding=True) == 128 and t.routed_max_seq(both, 256, padding=False) == 32
    assert t.at_least_as_fast(both[1], True) and not t.at_least_as_fast(both[1], False)
    # the other rows of a file do not disturb a head size's rule
    assert t.routed_max_seq(rows + both, 64) == 256 and t.routed_max_seq(rows + both, 256) == 128


def test_the_row_format(tmp_path):
    t = tool()
    path = tmp_path / "rows.jsonl"
    path.write_text(json.dumps(row(64, 192, 1.0, 2.0)) + "\n\n" + json.dumps(row(64, 256, 1.0, 2.0)) + "\n")
    rows = t.read_rows(str(path))
    assert [r["tokens"] for r in rows] == [192, 256] and all(set(t.ROW_KEYS) <= set(r) for r in rows)
    bad = row(64, 192, 1.0, 2.0)
    del bad["before_us"]
    path.write_text(json.dumps(bad) + "\n")
    with pytest.raises(AssertionError, match="before_us"):
        t.read_rows(str(path))
    assert t.batch_of(512) == 256 and t.batch_of(1024) == 64 and t.batch_of(2048) == 64
    assert t.LENGTHS == {"bert": (192, 256, 384, 512), "qwen3": (129, 192, 256, 384, 512, 1024, 2048), "gemma3": (32, 64, 128, 192, 256, 384, 512)}
    assert {name: f[2] for name, f in t.FAMILIES.items()} == {"bert": 64, "qwen3": 128, "gemma3": 256}


def test_the_routing_tables_follow_from_the_recorded_rows():
    t = tool()
    rows = t.read_rows(os.path.join(ROOT, "profiles", "attention_bf16_timing.jsonl"))
    for name, (_, _, hd, causal, _) in t.FAMILIES.items():
        mine = [r for r in rows if r["head_dim"] == hd]
        assert tuple(sorted(r["tokens"] for r in mine)) == t.LENGTHS[name], name
        assert all(r["batch"] == t.batch_of(r["tokens"]) and r["causal"] == causal and r["rounds"] >= 5 for r in mine)
        assert ff._BF16_TILED_ROUTED_MAX_SEQ[hd] == t.routed_max_seq(rows, hd, True), (name, t.routed_max_seq(rows, hd, True))
        # without padding heads of 256 win at 32 tokens in these rows (18.4 against 21.2 us) and lost in the encoder-in-loop step (5.83
        # against 5.70 ms, profiles/HISTORY.md Round 24): a table never routes more than the rows allow, and here it routes less
        want = 0 if hd == 256 else t.routed_max_seq(rows, hd, False)
        assert ff._BF16_TILED_ROUTED_MAX_SEQ_NO_PADDING[hd] == want <= t.routed_max_seq(rows, hd, False), (name, t.routed_max_seq(rows, hd, False))
    assert t.routed_max_seq(rows, 256, False) == 32
