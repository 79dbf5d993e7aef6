"""tools/attention_ab.py, the byte-for-byte A/B of the attention entry points of two builds, without a GPU: --compare on archives
written here (equal; one bit, one key, one shape apart) and what the case list of --dump reaches."""
import importlib.util
import io
from pathlib import Path

import numpy as np

_spec = importlib.util.spec_from_file_location("attention_ab", Path(__file__).resolve().parents[1] / "tools" / "attention_ab.py")
ab = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ab)


def _archive(path, **changes):
    rng = np.random.default_rng(7)
    arrays = {"entry=ts_attention_short/S=17/out": rng.integers(0, 1 << 16, (3, 17, 192), dtype=np.uint16),
              "entry=ts_attention_float/S=17/out": rng.integers(0, 1 << 32, (2, 17, 384), dtype=np.uint32),
              "entry=ts_attention_float/S=17/pieces": rng.integers(0, 1 << 16, (34, 1152), dtype=np.uint16)}
    for k, v in changes.items():
        if v is None:
            del arrays[k]
        else:
            arrays[k] = v(arrays[k])
    np.savez(path, **arrays)
    return str(path)


def _compare(a, b):
    out = io.StringIO()
    return ab.compare(a, b, out=out), out.getvalue()


def test_compare_passes_on_equal_archives(tmp_path):
    n, report = _compare(_archive(tmp_path / "a.npz"), _archive(tmp_path / "b.npz"))
    assert n == 0, report
    assert "3 arrays" in report and "0 differ" in report


def test_compare_fails_on_one_bit_a_missing_key_and_a_shape(tmp_path):
    a = _archive(tmp_path / "a.npz")
    key = "entry=ts_attention_float/S=17/out"

    def flip(x):
        y = x.copy()
        y[1, 16, 383] ^= np.uint32(1)                       # the lowest bit of the last element
        return y

    n, report = _compare(a, _archive(tmp_path / "bit.npz", **{key: flip}))
    assert n == 1 and key + ": 1 of" in report, report
    n, report = _compare(a, _archive(tmp_path / "key.npz", **{key: None}))
    assert n == 1 and key + ": only in" in report, report
    n, report = _compare(_archive(tmp_path / "key2.npz", **{key: None}), a)      # ... whichever side misses it
    assert n == 1 and key + ": only in" in report, report
    n, report = _compare(a, _archive(tmp_path / "shape.npz", **{key: lambda x: x.reshape(2 * 17, 384)}))
    assert n == 1 and key + ": uint32 (2, 17, 384) against uint32 (34, 384)" in report, report
    # the same bytes under another element type are not the same array either
    n, report = _compare(a, _archive(tmp_path / "dtype.npz", **{key: lambda x: x.view(np.int32)}))
    assert n == 1, report


def test_case_list_reaches_every_instantiation():
    cases = ab.cases()
    keys = [ab.case_key(c) for c in cases]
    assert len(set(keys)) == len(keys)
    for entry, hd in (("ts_attention_short", 64), ("ts_attention_gqa", 128)):
        mine = [c for c in cases if c["entry"] == entry]
        assert {c["hd"] for c in mine} == {hd}
        assert {(c["S"] + 15) // 16 for c in mine} == set(range(1, 9))                       # every T of both kernel forms
        for t in range(1, 9):
            assert {c["S"] for c in mine if (c["S"] + 15) // 16 == t} == {16 * t - 15, 16 * t - 1, 16 * t}
        assert {c["mask"] for c in mine} == set(ab.MASKS) == {"none", "tail", "keyless"}
    gqa = [c for c in cases if c["entry"] == "ts_attention_gqa"]
    for t in range(1, 9):
        combos = {(ab.gqa_rows_r(c["hq"], c["hkv"]), c["causal"]) for c in gqa if (c["S"] + 15) // 16 == t}
        assert combos == {(r, causal) for r in (1, 2, 4) for causal in (0, 1)}
    assert min(c["S"] for c in cases) == 1
    for entry in ("ts_attention_float", "ts_attention_tiled"):
        mine = [c for c in cases if c["entry"] == entry]
        assert {(c["hd"], c["causal"], c["bias"], c["want_out"], c["mask"]) for c in mine} == {
            (hd, causal, bias, want, mask) for hd in (64, 128, 256) for causal in (0, 1) for bias in (0, 1) for want in (0, 1) for mask in ab.MASKS}
        for hd in (64, 128, 256):
            chunk = ab.TILED_CHUNK[hd]
            want = {1, 15, 16, 17, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 1, 4 * chunk + 17}
            if entry == "ts_attention_float":
                want = {s for s in want if s <= ab.F32_MAX_SEQ[hd]}
            assert {c["S"] for c in mine if c["hd"] == hd} == want
    # the tool's copies of the plan's constants are the forwards' own
    from theoremsearch_amd import fused_forward as ff
    assert ab.F32_MAX_SEQ == ff._FLOAT_ATTENTION_MAX_SEQ and ab.TILED_CHUNK == ff._TILED_CHUNK


def test_judge_passes_up_to_the_parents_median_plus_its_spread(tmp_path):
    import json

    def runs(side, rows):                                   # rows: name -> the three runs' us per call
        paths = []
        for i in range(3):
            p = tmp_path / ("%s_%d.json" % (side, i))
            p.write_text(json.dumps({"rows": {k: {"us_per_call": v[i]} for k, v in rows.items()}}))
            paths.append(str(p))
        return paths

    # parent: median 100, spread 104 - 98 = 6 -> allowed 106 (binary fractions: the limit is exact)
    parent = runs("parent", {"faster": (98.0, 100.0, 104.0), "at the limit": (98.0, 100.0, 104.0), "slower": (98.0, 100.0, 104.0),
                             "one slow run": (98.0, 100.0, 104.0)})
    new = runs("new", {"faster": (90.0, 99.0, 120.0), "at the limit": (106.0, 100.0, 110.0), "slower": (106.25, 106.5, 100.0),
                       "one slow run": (100.0, 500.0, 101.0)})                  # the median of three, not the worst, is judged
    out = io.StringIO()
    assert ab.judge(parent, new, out=out) == 1
    verdict = {ln[:32].strip(): ln.split()[-1] for ln in out.getvalue().splitlines()[1:-1]}
    assert verdict == {"faster": "pass", "at the limit": "pass", "slower": "FAIL", "one slow run": "pass"}
    assert "4 rows, 1 slower than the parent's median + spread" in out.getvalue()
    assert ab.judge(parent, parent, out=io.StringIO()) == 0


def test_masks_are_none_a_padded_tail_and_a_keyless_sequence():
    assert ab.key_mask("none", 3, 17) is None
    tail = ab.key_mask("tail", 3, 17)
    assert tail.sum(1).tolist() == [16, 13, 10] and bool((tail[:, :10] == 1).all())
    assert ab.key_mask("tail", 3, 1).sum(1).tolist() == [1, 1, 1]
    keyless = ab.key_mask("keyless", 3, 17)
    assert keyless.sum(1).tolist() == [16, 0, 10]
