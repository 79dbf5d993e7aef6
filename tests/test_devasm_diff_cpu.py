"""tools/devasm_diff.py, the per-symbol comparison of two `make devasm` directories, on tiny listings written here: nothing is
compiled.  Identical code up to label numbers and the per-build __hip_cuid_ symbol gives 0 differences; a changed instruction,
a changed kernel-descriptor value and a symbol present on one side only are each reported with their symbol."""
import importlib.util
import io
from pathlib import Path

_spec = importlib.util.spec_from_file_location("devasm_diff", Path(__file__).resolve().parents[1] / "tools" / "devasm_diff.py")
devasm_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(devasm_diff)


def _kernel(sym, fn, body, vgprs=12, cuid="abc123"):
    """One kernel the way hipcc -S prints it; `fn` numbers its local labels."""
    return f"""\t.text
\t.globl\t{sym}
\t.p2align\t8
\t.type\t{sym},@function
{sym}:                                   ; @{sym}
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_cbranch_scc1 .LBB{fn}_2
.LBB{fn}_1:                               ; =>This Inner Loop Header: Depth=1
{body}
\ts_cbranch_scc0 .LBB{fn}_1
.LBB{fn}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {sym}
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgprs}
\t\t.amdhsa_next_free_sgpr 16
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{fn}:
\t.size\t{sym}, .Lfunc_end{fn}-{sym}
\t.type\t__hip_cuid_{cuid},@object
\t.globl\t__hip_cuid_{cuid}
__hip_cuid_{cuid}:
\t.byte\t0
"""


def _compare(tmp_path, a_units, b_units):
    for side, units in (("a", a_units), ("b", b_units)):
        (tmp_path / side).mkdir()
        for name, text in units.items():
            (tmp_path / side / name).write_text(text)
    out = io.StringIO()
    n = devasm_diff.compare_dirs(tmp_path / "a", tmp_path / "b", out=out)
    return n, out.getvalue()


BODY = "\tv_add_f32_e32 v1, v0, v0\n\ts_add_i32 s2, s2, 1  ; a comment"


def test_same_code_up_to_labels_and_cuid(tmp_path):
    a = _kernel("kern_a", 0, BODY, cuid="111") + _kernel("kern_b", 1, BODY, cuid="111")
    b = _kernel("kern_b", 0, BODY, cuid="222") + _kernel("kern_a", 1, BODY, cuid="222")      # other order, other label numbers
    n, report = _compare(tmp_path, {"u.s": a}, {"u.s": b})
    assert n == 0, report
    assert "1 units, 2 functions, 2 descriptors compared: 0 differences" in report


def test_changed_instruction_is_reported_with_its_symbol(tmp_path):
    a = _kernel("kern_a", 0, BODY) + _kernel("kern_b", 1, BODY)
    b = _kernel("kern_a", 0, BODY) + _kernel("kern_b", 1, BODY.replace("v_add_f32_e32 v1, v0, v0", "v_add_f32_e32 v1, v0, v2"))
    n, report = _compare(tmp_path, {"u.s": a}, {"u.s": b})
    assert n == 1, report
    assert "u.s: function kern_b: instructions differ" in report and "kern_a" not in report
    assert "+v_add_f32_e32 v1, v0, v2" in report


def test_changed_descriptor_value_is_reported(tmp_path):
    n, report = _compare(tmp_path, {"u.s": _kernel("kern_a", 0, BODY, vgprs=12)}, {"u.s": _kernel("kern_a", 0, BODY, vgprs=13)})
    assert n == 1, report
    assert "u.s: descriptor kern_a: .amdhsa_next_free_vgpr 12 -> 13" in report


def _summary(tmp_path, a_units, b_units):
    for side, units in (("a", a_units), ("b", b_units)):
        (tmp_path / side).mkdir()
        for name, text in units.items():
            (tmp_path / side / name).write_text(text)
    out = io.StringIO()
    n = devasm_diff.compare_dirs(tmp_path / "a", tmp_path / "b", out=out, summary=True)
    return n, out.getvalue()


MEM_BODY = "\tds_read_b128 v[4:7], v2\n\tv_mfma_f32_16x16x4_f32 v[8:11], v4, v5, v[8:11]\n\tglobal_store_dwordx4 v3, v[8:11], s[0:1]\n\ts_barrier"


def test_summary_accepts_a_moved_kernel_that_keeps_its_static_figures(tmp_path):
    a = _kernel("kern_a", 0, MEM_BODY, vgprs=60) + _kernel("kern_b", 1, BODY)
    b = _kernel("kern_a", 0, MEM_BODY.replace("v[4:7], v2", "v[12:15], v1"), vgprs=64) + _kernel("kern_b", 1, BODY)
    n, report = _summary(tmp_path, {"u.s": a}, {"u.s": b})
    assert n == 0, report
    assert "u.s: kern_a: moved, static gate holds" in report and "kern_b" not in report
    assert "1 kernels moved, 0 one-sided or failing" in report
    row = {ln.split()[0]: ln.split()[1:3] for ln in report.splitlines() if ln.startswith("    ") and len(ln.split()) >= 3}
    assert row["next_free_vgpr"] == ["60", "64"] and row["waves_per_simd"] == ["8", "8"]
    assert row["v_mfma"] == ["1", "1"] and row["ds_read"] == ["1", "1"] and row["global_store"] == ["1", "1"] and row["s_barrier"] == ["1", "1"]
    assert row["group_segment_fixed_size"] == ["0", "0"]


def test_summary_fails_on_a_count_lds_or_occupancy_change(tmp_path):
    a = _kernel("kern_a", 0, MEM_BODY, vgprs=64) + _kernel("kern_b", 1, MEM_BODY, vgprs=64) + _kernel("kern_c", 2, MEM_BODY)
    b = (_kernel("kern_a", 0, MEM_BODY + "\n\tds_read_b128 v[4:7], v2", vgprs=64) + _kernel("kern_b", 1, MEM_BODY, vgprs=72)
         + _kernel("kern_c", 2, MEM_BODY).replace("group_segment_fixed_size 0", "group_segment_fixed_size 1024"))
    n, report = _summary(tmp_path, {"u.s": a}, {"u.s": b})
    assert n == 3, report
    assert "u.s: kern_a: STATIC GATE FAILS: ds_read" in report
    assert "u.s: kern_b: STATIC GATE FAILS: waves_per_simd" in report                 # 512 // 64 = 8 -> 512 // 72 = 7
    assert "u.s: kern_c: STATIC GATE FAILS: group_segment_fixed_size" in report
    assert devasm_diff.waves_per_simd(128) == 4 and devasm_diff.waves_per_simd(129) == 3 and devasm_diff.waves_per_simd(512) == 1


def test_symbol_or_unit_on_one_side_only_is_reported(tmp_path):
    a = {"u.s": _kernel("kern_a", 0, BODY) + _kernel("kern_b", 1, BODY), "only_a.s": _kernel("kern_c", 0, BODY)}
    b = {"u.s": _kernel("kern_a", 0, BODY)}
    n, report = _compare(tmp_path, a, b)
    assert n == 3, report                       # the function, its descriptor, the unit
    assert "u.s: function kern_b: only in" in report and "u.s: descriptor kern_b: only in" in report
    assert "unit only_a.s: only in" in report
