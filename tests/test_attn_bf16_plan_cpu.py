"""ts_attention_flash's host decisions without a GPU (theoremsearch_amd/csrc/encoder_plan.h: chunk sizes, LDS, tiles, query blocks,
grid, the refusals, the chunk count of a block) are plain integer arithmetic in a header that needs no HIP.
tests/attn_bf16_plan_check.cpp checks them in a program of its own, built with the host compiler under the address and
undefined-behaviour sanitizers and run as a child process; nothing of it is loaded into Python.  The program prints the chunk sizes
and the token limit; fused_forward's and the tests' mirrors are held against them.  And the helper that picks the bf16 attention
of a forward ("short" / "gqa" / "tiled" / None) at the edges of each kernel's range."""
import os
import shutil
import subprocess

import torch

import attention_bf16_tiled_common as at
from conftest import ROOT
from theoremsearch_amd import fused_forward as ff


def test_bf16_plan_checks_pass_under_the_host_sanitizers_and_the_python_mirrors_match(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "attn_bf16_plan_check"
    # the sanitizers' runtimes linked into the program (clang's default): it starts whatever else the loader brings in
    static_rt = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         *static_rt, "-I", os.path.join(ROOT, "theoremsearch_amd", "csrc"), os.path.join(ROOT, "tests", "attn_bf16_plan_check.cpp"), "-o", str(exe)],
        capture_output=True, text=True, timeout=280)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout
    words = [line.split() for line in run.stdout.splitlines()]
    chunk = {int(w[1]): int(w[2]) for w in words if w and w[0] == "chunk"}
    max_seq = [int(w[1]) for w in words if w and w[0] == "max_seq"]
    assert chunk == ff._BF16_TILED_CHUNK == at.CHUNK and max_seq == [ff._BF16_TILED_MAX_SEQ], (chunk, max_seq)
    assert set(ff._BF16_TILED_CHUNK) == set(ff._BF16_TILED_ROUTED_MAX_SEQ)


def test_the_helper_names_the_kernel_of_every_range(monkeypatch):
    monkeypatch.delenv("TS_ENCODER_ATTENTION", raising=False)
    f32, bf16 = torch.empty(0, dtype=torch.float32), torch.empty(0, dtype=torch.bfloat16)
    kind = ff.bf16_attention_kind
    # where the forwards took ts_attention_short / ts_attention_gqa before, they still do
    for S in (1, 64, 65, 128):
        assert kind(bf16, S, 64, False) == "short" and kind(bf16, S, 128, True) == "gqa"
        assert kind(bf16.new_empty((2, 4)).t(), S, 128, True) is None            # (hidden states that are not contiguous)
        assert kind(bf16, S, 64, True) is None and kind(bf16, S, 128, False) is None
        for hd in (64, 128, 256):
            assert kind(f32, S, hd, False) is None and kind(f32, S, hd, True) is None
    assert ff._BF16_TILED_ROUTED_MAX_SEQ == {64: 256, 128: 2048, 256: 512} and ff._BF16_TILED_ROUTED_MAX_SEQ_NO_PADDING == {64: 0, 128: 384, 256: 0}
    for padding, table in ((True, ff._BF16_TILED_ROUTED_MAX_SEQ), (False, ff._BF16_TILED_ROUTED_MAX_SEQ_NO_PADDING)):
        assert set(table) == set(ff._BF16_TILED_CHUNK)
        for hd, routed in table.items():
            assert 0 <= routed <= ff._BF16_TILED_MAX_SEQ
            floor = 128 if hd in (64, 128) else 0                                   # below 129 tokens heads of 64 / 128 stay where they are
            for causal in (False, True):
                for S in (floor + 1, routed):
                    if floor < S <= routed:
                        assert kind(bf16, S, hd, causal, padding) == "tiled", (hd, S, causal, padding)
                assert kind(bf16, max(routed, floor) + 1, hd, causal, padding) is None
                assert kind(bf16, ff._BF16_TILED_MAX_SEQ + 1, hd, causal, padding) is None
    assert kind(bf16, 200, 256, False) == kind(bf16, 200, 256, False, True) == "tiled"            # (the default: a batch with padding)
    for hd in (32, 96, 512):
        assert kind(bf16, 16, hd, False) is None and kind(bf16, 1000, hd, True) is None
    # TS_ENCODER_FLASH=0: the routing before this entry - short / gqa as ever, torch's attention where "tiled" stood
    monkeypatch.setenv("TS_ENCODER_FLASH", "0")
    assert kind(bf16, 200, 256, False) is None and kind(bf16, 200, 128, True) is None and kind(bf16, 200, 128, True, False) is None
    assert kind(bf16, 128, 64, False) == "short" and kind(bf16, 128, 128, True) == "gqa"
    monkeypatch.delenv("TS_ENCODER_FLASH")
    monkeypatch.setenv("TS_ENCODER_ATTENTION", "0")
    for hd in (64, 128, 256):
        for S in (16, 128, 129, 200):
            assert kind(bf16, S, hd, False) is None and kind(bf16, S, hd, True) is None
