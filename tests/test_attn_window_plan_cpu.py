"""The sliding-window attention's walked ranges without a GPU (attn_window_range, theoremsearch_amd/csrc/encoder_plan.h: plain integer
arithmetic in a header that needs no HIP).  tests/attn_window_plan_check.cpp holds them against brute force - the smallest and largest
key a block's, and a wave's, queries may read - for every S in 1 .. 700, fourteen windows, causal and not, chunks of 32 / 64 / 128
keys, in a program of its own built with the host compiler under the address and undefined-behaviour sanitizers and run as a child
process; nothing of it is loaded into Python.  The program prints one hash of all ranges per (chunk, causal, window);
attention_window_common.window_range, the tests' restatement of the four formulas, must give the same."""
import os
import shutil
import subprocess

import attention_window_common as aw
from conftest import ROOT

WINDOWS = (1, 2, 16, 17, 31, 32, 33, 64, 65, 128, 129, 257, 700, 701)
CHUNKS = (32, 64, 128)
MAX_SEQ = 700


def python_hash(C: int, causal: bool, W: int) -> int:
    h = 0
    for S in range(1, MAX_SEQ + 1):
        T = -(-S // 16)
        for qblk in range(-(-T // 4)):
            for wave in range(4):
                for v in aw.window_range(S, W, causal, C, qblk, wave):
                    h = (h * 1000003 + v) & 0xFFFFFFFFFFFFFFFF
    return h


def test_window_ranges_pass_under_the_host_sanitizers_and_the_python_restatement_matches(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "attn_window_plan_check"
    # the sanitizers' runtimes linked into the program (clang's default): it starts whatever else the loader brings in
    static_rt = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         *static_rt, "-I", os.path.join(ROOT, "theoremsearch_amd", "csrc"), os.path.join(ROOT, "tests", "attn_window_plan_check.cpp"), "-o", str(exe)],
        capture_output=True, text=True, timeout=280)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout
    got = {tuple(int(x) for x in w[1:4]): int(w[4]) for w in (line.split() for line in run.stdout.splitlines()) if w and w[0] == "hash"}
    assert set(got) == {(C, c, W) for C in CHUNKS for c in (0, 1) for W in WINDOWS}
    for (C, causal, W), h in sorted(got.items()):
        assert python_hash(C, bool(causal), W) == h, (C, causal, W)


def test_the_chunks_of_the_issues_example():
    """Head 256 (chunks of 32 keys), W = 257, 2,048 tokens: keys 64 qblk - 256 .. 64 qblk + 319, 576 of them from a multiple of 32 -
    a block walks at most 18 of the 64 chunks."""
    worst = max(aw.window_range(2048, 257, False, 32, qblk, 0)[1] for qblk in range(32))
    assert worst == 18
