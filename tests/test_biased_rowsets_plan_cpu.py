"""The host decisions of ts_search_biased_rowsets (theoremsearch_amd/csrc/biased_rowsets_plan.h: the validation of the entry's
arguments, the classes (set, weight) and the delegation, the partition of a mixed batch into the shared pass and the per-class
groups, the TS_ALGO_MFMA refusal, the blocks of 256, the histograms a pass needs and their cost formula) and the weight mapping
of its threshold estimate (one histogram of the raw bias read through each query's weight, and the solver on it) are plain
arithmetic in a header that needs no HIP.  tests/biased_rowsets_plan_check.cpp checks them in a program of its own, built with
the host compiler under the address and undefined-behaviour sanitizers and run as a child process; nothing of it is loaded into
Python."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_biased_rowsets_plan_header_checks_pass_under_the_host_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "biased_rowsets_plan_check"
    # the sanitizers' runtimes linked into the program (clang's default): it starts whatever else the loader brings in
    static_rt = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         *static_rt, "-I", os.path.join(ROOT, "theoremsearch_amd", "csrc"), os.path.join(ROOT, "tests", "biased_rowsets_plan_check.cpp"),
         "-o", str(exe)],
        capture_output=True, text=True, timeout=280)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout
