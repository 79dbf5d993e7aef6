"""The library's one owner of device memory (theoremsearch_amd/csrc/dev_array.h: keep or re-make, zero a fresh allocation,
re-make a group, borrow, move, free exactly once) is a header that needs no HIP.  tests/dev_array_check.cpp instantiates it
over malloc / free with a counting, failable allocator in a program of its own, built with the host compiler under the
address (and leak) and undefined-behaviour sanitizers and run as a child process; nothing of it is loaded into Python."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_dev_array_header_checks_pass_under_the_host_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "dev_array_check"
    # the sanitizers' runtimes linked into the program (clang's default): it starts whatever else the loader brings in
    static_rt = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         *static_rt, "-I", os.path.join(ROOT, "theoremsearch_amd", "csrc"), os.path.join(ROOT, "tests", "dev_array_check.cpp"), "-o", str(exe)],
        capture_output=True, text=True, timeout=280)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout
