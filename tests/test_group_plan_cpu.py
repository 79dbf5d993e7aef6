"""The grouped search's host decisions (theoremsearch_amd/csrc/group_plan.h: the depths of the ladder, the certificate of a
collapsed list, the membership search the exclusion kernel runs, the validation of the three entries) are plain integer
arithmetic in a header that needs no HIP.  tests/group_plan_check.cpp checks them in a program of its own, built with the host
compiler under the address and undefined-behaviour sanitizers and run as a child process; nothing of it is loaded into Python."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_group_plan_header_checks_pass_under_the_host_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "group_plan_check"
    # the sanitizers' runtimes linked into the program (clang's default): it starts whatever else the loader brings in
    static_rt = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         *static_rt, "-I", os.path.join(ROOT, "theoremsearch_amd", "csrc"), os.path.join(ROOT, "tests", "group_plan_check.cpp"), "-o", str(exe)],
        capture_output=True, text=True, timeout=280)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout
