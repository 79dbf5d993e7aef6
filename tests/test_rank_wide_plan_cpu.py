"""The k-chunked rank pass's host decisions (theoremsearch_amd/csrc/rank_wide_plan.h: the widths it serves, the tile and the
LDS bytes of its launches) are plain integer arithmetic in a header that needs no HIP.  tests/rank_wide_plan_check.cpp checks
them in a program of its own, built with the host compiler under the address and undefined-behaviour sanitizers and run as a
child process; nothing of it is loaded into Python.

And what tests/test_rank_many_wide_gpu.py takes for granted, checked without a GPU: on its parity inputs the fp32 chain the
kernels add (wide_common.chain_scores) stays within SCORE_TOL / 2 of the fp64 scores, which is why the parity test keeps the
narrower widths' tolerance."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rank_common as RC
import rank_wide_common as RW
import wide_common as WC
from conftest import ROOT
from oracle import oracle


def test_rank_wide_plan_header_checks_pass_under_the_host_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "rank_wide_plan_check"
    # the sanitizers' runtimes linked into the program (clang's default): it starts whatever else the loader brings in
    static_rt = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         *static_rt, "-I", os.path.join(ROOT, "theoremsearch_amd", "csrc"), os.path.join(ROOT, "tests", "rank_wide_plan_check.cpp"), "-o", str(exe)],
        capture_output=True, text=True, timeout=280)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout


def test_the_tolerances_are_the_narrower_widths():
    assert RC.SCORE_TOL == WC.SCORE_TOL == 1e-5 and RC.GAP == WC.GAP == 1e-6


@pytest.mark.parametrize("nq", RW.PARITY_NQ)
@pytest.mark.parametrize("dtype,d", RW.PARITY_WIDTHS, ids=lambda v: str(v))
def test_the_chain_model_stays_within_half_the_score_tolerance_on_the_parity_inputs(dtype, d, nq):
    """Every query against the first 512 rows of the parity case (the rows are independent draws: the error of a score does not
    depend on the row's position)."""
    _, _, qp, cp = RW.parity_inputs(dtype, d, nq)
    qp, cp = np.asarray(qp, dtype=np.float32), np.asarray(cp, dtype=np.float32)[:512]
    truth = oracle.scores_fp64(qp, cp)
    model = WC.chain_scores(qp, cp, dtype)
    worst = float(np.abs(model.astype(np.float64) - truth).max())
    print(dtype, d, nq, "worst |chain - fp64|", worst)
    assert worst <= RC.SCORE_TOL / 2
