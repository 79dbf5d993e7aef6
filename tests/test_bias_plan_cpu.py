"""The biased matrix search's host decisions and its threshold solver (theoremsearch_amd/csrc/bias_plan.h) need no HIP.
tests/bias_plan_check.cpp walks the served / refused table and the AUTO rule and, as `bias_plan_check solve`, answers threshold
problems given on stdin; it is built with the host compiler under the address and undefined-behaviour sanitizers and run as a
child process - nothing of it is loaded into Python.

The solver is held against a CPU model of the search: seeded iid Gaussian similarities (sd 1 / sqrt(768), what normalised
768-dimensional rows give) plus the citation recipe of tests/test_api_gpu.py's biased test (None / 0 / 1..399, twelve rows at
1e6..1e8, w = 0.02), sampled as search_mfma.hip samples (every stride-th tile of 32 rows, at most 4,096 rows below 4M).  The
threshold of a query is max(k-th best weighted sample score, solver); what the full pass would admit is counted exactly.
The solver's histogram is the search's: w * bias over every row the call may return, scale 1.  A second recipe, power-law
citation counts with w = 0.05, is the case in which a histogram of the sample's rows alone fails; that is pinned too."""
import functools
import math
import os
import shutil
import statistics
import subprocess

import numpy as np
import pytest

from conftest import ROOT

W = np.float32(0.02)
BINS = 1024
CAND_CAP = 8192          # candidate slots per query (host.h: kCandCap)


@functools.lru_cache(maxsize=1)
def check_program():
    import tempfile
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tempfile.mkdtemp(prefix="bias_plan_check_"), "bias_plan_check")
    # the sanitizers' runtimes linked into the program (clang's default): it starts whatever else the loader brings in
    static_rt = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         *static_rt, "-I", os.path.join(ROOT, "theoremsearch_amd", "csrc"), os.path.join(ROOT, "tests", "bias_plan_check.cpp"), "-o", exe],
        capture_output=True, text=True, timeout=280)
    assert build.returncode == 0, build.stdout + build.stderr
    return exe


def test_bias_plan_header_checks_pass_under_the_host_sanitizers():
    run = subprocess.run([check_program()], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout


# ---- the CPU model ----------------------------------------------------------------------------------------------------------
def powerlaw_bias(n):
    """ln of citation counts with a power-law tail: most rows 1 (no bonus), a few in the thousands and beyond."""
    return np.log(np.random.default_rng(9).zipf(2.0, n).astype(np.float64)).astype(np.float32)


def recipe_bias(n):
    rng = np.random.default_rng(9)
    u, v = rng.random(n), rng.integers(1, 400, n)
    cites = np.where(u < 0.2, 0, v).astype(np.float64)            # None and 0 both give no bonus
    cites[rng.choice(n, 12, replace=False)] = 10.0 ** rng.integers(6, 9, 12)
    return np.where(cites > 0, np.log(np.maximum(cites, 1.0)), 0.0).astype(np.float32)


def sample_rows(n):
    """search_mfma.hip, plan_levels under the default two-level search: every stride-th 32-row tile, stride the smallest
    power of two that leaves at most 4,096 sample rows (n < 4M)."""
    tiles = (n + 31) // 32
    stride = 2
    while ((tiles + stride - 1) // stride) * 32 > 4096:
        stride *= 2
    rows = (np.arange((tiles + stride - 1) // stride)[:, None] * stride * 32 + np.arange(32)[None, :]).ravel()
    return rows[rows < n]


def tail_z(p):
    return statistics.NormalDist().inv_cdf(1.0 - min(0.25, p))


def solve(problems):
    """problems: (lo, hi, mu, sigma, scale, target, histogram) -> thresholds from `bias_plan_check solve`."""
    lines = []
    for lo, hi, mu, sigma, scale, target, hist in problems:
        nz = np.flatnonzero(hist)
        lines.append(" ".join([repr(float(lo)), repr(float(hi)), repr(float(mu)), repr(float(sigma)), repr(float(scale)), repr(float(target)),
                               str(nz.size)] + [f"{b} {hist[b]}" for b in nz]))
    run = subprocess.run([check_program(), "solve"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    out = [float(t) for t in run.stdout.split()]
    assert len(out) == len(problems)
    return np.array(out)


def model(sims, bias, k, allowed=None, w=W, hist_rows="all"):
    """Per query: candidates the full pass admits under the solver's threshold, and under the mean + z sd rule on the
    weighted sample scores (level_threshold's estimate, which the biased search does not use).  hist_rows: "all" - the
    histogram over every (allowed) row, scale 1, as the search takes it - or "sample": over the sample's rows, scaled up."""
    n = bias.shape[0]
    term = np.float32(w) * bias                                   # fp32, as the kernels form it
    rows = sample_rows(n)
    if allowed is not None:
        rows = rows[allowed[rows]]
    pop = n if allowed is None else int(allowed.sum())
    target = max(64, 6 * k)
    ht = term[rows] if hist_rows == "sample" else (term if allowed is None else term[allowed])
    scale = pop / ht.shape[0]
    lo, hi = ht.min(), ht.max()
    width = np.float32((hi - lo) / np.float32(BINS)) if hi > lo else np.float32(0)
    bins = np.zeros(ht.shape[0], np.int64) if width == 0 else np.clip(((ht - lo) / width).astype(np.int64), 0, BINS - 1)
    hist = np.bincount(bins, minlength=BINS)
    weighted = sims + term[None, :].astype(np.float64)
    if allowed is not None:
        weighted = np.where(allowed[None, :], weighted, -np.inf)
    sw = weighted[:, rows]
    bound = -np.sort(-sw, axis=1)[:, k - 1]
    raw = sims[:, rows]
    thr = solve([(lo, hi, raw[b].mean(), raw[b].std(), scale, target, hist) for b in range(sims.shape[0])])
    solver_counts = (weighted >= np.maximum(bound, thr)[:, None]).sum(axis=1)
    naive = sw.mean(axis=1) + tail_z(target / pop) * sw.std(axis=1)
    naive_counts = (weighted >= np.maximum(bound, naive)[:, None]).sum(axis=1)
    return solver_counts, naive_counts


@functools.lru_cache(maxsize=1)
def million():
    n, nq = 1_000_000, 64
    sims = np.random.default_rng(123).standard_normal((nq, n), dtype=np.float32).astype(np.float64) / math.sqrt(768.0)
    return sims, recipe_bias(n)


@pytest.mark.parametrize("k", [10, 100])
def test_one_million_rows_every_query_gets_between_k_and_the_buffer(k):
    sims, bias = million()
    got, naive = model(sims, bias, k)
    print("k", k, "solver candidates", got.min(), "..", got.max(), "naive rule under-fills", int((naive < k).sum()), "of", got.shape[0])
    assert (got >= k).all() and (got <= CAND_CAP).all(), got
    # the estimate does its job, not only the guaranteed bound: within a factor of a few of the target max(64, 6 k)
    assert got.max() <= 4 * max(64, 6 * k), got


def test_a_forty_per_cent_mask_over_20011_rows():
    n, nq, k = 20_011, 40, 10
    rng = np.random.default_rng(5)
    sims = rng.standard_normal((nq, n)) / math.sqrt(768.0)
    allowed = rng.random(n) < 0.4
    got, _ = model(sims, recipe_bias(n), k, allowed)
    print("masked: solver candidates", got.min(), "..", got.max())
    assert (got >= k).all() and (got <= CAND_CAP).all(), got


def test_mean_plus_z_sd_of_the_weighted_scores_under_fills_most_queries():
    """The reason for the design: the weighted score is a Gaussian plus a bounded, left-skewed term with a spike at 0; the
    Gaussian extrapolation of its sd overshoots the quantile, and a query with fewer than k candidates is an exact re-run."""
    sims, bias = million()
    _, naive = model(sims, bias, 10)
    assert (naive < 10).sum() > naive.shape[0] // 2, naive


@pytest.mark.parametrize("k", [10, 100])
def test_power_law_counts_over_one_million_rows(k):
    """Power-law citation counts, w = 0.05: the top k are decided by the far tail of the term (up to 16 sd of the
    similarities above the rest).  With the histogram over all rows every query is served."""
    sims, _ = million()
    got, _ = model(sims, powerlaw_bias(sims.shape[1]), k, w=0.05)
    print("power law, k", k, "candidates", got.min(), "..", got.max())
    assert (got >= k).all() and (got <= CAND_CAP).all(), got
    assert got.max() <= 4 * max(64, 6 * k), got


def test_the_histogram_of_the_sample_alone_under_fills_under_power_law_counts():
    """Why the search pays a pass over the whole bias array: a 3,936-row sample of 1M rows holds two or three rows of the
    tail, each then stands for 254 rows with exactly its term, and the threshold aims at the upper part of such a phantom
    pile.  More than 2 of 256 queries with fewer than k candidates is the share at which the estimator is not doing its job."""
    sims, _ = million()
    got, _ = model(sims, powerlaw_bias(sims.shape[1]), 10, w=0.05, hist_rows="sample")
    print("power law, sample histogram: candidates", got.min(), "..", got.max(), "under-filled", int((got < 10).sum()), "of", got.shape[0])
    assert (got < 10).mean() > 2 / 256, got
