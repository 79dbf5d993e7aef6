"""Host side of the corpus PCA (theoremsearch_amd/pca.py) from hand-made moments, no device: `fit_moments` against an fp64 SVD
of the centred matrix (and sklearn's full-SVD PCA where sklearn is installed), `means_from_sums` against the mean of the
transformed rows, `closest_pairs`' order, one committed tiny case, and the new entry points' behaviour without a device.

tests/golden/pca_small.json, recipe (`golden_case` below is the generator; the file holds its seeds and its outputs):
    rng = numpy.random.default_rng(seed); centres = rng.normal(size=(ncats, d)) * 2
    cat = rng.integers(0, ncats, size=n); X = float32(centres[cat] + rng.normal(size=(n, d)))
    model = pca.fit_moments(n, X.sum(0), X.T @ X in fp64, 2)
    cats, M, counts = pca.means_from_sums(names, bincount(cat), per-category sums, model); pairs = pca.closest_pairs(cats, M, 5)
with names "c<k>" (so "c10" sorts before "c2").  Written by `python tests/test_pca_cpu.py` from the repository root."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, gpu_available, golden_path
from theoremsearch_amd import _ffi, pca

EPS = 2.0 ** -52


def planted(n=500, d=64, seed=7):
    """[n x d] fp64 rows with covariance eigenvalues 50, 20, 8 and then at most 1, plus a mean of about 0.5 a column."""
    rng = np.random.default_rng(seed)
    u, _ = np.linalg.qr(rng.normal(size=(n, d)))
    u -= u.mean(axis=0)                                  # centred columns: the centred matrix is u diag(s) v^T up to rounding
    u, _ = np.linalg.qr(u)
    v, _ = np.linalg.qr(rng.normal(size=(d, d)))
    lam = np.concatenate([[50.0, 20.0, 8.0], np.linspace(1.0, 0.1, d - 3)])
    x = (u * np.sqrt(lam * (n - 1))) @ v.T
    x -= x.mean(axis=0)
    return x + rng.normal(size=d) * 0.5, lam


def tolerances(x, gram, k):
    """Perturbation bounds, computed: the covariance from moments carries dC <= c eps (||G|| + n |mean|^2) / (n - 1) of fp64
    rounding (c = 4 d: a d-term inner product per entry, the outer product, the subtraction); Weyl moves an eigenvalue by at
    most dC, Davis-Kahan turns an eigenvector by at most 2 dC / gap.  The SVD it is compared with carries the same order."""
    n, d = x.shape
    mean = x.mean(axis=0)
    dC = 4 * d * EPS * (np.linalg.norm(gram, 2) + n * float(mean @ mean)) / (n - 1)
    lam = np.sort(np.linalg.eigvalsh(np.cov(x.T)))[::-1]
    gap = min(lam[i] - lam[i + 1] for i in range(k))
    return 2 * dC, 2 * 2 * dC / gap


def test_fit_agrees_with_the_svd_of_the_centred_matrix():
    x, lam = planted()
    n, d = x.shape
    k = 3
    gram = x.T @ x
    m = pca.fit_moments(n, x.sum(axis=0), gram, k)
    xc = x - x.mean(axis=0)
    _, s, vt = np.linalg.svd(xc, full_matrices=False)
    tol_val, tol_vec = tolerances(x, gram, k)
    print("tolerances", tol_val, tol_vec)
    assert tol_vec < 1e-9, "the planted gap makes the bound a sharp one"
    assert m.n_samples_seen_ == n and m.components_.shape == (k, d)
    assert np.abs(m.mean_ - x.mean(axis=0)).max() <= 4 * EPS * np.abs(x).max()
    var = s[:k] ** 2 / (n - 1)
    assert np.abs(m.explained_variance_ - var).max() <= tol_val
    assert np.abs(m.explained_variance_ - lam[:k]).max() <= 1e-9 * lam[0]          # the planted spectrum itself
    assert np.abs(m.explained_variance_ratio_ - var / (s ** 2).sum() * (n - 1)).max() <= tol_val / var.sum() + 4 * d * EPS
    for i in range(k):
        ref = vt[i] * np.sign(vt[i][np.argmax(np.abs(vt[i]))])                    # the sign rule applied to the reference
        assert np.linalg.norm(m.components_[i] - ref) <= tol_vec, i
        assert m.components_[i][np.argmax(np.abs(m.components_[i]))] > 0
        assert abs(np.linalg.norm(m.components_[i]) - 1) <= 4 * d * EPS
    assert np.abs(m.transform(x) - xc @ m.components_.T).max() <= 8 * d * EPS * np.abs(xc).max() * 2


def test_fit_agrees_with_sklearn_full_pca():
    skd = pytest.importorskip("sklearn.decomposition")
    x, _ = planted()
    n, d = x.shape
    k = 3
    gram = x.T @ x
    m = pca.fit_moments(n, x.sum(axis=0), gram, k)
    ref = skd.PCA(n_components=k, svd_solver="full").fit(x)
    tol_val, tol_vec = tolerances(x, gram, k)
    assert np.abs(m.explained_variance_ - ref.explained_variance_).max() <= tol_val
    assert np.abs(m.explained_variance_ratio_ - ref.explained_variance_ratio_).max() <= tol_val / ref.explained_variance_.sum() + 4 * d * EPS
    for i in range(k):
        assert np.linalg.norm(m.components_[i] - ref.components_[i]) <= tol_vec, i        # signs included
    assert np.abs(m.mean_ - ref.mean_).max() <= 4 * EPS * np.abs(x).max()


def test_fit_refuses_what_has_no_pca():
    with pytest.raises(ValueError):
        pca.fit_moments(1, np.zeros(4), np.zeros((4, 4)), 2)
    with pytest.raises(ValueError):
        pca.fit_moments(10, np.zeros(4), np.zeros((4, 4)), 5)


def test_category_means_are_the_means_of_the_transformed_rows():
    x, _ = planted()
    n, d = x.shape
    rng = np.random.default_rng(3)
    names = ["math.AG", "math.NT", "math.CO", "math.empty", "math.AP"]
    cat = rng.choice([0, 1, 2, 4], size=n)                                          # category 3 has no row
    m = pca.fit_moments(n, x.sum(axis=0), x.T @ x, 2)
    sums = np.zeros((len(names), d))
    np.add.at(sums, cat, x)
    cats, M, counts = pca.means_from_sums(names, np.bincount(cat, minlength=len(names)), sums, m)
    assert cats == ["math.AG", "math.AP", "math.CO", "math.NT"] and M.dtype == np.float32 and M.shape == (4, 2)
    z = m.transform(x)
    for row, c in enumerate(cats):
        sel = cat == names.index(c)
        ref = z[sel].mean(axis=0)
        assert counts[row] == sel.sum()
        # fp64 sums of at most n terms on both sides, then one rounding to float32
        tol = 2.0 ** -24 * np.abs(ref).max() + 4 * n * EPS * np.abs(z).max()
        assert np.abs(M[row].astype(np.float64) - ref).max() <= tol, c


def test_closest_pairs_are_ordered_by_distance_then_names():
    cats = ["b", "a", "d", "c"]
    M = np.array([[0, 0], [3, 4], [0, 5], [3, 0]], dtype=np.float32)      # distances: 3, sqrt(10), 4, 5 twice (a tie), sqrt(34)
    pairs = pca.closest_pairs(cats, M, topk=None)
    assert [p[0] for p in pairs] == sorted(p[0] for p in pairs)
    assert pairs == sorted(pairs, key=lambda t: (t[0], t[1], t[2]))
    assert [(p[1], p[2]) for p in pairs] == [("b", "c"), ("a", "d"), ("a", "c"), ("b", "a"), ("b", "d"), ("d", "c")]
    assert pca.closest_pairs(cats, M, topk=2) == pairs[:2]
    D = pca.pairwise_distances(M)
    assert D.shape == (4, 4) and np.array_equal(D, D.T) and np.all(np.diag(D) == 0) and D[0, 1] == 5


def golden_case(seed=11, n=240, d=8, ncats=12):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(ncats, d)) * 2
    cat = rng.integers(0, ncats, size=n)
    x = (centres[cat] + rng.normal(size=(n, d))).astype(np.float32).astype(np.float64)
    names = [f"c{k}" for k in range(ncats)]
    m = pca.fit_moments(n, x.sum(axis=0), x.T @ x, 2)
    sums = np.zeros((ncats, d))
    np.add.at(sums, cat, x)
    cats, M, counts = pca.means_from_sums(names, np.bincount(cat, minlength=ncats), sums, m)
    return {"seed": seed, "n": n, "d": d, "ncats": ncats, "cats": cats, "means": M.astype(np.float64).tolist(), "counts": counts.tolist(),
            "explained_variance": m.explained_variance_.tolist(),
            "closest": [[p[0], p[1], p[2]] for p in pca.closest_pairs(cats, M, 5)]}


def test_committed_small_case():
    with open(golden_path("pca_small.json")) as f:
        want = json.load(f)
    got = golden_case(want["seed"], want["n"], want["d"], want["ncats"])
    assert got["cats"] == want["cats"] == sorted(want["cats"]) and got["counts"] == want["counts"]
    assert want["cats"].index("c10") < want["cats"].index("c2")
    # float32 means of O(1) numbers: another BLAS may move the fp64 value by rounding, the float32 by at most an ulp or two
    scale = np.abs(np.array(want["means"])).max()
    assert np.abs(np.array(got["means"]) - np.array(want["means"])).max() <= 4 * 2.0 ** -24 * scale
    assert np.abs(np.array(got["explained_variance"]) - np.array(want["explained_variance"])).max() <= 1e-12 * want["explained_variance"][0]
    assert [p[1:] for p in got["closest"]] == [p[1:] for p in want["closest"]]
    assert np.abs(np.array([p[0] for p in got["closest"]]) - np.array([p[0] for p in want["closest"]])).max() <= 8 * 2.0 ** -24 * scale


def test_moments_plan_needs_no_device_and_refuses_other_widths():
    lib = _ffi.load()
    L, panel, ranges, pbytes = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0)
    assert lib.ts_moments_plan(_ffi.TS_BF16, 1024, 10_000_000, 256, C.byref(L), C.byref(panel), C.byref(ranges), C.byref(pbytes)) == 0
    assert L.value == 8192 and panel.value == 128 and 1 <= ranges.value <= 512 and 0 < pbytes.value <= 256 << 20
    for d in (64, 1088, 2048, 200):
        assert lib.ts_moments_plan(_ffi.TS_F32, d, 1000, 256, None, None, None, None) == -5
        assert b"no kernel" in lib.ts_last_error()


@pytest.mark.skipif(gpu_available(), reason="checks the no-device behaviour")
def test_moments_fail_loudly_without_device():
    """No index can exist without a device, so `TheoremIndex.moments` / `group_sums` and `pca.fit` fail where every compute entry
    does: at the handle, with TS_ERR_NODEVICE; the entry points themselves refuse the missing handle."""
    from theoremsearch_amd import TheoremIndex
    assert _ffi.device_count() == 0
    with pytest.raises(_ffi.TSearchError) as e:
        with TheoremIndex(16, 128) as ix:
            pca.fit(ix)
    assert e.value.code == -4 and "no CPU path" in str(e.value)
    lib = _ffi.load()
    cnt, s = C.c_int64(7), np.zeros(128)
    assert lib.ts_index_moments(None, None, C.byref(cnt), _ffi.as_ptr(s), None, None) == -1
    assert b"NULL" in lib.ts_last_error()
    assert lib.ts_index_group_sums(None, None, 0, 1, None, None, None, None) == -1
    assert b"NULL" in lib.ts_last_error()


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    with open(os.path.join(ROOT, "tests", "golden", "pca_small.json"), "w") as f:
        json.dump(golden_case(), f, indent=1)
        f.write("\n")
