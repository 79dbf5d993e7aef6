"""PCA of the whole embedding table from its moments, taken where the rows lie in HBM, and the category means in PCA space.

The reference's ``experiments/pca_plotting.py`` (the paper's Figure 1 and Figure 2) streams every embedding out of Postgres
twice, in batches of 5,000: once through ``IncrementalPCA.partial_fit``, once through ``transform`` to accumulate a mean per
``primary_category``.  Here the table is a `TheoremIndex` and the categories a `MetaTable` column, and the only heavy step is
``TheoremIndex.moments`` - count, column sums and the Gram matrix X^T X of the stored rows, two HIP passes - plus
``TheoremIndex.group_sums`` for the per-category sums.  The rest is linear algebra on d x d and C x d numbers in fp64 on the host:

* the covariance is ``(G - n mean mean^T) / (n - 1)`` and its eigenvectors are the components.  This is the EXACT PCA of the
  rows: the one ``IncrementalPCA`` approximates batch by batch (its result depends on the batch order and size; this does not);
* ``mean_c(Z) = (mean_c(X) - mean(X)) V^T``: the category means need no pass over projected rows.

Moments are additive, so those of a sharded corpus are the sums of its shards' (`fit_moments` takes the sums).
numpy only; nothing here plots.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np


class PCAModel:
    """The fitted decomposition, named as sklearn names it: ``mean_`` [d], ``components_`` [k x d] (rows of unit length),
    ``explained_variance_`` [k], ``explained_variance_ratio_`` [k], ``n_samples_seen_``."""

    def __init__(self, mean, components, explained_variance, explained_variance_ratio, n_samples_seen):
        self.mean_ = mean
        self.components_ = components
        self.explained_variance_ = explained_variance
        self.explained_variance_ratio_ = explained_variance_ratio
        self.n_samples_seen_ = int(n_samples_seen)
        self.n_components_ = components.shape[0]

    def transform(self, X) -> np.ndarray:
        """``(X - mean_) components_^T`` in fp64."""
        X = np.asarray(X, dtype=np.float64)
        return (X - self.mean_) @ self.components_.T


def fit_moments(count: int, total, gram, n_components: int = 2) -> PCAModel:
    """The PCA of rows known only by their moments: ``count`` rows, their column sums ``total`` [d] and Gram matrix ``gram``
    [d x d].  Covariance ``(G - n mean mean^T) / (n - 1)`` in fp64, ``numpy.linalg.eigh``, largest eigenvalues first; in each
    component the entry of largest magnitude is positive (sklearn's sign rule for PCA)."""
    n = int(count)
    total = np.asarray(total, dtype=np.float64)
    gram = np.asarray(gram, dtype=np.float64)
    d = total.shape[0]
    if n < 2:
        raise ValueError(f"a PCA needs at least two rows, got {n}")
    if not 1 <= n_components <= d:
        raise ValueError(f"n_components = {n_components} outside [1, {d}]")
    mean = total / n
    cov = (gram - n * np.outer(mean, mean)) / (n - 1)
    cov = (cov + cov.T) * 0.5
    w, v = np.linalg.eigh(cov)                       # ascending
    order = np.argsort(-w, kind="stable")[:n_components]
    comps = v[:, order].T.copy()
    big = np.argmax(np.abs(comps), axis=1)
    signs = np.sign(comps[np.arange(comps.shape[0]), big])
    signs[signs == 0] = 1.0
    comps *= signs[:, None]
    var = np.maximum(w[order], 0.0)
    total_var = float(np.trace(cov))
    ratio = var / total_var if total_var > 0 else np.zeros_like(var)
    return PCAModel(mean, comps, var, ratio, n)


def fit(index, n_components: int = 2, rowset=None) -> PCAModel:
    """PCA of the stored rows of ``index`` (those ``rowset`` allows): one `TheoremIndex.moments` call, then `fit_moments`.
    The exact PCA that the reference's ``IncrementalPCA`` approximates batch by batch."""
    count, total, gram = index.moments(rowset=rowset, gram=True)
    return fit_moments(count, total, gram, n_components)


def means_from_sums(names: Sequence, counts, sums, model: PCAModel):
    """``(cats sorted, M float32 [C x n_components], counts int64)`` from per-category counts and column sums: the mean of each
    category's rows in PCA space, ``(sums_c / count_c - mean_) components_^T``.  Categories without a row are dropped (the
    reference's ``MeanAccumulator`` never sees them); the categories are sorted by their names as strings."""
    counts = np.asarray(counts, dtype=np.int64)
    sums = np.asarray(sums, dtype=np.float64)
    keep = [i for i in np.argsort(np.array([str(c) for c in names], dtype=object), kind="stable") if counts[i] > 0]
    k = model.components_.shape[0]
    if not keep:
        return [], np.zeros((0, k), dtype=np.float32), np.zeros(0, dtype=np.int64)
    means = sums[keep] / counts[keep, None]
    M = ((means - model.mean_) @ model.components_.T).astype(np.float32)
    return [names[i] for i in keep], M, counts[keep]


def category_means(index, meta, column, model: PCAModel, rowset=None):
    """The mean of every category of ``meta``'s ``column`` in the PCA space of ``model``, over all rows of ``index`` (those
    ``rowset`` allows): one `TheoremIndex.group_sums` pass, then `means_from_sums`.  No row is projected."""
    names, counts, sums = index.group_sums(meta, column, rowset=rowset)
    return means_from_sums(names, counts, sums, model)


def pairwise_distances(M) -> np.ndarray:
    """Euclidean distance between every two rows of ``M`` [C x k]: D [C x C]."""
    M = np.asarray(M)
    diff = M[:, None, :] - M[None, :, :]
    return np.sqrt((diff * diff).sum(axis=2))


def closest_pairs(cats: Sequence, M, topk: Optional[int] = 30):
    """The ``topk`` closest pairs of category means (all for None): ``[(distance, cat_i, cat_j), ...]`` with i before j in
    ``cats``, ordered by distance, then by the two names."""
    D = pairwise_distances(M)
    n = len(cats)
    pairs = [(float(D[i, j]), cats[i], cats[j]) for i in range(n) for j in range(i + 1, n)]
    pairs.sort(key=lambda t: (t[0], str(t[1]), str(t[2])))
    return pairs if topk is None else pairs[:topk]


def _f64_rows(rows: np.ndarray) -> np.ndarray:
    if rows.dtype == np.uint16:                      # bf16 bits
        rows = (rows.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return rows.astype(np.float64)


def project_sample(index, model: PCAModel, rows, via: str = "download") -> np.ndarray:
    """The sample of the scatter plot: rows ``rows`` (local row numbers) of ``index`` in the PCA space of ``model``, float64
    [len(rows) x n_components].

    ``via="download"`` (the default) fetches the stored rows (``ts_index_download``, one call per run of consecutive rows) and
    projects them on the host in fp64.  ``via="scores"`` scores ALL rows against the components as queries (``ts_scores``: a
    [n_components x n] float32 matrix, small tables only) and picks the sample's columns; on that path a bf16 index rounds
    the components to bf16 and the products are added in fp32, so the coordinates carry about three decimal digits.  The
    category means (`category_means`) never go that way: they come from fp64 sums and the fp64 components."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    k = model.components_.shape[0]
    if rows.size == 0:
        return np.zeros((0, k), dtype=np.float64)
    if via == "scores":
        s = index.scores(model.components_.astype(np.float32))             # [k x n]
        return s[:, rows].T.astype(np.float64) - model.mean_ @ model.components_.T
    if via != "download":
        raise ValueError(f"via = {via!r}: 'download' or 'scores'")
    order = np.argsort(rows, kind="stable")
    out = np.empty((rows.size, k), dtype=np.float64)
    i = 0
    while i < rows.size:
        j = i
        while j + 1 < rows.size and rows[order[j + 1]] == rows[order[j]] + 1:
            j += 1
        block = _f64_rows(index.download(int(rows[order[i]]), j - i + 1))
        out[order[i:j + 1]] = model.transform(block)
        i = j + 1
    return out
