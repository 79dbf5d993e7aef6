"""Helpers of the k-chunked matrix search's tests (theoremsearch_amd/csrc/kernels_mfma_wide.h; tests/test_wide_gpu.py on the
GPU, tests/test_wide_common_cpu.py for what holds without one).

The block-marker corpus.  The kernel stages a row in k-chunks of 1,024 bytes (8 blocks of 64 elements on bf16, 4 on fp32)
and carries the accumulators across them; what can go wrong is a chunk that is dropped, added twice, taken from the wrong
place of the row or read from a buffer that still holds an earlier chunk.  So every row marks ONE 64-element block:
  * row r is non-zero only in block b = r mod (d / 64), where it holds the constant a_r in 1 .. 8;
  * query j holds ((j + 3 blk + t) mod 5) - 2 at element 64 blk + t;
  * n = 3 d / 64 + 1 rows: every block is marked by three rows, the last row is all ones (it sees every block at once).
Every value is a small integer that bf16 holds exactly and every partial sum of every score stays far below 2^24, so fp32
adds a score exactly in any order: the library's scores must equal the integer dot products bit for bit.  Blocks five apart
see the same query pattern (3 blk mod 5), so a swap of two such blocks is invisible to the marker rows; the swaps the kernel
can make are whole chunks one or two apart (the other buffer, or this one a turn early): 4, 8 or 16 blocks, none a multiple
of five.  tests/test_wide_common_cpu.py checks with faulty_scores() which faults the corpus shows.

The chain model.  chain_scores() evaluates in numpy fp32 the sum the kernels make: one chain over the k-steps of 64 bytes in
ascending order; a bf16 k-step adds the 32 products of the step to the accumulator, an fp32 k-step is four steps of its own,
each adding the four products of float i of the step's four 16-byte pieces.  The matrix unit's own rounding inside a step
is not specified; the model rounds the step's sum to fp32 once, which is the coarsest reading.
"""
import numpy as np

MARKER_WIDTHS = {"bf16": (2304, 2560, 4096, 8192), "f32": (1280, 1536, 4096)}

GAP = 1e-6          # fp64 gap below which two ranks count as tied (tests/test_anywidth_gpu.py's)
SCORE_TOL = 1e-5    # ... and its score tolerance: kept, since the chain model stays within SCORE_TOL / 2 of fp64 on the parity
                    # cases (tests/test_wide_common_cpu.py computes it: the worst of the four is 1e-7)
PARITY = [("bf16", 2560, 20_011, 256, 10, "ip"), ("bf16", 2304, 16_385, 40, 100, "cos"),
          ("f32", 1536, 20_011, 256, 10, "cos"), ("f32", 1280, 16_384, 17, 256, "ip")]
PARITY_SEED = 7


def marker_corpus(d, nq=256):
    """(queries [nq x d] f32, rows [n x d] f32, exact scores [nq x n] int64) of the block-marker corpus at width d."""
    assert d % 64 == 0
    nb = d // 64
    n = 3 * nb + 1
    c = np.zeros((n, d), dtype=np.float32)
    r = np.arange(n - 1)
    a = 1 + (r // nb + 3 * (r % nb)) % 8                         # 1 .. 8; the three rows of a block differ
    for i in range(n - 1):
        b = i % nb
        c[i, 64 * b:64 * b + 64] = a[i]
    c[n - 1, :] = 1.0
    e = np.arange(d)
    q = (((np.arange(nq)[:, None] + 3 * (e // 64)[None, :] + (e % 64)[None, :]) % 5) - 2).astype(np.float32)
    exact = (q.astype(np.float64) @ c.astype(np.float64).T).astype(np.int64)      # small integers: exact in fp64 too
    assert np.abs(exact).max() < 2 ** 24 and np.abs(q).max() <= 2 and c.max() <= 8
    return q, c, exact


def canonical_topk(scores, k):
    """(scores f32 [nq x k], ids int64 [nq x k]): score descending, then row ascending, padded with (-inf, -1)."""
    nq, n = scores.shape
    out_s = np.full((nq, k), -np.inf, dtype=np.float32)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    m = min(k, n)
    for b in range(nq):
        order = np.lexsort((np.arange(n), -scores[b]))[:m]
        out_i[b, :m] = order
        out_s[b, :m] = scores[b, order].astype(np.float32)
    return out_s, out_i


def faulty_scores(q, c, exact, fault, b0, b1=None):
    """Integer scores of a pass that mishandles 64-element block b0 of every row (`exact`: the right ones): 'drop' leaves it
    out, 'double' adds it twice, 'swap' multiplies the rows' block b0 by the queries' block b1 and the other way round (a
    chunk taken from the wrong place, or a buffer read while it still holds another chunk)."""
    def prod(bq, bc):                 # small integers: the fp64 product is exact
        return (q[:, 64 * bq:64 * bq + 64].astype(np.float64) @ c[:, 64 * bc:64 * bc + 64].astype(np.float64).T).astype(np.int64)
    own = prod(b0, b0)
    if fault == "drop":
        return exact - own
    if fault == "double":
        return exact + own
    assert fault == "swap" and b1 is not None and b1 != b0
    return exact - own - prod(b1, b1) + prod(b1, b0) + prod(b0, b1)


def chain_scores(qp, cp, dtype):
    """fp32 scores [nq x n] of prepared operands (float32 arrays holding the stored values) as the kernels' chain adds them
    (module docstring)."""
    qp = np.ascontiguousarray(qp, dtype=np.float32)
    cp = np.ascontiguousarray(cp, dtype=np.float32)
    d = qp.shape[1]
    acc = np.zeros((qp.shape[0], cp.shape[0]), dtype=np.float32)
    if dtype == "bf16":
        for s in range(0, d, 32):
            acc += (qp[:, s:s + 32].astype(np.float64) @ cp[:, s:s + 32].astype(np.float64).T).astype(np.float32)
        return acc
    for s in range(0, d, 16):
        for i in range(4):
            cols = s + 4 * np.arange(4) + i                      # float i of the step's four 16-byte pieces
            acc += (qp[:, cols].astype(np.float64) @ cp[:, cols].astype(np.float64).T).astype(np.float32)
    return acc


def pinned_positions(truth, k):
    """[nq x k] bool: positions of the fp64 ranking whose neighbours on both sides are more than GAP away."""
    top = -np.sort(-truth, axis=1)[:, :k + 1]
    gaps = top[:, :-1] - top[:, 1:]
    hi = gaps > GAP
    lo = np.ones_like(hi)
    lo[:, 1:] = hi[:, :-1]
    return lo & hi
