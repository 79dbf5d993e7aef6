"""The cross-shard merge (kernels_merge.h: merge_kernel, launch_merge) against a numpy model, at the sizes where launch_merge
changes its instantiation: nparts * k_in <= 128 runs one wave, <= 1024 the 1,024-entry form, the rest up to kMergeMax =
4,096 the large one.  Both entry points of shards.hip: ts_merge_topk (host arrays) and ts_merge_topk_packed (one device
buffer laid out as the sharded search lays out its exchange blocks), and their refusals.

The model: entries with a negative id or a NaN score are padding; the rest in order of score descending, then id ascending;
missing results are (-inf, -1).  Scores and ids are compared exactly."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ = 3
SHAPES = [(2, 64), (3, 43), (16, 64), (5, 205), (16, 256)]     # 128, 129, 1024, 1025, 4096 entries per query
K_OUT = [1, 10, 256]
TS_ERR_INVALID, TS_ERR_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


@functools.lru_cache(maxsize=None)
def make_case(nparts, k_in, k_out):
    """-> (scores [nparts, NQ, k_in] f32, ids [nparts, NQ, k_in] i64, expected scores [NQ, k_out], expected ids); read-only"""
    m = nparts * k_in
    rng = np.random.default_rng(1000 * nparts + k_in)
    scores = rng.standard_normal((nparts, NQ, k_in)).astype(np.float32)
    ids = np.empty((nparts, NQ, k_in), np.int64)
    for q in range(NQ):
        perm = rng.permutation(m).astype(np.int64)
        v = perm * 3 + 7                                          # distinct within a query ...
        v[perm % 4 == 0] += (1 << 33) + 5                         # ... a quarter of them above 2^33
        ids[:, q, :] = v.reshape(nparts, k_in)
    # query 0: a run of equal scores across the parts, at the top (the order inside it is the ids')
    scores[:, 0, 0] = 3.5
    scores[0, 0, 1:3] = 3.5
    # query 1: padding entries (as a shard with fewer rows than k returns them), ids without a score, scores without an id
    scores[:, 1, k_in - 3:] = -np.inf
    ids[:, 1, k_in - 3:] = -1
    scores[0, 1, 0:2] = np.nan                                    # NaN score, valid id: dropped
    scores[nparts - 1, 1, 5] = np.nan
    ids[0, 1, 4] = -1                                             # finite score, no id: dropped
    # query 2: fewer live entries than k_out (none at k_out = 1)
    live = min(5, k_out - 1)
    flat_s, flat_i = scores[:, 2, :].reshape(-1).copy(), ids[:, 2, :].reshape(-1).copy()
    keep = rng.permutation(m)[:live]
    dead = np.ones(m, bool)
    dead[keep] = False
    flat_s[dead] = -np.inf
    flat_i[dead] = -1
    scores[:, 2, :] = flat_s.reshape(nparts, k_in)
    ids[:, 2, :] = flat_i.reshape(nparts, k_in)

    exp_s = np.full((NQ, k_out), -np.inf, np.float32)
    exp_i = np.full((NQ, k_out), -1, np.int64)
    for q in range(NQ):
        s, i = scores[:, q, :].reshape(-1), ids[:, q, :].reshape(-1)
        ok = (i >= 0) & ~np.isnan(s)
        s, i = s[ok], i[ok]
        order = np.lexsort((i, -s))[:k_out]
        exp_s[q, :order.size] = s[order]
        exp_i[q, :order.size] = i[order]
    for a in (scores, ids, exp_s, exp_i):
        a.setflags(write=False)
    return scores, ids, exp_s, exp_i


def packed_buffer(torch, scores, ids, extra):
    """The parts as blocks of one device buffer, as distributed.py lays them out: scores at 0, ids at the 8-byte-rounded
    offset, part p at p * stride; `extra` bytes of slack behind each block.  -> (tensor, stride, idx offset)"""
    from theoremsearch_amd.distributed import packed_bytes, packed_idx_off
    nparts, nq, k_in = scores.shape
    off, stride = packed_idx_off(nq, k_in), packed_bytes(nq, k_in) + extra
    host = np.full(nparts * stride, 0xA5, np.uint8)
    for p in range(nparts):
        host[p * stride:p * stride + nq * k_in * 4] = np.ascontiguousarray(scores[p]).view(np.uint8).reshape(-1)
        host[p * stride + off:p * stride + off + nq * k_in * 8] = np.ascontiguousarray(ids[p]).view(np.uint8).reshape(-1)
    return torch.from_numpy(host).cuda(), stride, off


def merge_packed(buf, stride, off, nparts, nq, k_in, k_out):
    """-> (return code, scores, ids) of ts_merge_topk_packed on the current stream"""
    import torch
    from theoremsearch_amd import _ffi
    out_s = torch.full((nq, k_out), 7.0, dtype=torch.float32, device="cuda")
    out_i = torch.full((nq, k_out), 7, dtype=torch.int64, device="cuda")
    rc = _ffi.load().ts_merge_topk_packed(0, C.c_void_p(buf.data_ptr()), stride, off, nparts, nq, k_in, k_out,
                                          C.c_void_p(out_s.data_ptr()), C.c_void_p(out_i.data_ptr()), None)
    torch.cuda.synchronize()
    return rc, out_s.cpu().numpy(), out_i.cpu().numpy()


@pytest.mark.parametrize("k_out", K_OUT)
@pytest.mark.parametrize("nparts,k_in", SHAPES)
def test_merge_matches_the_model_through_both_entry_points(ts, nparts, k_in, k_out):
    import torch
    scores, ids, exp_s, exp_i = make_case(nparts, k_in, k_out)
    got_s, got_i = ts.merge_topk(scores, ids, k_out)
    assert np.array_equal(got_i, exp_i)
    assert np.array_equal(got_s, exp_s)

    buf, stride, off = packed_buffer(torch, scores, ids, extra=24)
    rc, got_s, got_i = merge_packed(buf, stride, off, nparts, NQ, k_in, k_out)
    assert rc == 0
    assert np.array_equal(got_i, exp_i)
    assert np.array_equal(got_s, exp_s)


def test_more_entries_than_the_merge_holds_are_refused(ts):
    import torch
    nparts, k_in = 17, 241                                        # 4,097 entries
    scores = np.zeros((nparts, NQ, k_in), np.float32)
    ids = np.arange(nparts * NQ * k_in, dtype=np.int64).reshape(nparts, NQ, k_in)
    with pytest.raises(ts.TSearchError) as e:
        ts.merge_topk(scores, ids, 10)
    assert e.value.code == TS_ERR_UNSUPPORTED
    buf, stride, off = packed_buffer(torch, scores, ids, extra=24)
    rc, got_s, got_i = merge_packed(buf, stride, off, nparts, NQ, k_in, 10)
    assert rc == TS_ERR_UNSUPPORTED
    assert (got_s == 7.0).all() and (got_i == 7).all()            # nothing ran


def test_bad_packed_layouts_are_refused(ts):
    import torch
    nparts, k_in = 3, 43
    scores, ids, _, _ = make_case(nparts, k_in, 10)
    buf, stride, off = packed_buffer(torch, scores, ids, extra=24)
    for bad_stride, bad_off in [(stride + 4, off),                              # stride no multiple of 8
                                (stride, (NQ * k_in * 4 - 8) // 8 * 8)]:        # ids would overlap the scores
        rc, got_s, got_i = merge_packed(buf, bad_stride, bad_off, nparts, NQ, k_in, 10)
        assert rc == TS_ERR_INVALID
        assert (got_s == 7.0).all() and (got_i == 7).all()
