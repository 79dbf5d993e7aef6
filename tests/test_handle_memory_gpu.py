"""The index handle's device memory over its whole life, through the public Python API only: every buffer a handle makes
lazily (search scratch, result buffers at two sizes, mask and bias copies, the matrix path's lists, the int8 screen's image,
the rank buffers), the re-makes (a larger k, an append that moves the rows and with them the screen's image), the borrowed
pointers (a view's rows, rows attached by the caller) and the destruction of all of it - eight times in one process.  The
shapes are small (4,096 rows), so a buffer freed twice, freed early or kept past its owner shows as a wrong answer or an
error code: every answer of every cycle is compared exactly with the first cycle's, and the first cycle's with a rebuilt
index and with numpy.  No device-wide free-memory figure is read: the device is shared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, GROW, CYCLES = 4096, 600, 8      # GROW rows appended: past n_pad = 4,096, the rows move


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(20261019)
    out = {}
    for name, d, nq in (("bf16", 768, 256), ("f32", 100, 5)):
        out[name] = dict(d=d, c=rng.standard_normal((N + GROW, d), dtype=np.float32), q=rng.standard_normal((nq, d), dtype=np.float32))
    out["mask"] = rng.random(N) < 0.5
    out["bias"] = rng.random(N, dtype=np.float32)
    out["targets"] = [rng.integers(0, N, size=3) for _ in range(5)]
    return out


def device_search(ix, q_dev, nq, k, algo):
    import torch
    s = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    i = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    ix.search_device(q_dev.data_ptr(), "f32", nq, k, s.data_ptr(), i.data_ptr(), algo=algo)
    ix.synchronize()
    return [s.cpu().numpy(), i.cpu().numpy()]


def index_life(ts, data, name, dtype, metric, algo, options):
    """One index from creation to destruction; returns every answer it gave, in order."""
    import torch
    w = data[name]
    c, q, nq = w["c"], w["q"], w["q"].shape[0]
    q_dev = torch.from_numpy(q).cuda()
    got = []
    ix = ts.TheoremIndex.from_embeddings(c[:N], dtype=dtype, metric=metric)
    for o, v in options.items():
        ix.set_option(o, v)
    # host and device results at two result sizes: the larger k re-makes the handle's result buffers and the scan's partials
    for k in (10, 200):
        s, i, stats = ix.search(q, k, algo=algo, return_stats=True)
        if algo == "mfma":
            assert stats["algo"] == ts._ffi.TS_ALGO_MFMA and stats["screened"] == 1, stats    # the matrix path, int8 screen included
        got += [s, i] + device_search(ix, q_dev, nq, k, algo)
        assert np.array_equal(got[-1], i) and np.array_equal(got[-2], s)
    got += list(ix.search(q, 10, mask=data["mask"]))                                     # (so few rows: the scan serves a host mask)
    assert data["mask"][got[-1][got[-1] >= 0]].all()
    got += list(ix.search_biased(q, 10, data["bias"], 0.25))                            # the scan with a bias
    if algo == "mfma":
        got += list(ix.search_biased(q, 10, data["bias"], 0.25, algo="mfma"))           # the matrix pass with a bias
    ranks, scores = ix.rank_many(q[:5], data["targets"])
    got += ranks + scores
    got += list(ix.rank_of(q[:5], [t[0] for t in data["targets"]]))
    # growth past the padding: the rows move (and the screen's image is made anew); the answer is a rebuilt index's
    rows_before = ix.info()["rows_ptr"]
    assert ix.append(c[N:]) == N
    assert ix.info()["rows_ptr"] != rows_before
    s, i = ix.search(q, 10, algo=algo)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric=metric) as rebuilt:
        for o, v in options.items():
            rebuilt.set_option(o, v)
        rs, ri = rebuilt.search(q, 10, algo=algo)
        assert np.array_equal(ix.download(), rebuilt.download())
    assert np.array_equal(i, ri) and np.array_equal(s, rs)
    got += [s, i]
    # a view borrows the rows: it searches them, its destruction leaves them to the parent
    v = ix.view()
    got += list(v.search(q, 10, algo=algo))
    assert np.array_equal(got[-1], i)
    v.close()
    got += list(ix.search(q, 10, algo=algo))
    assert np.array_equal(got[-1], i) and np.array_equal(got[-2], s)
    ix.close()
    return got


def attached_life(ts, data, name, dtype, algo):
    """Rows that belong to the caller: searched in place, and still the caller's, bit for bit, after the index has gone."""
    import torch
    w = data[name]
    ld = (w["d"] + 63) // 64 * 64
    rows = torch.zeros((N, ld), dtype=torch.bfloat16 if dtype == "bf16" else torch.float32, device="cuda")
    rows[:, :w["d"]] = torch.from_numpy(w["c"][:N]).cuda().to(rows.dtype)
    before = rows.clone()
    torch.cuda.synchronize()
    ix = ts.TheoremIndex(N, w["d"], dtype=dtype, metric="ip")
    ix.attach_device(rows.data_ptr(), N, keep_alive=rows)
    got = list(ix.search(w["q"], 10, algo=algo))
    ix.close()
    torch.cuda.synchronize()
    assert torch.equal(rows.view(torch.int16 if dtype == "bf16" else torch.int32), before.view(torch.int16 if dtype == "bf16" else torch.int32))
    return got


def one_cycle(ts, data):
    return {
        "bf16": index_life(ts, data, "bf16", "bf16", "ip", "mfma", {"TS_MFMA_FIRST_ROWS": 2048}),    # 4,096 rows behind a threshold: screened
        "f32": index_life(ts, data, "f32", "f32", "cos", "scan", {}),
        "attached bf16": attached_life(ts, data, "bf16", "bf16", "mfma"),
        "attached f32": attached_life(ts, data, "f32", "f32", "scan"),
    }


def test_handles_made_used_grown_viewed_and_destroyed_eight_times_answer_the_same(ts, data):
    first = one_cycle(ts, data)
    # an anchor outside the library: the ten best rows of the fp32 index's first search are numpy's
    c, q = data["f32"]["c"][:N].astype(np.float64), data["f32"]["q"].astype(np.float64)
    truth = (q / np.linalg.norm(q, axis=1, keepdims=True)) @ (c / np.linalg.norm(c, axis=1, keepdims=True)).T
    idx = first["f32"][1]
    assert idx.shape == (5, 10)
    for r in range(5):
        assert set(idx[r].tolist()) == set(np.argsort(-truth[r])[:10].tolist())
    for cycle in range(1, CYCLES):
        got = one_cycle(ts, data)
        for life, answers in first.items():
            assert len(got[life]) == len(answers)
            for j, (a, b) in enumerate(zip(got[life], answers)):
                assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), f"cycle {cycle}, {life}: answer {j} differs from the first cycle's"
