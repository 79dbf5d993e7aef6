"""ShardedSearcher.rank_many on the CPU: two gloo ranks run the protocol (local rank_many for the owned targets, all-reduce
max of the scores, count_above_many for the others, all-reduce sum) with oracle-backed stand-ins for the two index calls,
on the fp32-cast truth.  What is tested is that the plumbing returns the whole-corpus ranks and scores for ragged lists."""
import datetime
import os
import socket

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import oracle


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_many_worker(rank, world, port, n, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        from theoremsearch_amd.distributed import ShardedSearcher, shard_bounds
        nq = 7
        q, c = oracle.golden_inputs(n, nq, 64, 321, "ip")
        c[5] = c[n - 2]                     # an exact tie across the two shards: the lower global id ranks first
        lo, hi = shard_bounds(n, world, rank)
        s32 = oracle.scores_fp64(q, c).astype(np.float32)      # the "kernel" scores of this stand-in
        calls = {"rank": 0, "count": 0}

        def local_rank_many(queries, targets):
            calls["rank"] += 1
            assert len(targets) == nq and np.array_equal(queries, q)
            ranks, scores = [], []
            for i, t in enumerate(targets):
                r = np.full(len(t), -1, np.int64)
                s = np.full(len(t), np.nan, np.float32)
                for j, row in enumerate(t):
                    if lo <= row < hi:
                        r[j] = oracle.rank_of(s32[i:i + 1, lo:hi], [row - lo])[0]
                        s[j] = s32[i, row]
                ranks.append(r)
                scores.append(s)
            return ranks, scores

        def local_count_above_many(queries, sc, ids):
            calls["count"] += 1
            assert len(sc) == nq and len(ids) == nq and np.array_equal(queries, q)
            out = []
            gids = np.arange(lo, hi)
            for i in range(nq):
                assert len(sc[i]) == len(ids[i])
                loc = s32[i, lo:hi]
                for gid in ids[i]:
                    assert not (lo <= gid < hi), "an owned target was sent to the counting call"
                out.append(np.array([int(np.sum((loc > t) | ((loc == t) & (gids < gid)))) for t, gid in zip(sc[i], ids[i])], np.int64))
            return out

        searcher = ShardedSearcher(lambda *_: None)
        rng = np.random.default_rng(5)
        targets = [[0, n - 1, 5, n - 2, n // 2, n // 2 - 1, n + 3],         # both sides of the cut, the tie, a row outside
                   [],                                                      # an empty list
                   [5, 5, n - 2, 5],                                        # a repeat
                   [int(x) for x in rng.integers(0, n, 41)],                # longer than a pass of 16
                   [n - 2], [n + 3, -1], [int(x) for x in rng.integers(0, n, 17)] + [n]]
        ranks, scores = searcher.rank_many(q, targets, local_rank_many=local_rank_many, local_count_above_many=local_count_above_many)
        ok = len(ranks) == nq and len(scores) == nq and calls == {"rank": 1, "count": 1}
        for i, t in enumerate(targets):
            t = np.asarray(t, dtype=np.int64)
            want = oracle.rank_of(s32[[i] * len(t)], t) if len(t) else np.zeros(0, np.int64)
            inside = (t >= 0) & (t < n)
            want_s = np.where(inside, s32[i, np.clip(t, 0, n - 1)], np.nan).astype(np.float32)
            ok = ok and ranks[i].dtype == np.int64 and scores[i].dtype == np.float32
            ok = ok and np.array_equal(ranks[i], want) and np.array_equal(scores[i], want_s, equal_nan=True)
            ok = ok and bool((ranks[i][~inside] == -1).all())
        # the planted tie: equal scores, the lower global id first, right behind each other
        ok = ok and scores[0][2] == scores[0][3] and ranks[0][3] == ranks[0][2] + 1
        # no targets at all: nothing is exchanged, empty lists come back
        r0, s0 = searcher.rank_many(q, [[] for _ in range(nq)], local_rank_many=local_rank_many, local_count_above_many=local_count_above_many)
        ok = ok and [len(x) for x in r0] == [0] * nq and [len(x) for x in s0] == [0] * nq
        ret[rank] = bool(ok)
    finally:
        dist.destroy_process_group()


def test_sharded_rank_many_two_gloo_ranks():
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_rank_many_worker, args=(world, _free_port(), 501, ret), nprocs=world, join=True)
    assert dict(ret) == {0: True, 1: True}
