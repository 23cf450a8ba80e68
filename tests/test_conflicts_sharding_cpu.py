"""Shard.allgather_records over gloo with two ranks (no GPU): every rank's variable-length array of scp_conflict records,
merged by row, is the sorted concatenation -- also when a list outgrows the agreed message capacity, and when a rank has
nothing; with one rank it is the identity."""
import os
import sys

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def records(n, seed, rows):
    from path_planning import _hip

    rng = np.random.default_rng(seed)
    out = np.zeros(n, dtype=_hip.CONFLICT_DTYPE)
    out["row"] = rows
    for f in ("min_dist", "t_min", "t_enter", "t_exit"):
        out[f] = rng.uniform(0.0, 1.0, n)
    out["min_dist"][: n // 2] *= -1.0  # sign bits and NaN payloads travel as bytes
    if n:
        out["t_min"][0] = np.nan
    out["pieces"] = rng.integers(1, 3, n)
    return out


def _worker(rank, world, port):
    sys.path.insert(0, os.path.join(ROOT, "ba-path-planning_amd"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from path_planning._sharding import Shard

    sh = Shard(10, rank, world)
    # disjoint, interleaved rows beyond 2^32; rank 0 has 5 records, rank 1 has 1500 (more than the default capacity)
    parts = [records(5, 1, (1 << 40) + 7 * np.arange(5)), records(1500, 2, 3 + 11 * np.arange(1500))]
    want = np.concatenate(parts)
    want = want[np.argsort(want["row"], kind="stable")]
    got = sh.allgather_records(parts[rank])
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert sh._records_cap >= 1500 * 6
    assert sh.allgather_records(parts[rank]).tobytes() == want.tobytes()  # the grown capacity: one collective
    # one rank with an empty list, then both
    got = sh.allgather_records(parts[0][: 0 if rank == 0 else 3])
    assert got.tobytes() == parts[0][:3].tobytes()
    assert sh.allgather_records(parts[0][:0]).size == 0
    # the ids exchange still works beside it (they share the message code)
    import torch

    ids, mx = sh.allgather_ids(torch.tensor([4 + rank, 10 + rank]), extra=float(rank))
    assert ids.tolist() == [4, 5, 10, 11] and mx == 1.0
    dist.destroy_process_group()


def test_allgather_records_two_ranks():
    port = 31500 + (os.getpid() * 7) % 1000
    mp.spawn(_worker, args=(2, port), nprocs=2, join=True)


def test_allgather_records_one_rank_is_the_identity():
    from path_planning._sharding import Shard

    a = records(4, 3, [9, 2, 5, 1])  # not even sorted: returned as it is
    assert Shard(4).allgather_records(a) is a
