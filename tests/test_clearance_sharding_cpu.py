"""Shard.all_argmin_arrays and the element-wise all_min / all_sum_int over gloo with two ranks (no GPU): the entry-wise merge
of the clearance profiles of two ranks is the lexicographic minimum of (min_dist, row) carrying t, the minimum and the integer
sum; with one rank they return their inputs."""
import os
import sys

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_ROW = np.uint64(2**64 - 1)


def parts():
    """two ranks' (min_dist, row, t, sample, n_violating): a smaller value on either rank, an exact tie decided by the row
    (rows beyond 2^63 included), an entry empty on one rank and one empty on both"""
    inf = np.inf
    a = (np.array([1.0, 3.0, 0.5, 0.5, inf, inf, 0.0]), np.array([7, 9, 4, 1 << 63, NO_ROW, NO_ROW, 5], dtype=np.uint64),
         np.array([0.1, 0.2, 0.01, 0.02, 0.0, 0.0, 0.0]), np.array([1.5, 3.0, 0.6, 0.5, inf, inf, 0.0]),
         np.array([0, 0, 2, 1, 0, 0, 3], dtype=np.uint64))
    b = (np.array([2.0, 2.5, 0.5, 0.5, 4.0, inf, 0.0]), np.array([1, 2, 3, (1 << 63) + 1, 6, NO_ROW, 8], dtype=np.uint64),
         np.array([0.15, 0.05, 0.03, 0.04, 0.07, 0.0, 0.0]), np.array([2.0, 2.5, 0.7, 0.4, 4.0, inf, 0.0]),
         np.array([0, 1, 1, 1, 0, 0, 4], dtype=np.uint64))
    want = (np.array([1.0, 2.5, 0.5, 0.5, 4.0, inf, 0.0]), np.array([7, 2, 3, 1 << 63, 6, NO_ROW, 5], dtype=np.uint64),
            np.array([0.1, 0.05, 0.03, 0.02, 0.07, 0.0, 0.0]), np.array([1.5, 2.5, 0.6, 0.4, 4.0, inf, 0.0]),
            np.array([0, 1, 3, 2, 0, 0, 7], dtype=np.uint64))
    return a, b, want


def _worker(rank, world, port):
    sys.path.insert(0, os.path.join(ROOT, "ba-path-planning_amd"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from path_planning._sharding import Shard

    sh = Shard(10, rank, world)
    a, b, want = parts()
    mine = (a, b)[rank]
    m, row, t = sh.all_argmin_arrays(mine[0], mine[1], mine[2])
    assert row.dtype == np.uint64 and m.tobytes() == want[0].tobytes() and row.tobytes() == want[1].tobytes()
    assert t.tobytes() == want[2].tobytes()
    assert sh.all_min(mine[3]).tobytes() == want[3].tobytes()
    total = sh.all_sum_int(mine[4])
    assert total.dtype == np.uint64 and total.tobytes() == want[4].tobytes()
    # the scalar forms are what they were
    assert sh.all_min(float(rank)) == 0.0 and sh.all_sum_int(rank + 1) == 3 and sh.all_argmin(1.0, 5 - rank, float(rank)) == (1.0, 4, 1.0)
    dist.destroy_process_group()


def test_array_reductions_two_ranks():
    port = 32500 + (os.getpid() * 7) % 1000
    mp.spawn(_worker, args=(2, port), nprocs=2, join=True)


def test_array_reductions_one_rank_are_the_identity():
    from path_planning._sharding import Shard

    a, _, _ = parts()
    sh = Shard(4)
    m, row, t = sh.all_argmin_arrays(a[0], a[1], a[2])
    assert m is a[0] and row is a[1] and t is a[2]
    assert sh.all_min(a[3]) is a[3] and sh.all_sum_int(a[4]) is a[4]
    assert sh.all_min(2.5) == 2.5 and sh.all_sum_int(3) == 3
