"""The multi-rank cut of the delay margins over gloo with two ranks (no GPU): every rank computes the entries of its own
vehicles (Shard.agent_range) and solvers.scp.gather_delay_blocks concatenates the blocks in vehicle order, byte for byte --
nothing is merged; with one rank it returns its input."""
import os
import sys

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, S = 5, 2


def full():
    """N x (S + 1) entries with distinct bits in every field: an empty entry, a negative zero, huge counts"""
    from path_planning import _hip

    e = np.zeros((N, S + 1), dtype=_hip.DELAY_DTYPE)
    k = np.arange(N * (S + 1)).reshape(N, S + 1)
    e["min_dist"] = 0.25 + k / 7.0
    e["t_min"] = k / 90.0
    e["partner"] = (k * 3 + 1) % N
    e["segment"] = k % 11
    e["n_violating"] = k * (1 << 40)
    e[3, 1] = (np.inf, 0.0, _hip.NO_INDEX, _hip.NO_INDEX, 0)
    e["t_min"][4, 2] = -0.0
    return e


def _worker(rank, world, port):
    sys.path.insert(0, os.path.join(ROOT, "ba-path-planning_amd"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from path_planning import _hip
    from path_planning._sharding import Shard
    from path_planning.solvers.scp import gather_delay_blocks

    sh = Shard(N, rank, world)
    a0, a1 = sh.agent_range()
    assert (a0, a1) == ((0, 2), (2, 5))[rank]
    want = full()
    got = gather_delay_blocks(sh, np.ascontiguousarray(want[a0:a1]), a0)
    assert got.shape == (N * (S + 1),)
    for f in _hip.DELAY_DTYPE.names:
        assert np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(want.reshape(-1)[f]).tobytes(), f
    dist.destroy_process_group()


def test_blocks_of_two_ranks_concatenate():
    port = 33500 + (os.getpid() * 7) % 1000
    mp.spawn(_worker, args=(2, port), nprocs=2, join=True)


def test_one_rank_is_the_identity():
    from path_planning import _hip
    from path_planning._sharding import Shard
    from path_planning.solvers.scp import gather_delay_blocks

    want = full()
    got = gather_delay_blocks(Shard(N, 0, 1), want, 0)
    for f in _hip.DELAY_DTYPE.names:
        assert np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(want.reshape(-1)[f]).tobytes(), f
