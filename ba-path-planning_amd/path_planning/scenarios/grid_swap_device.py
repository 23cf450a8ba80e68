"""The grid-swap-device scenario family: grid-swap scenarios generated in batches on the GPU (scp_generate_grid_swap).

Same geometry and acceptance rules as ``generate_grid_swap`` -- jittered grid starts, goals permuted inside blocks of
``block`` x ``block`` cells, a block redrawn (256 candidates per round) until its straight-line motions keep ``min_sep``,
cross-block sweeps -- but the random draws come from a counter-based hash (include/scp_hip.h states the algorithm), so a
scenario depends only on its seed and the parameters, never on the batch it was generated in.  It is a family of its own,
not a copy of ``generate_grid_swap``'s numpy stream.  There is no CPU path: without a GPU these functions raise
``_hip.HipError`` like ``SCP``.
"""
import threading

import numpy as np

from .. import _hip

_CONTEXTS = {}
_LOCK = threading.Lock()


def _context(device):
    """one context per (device, current stream) and thread, kept for the process (a context costs a few allocations)"""
    import torch

    if not torch.cuda.is_available():
        raise _hip.HipError(-101, "no GPU visible: grid-swap-device scenarios are generated on the GPU only")
    dev = 0 if device is None else int(device)
    key = (dev, torch.cuda.current_stream(dev).cuda_stream, threading.get_ident())
    with _LOCK:
        ctx = _CONTEXTS.get(key)
        if ctx is None:
            ctx = _CONTEXTS[key] = _hip.Context(dev)
    return ctx


def generate_grid_swap_batch(n_agents, seeds, dim=2, device=0, **params):
    """B = len(seeds) scenarios of ``n_agents`` agents in one call.

    params: pitch (2.0), jitter (0.2), block (4), layer_gap (2.0), min_sep (0.3), max_tries (8192), sweeps (20).
    Returns (init, goal, space, stats): device tensors init (B, N, dim), goal (B, N, dim), space (B, 2 dim) = [lo..., hi...],
    and a dict of numpy arrays of length B: ``sweeps`` (redraw sweeps used), ``unmet_blocks`` (blocks without an
    acceptable candidate), ``conflicts`` (cross-block pairs left closer than min_sep), ``min_approach`` (closest
    straight-line approach over all pairs) and ``ok`` (min_approach >= min_sep)."""
    ctx = _context(device)
    init, goal, space, st = ctx.generate_grid_swap(int(n_agents), int(dim), seeds, _hip.gen_params(**params))
    stats = {k: st[k].copy() for k in ("sweeps", "unmet_blocks", "conflicts", "min_approach")}
    stats["ok"] = st["ok"].astype(bool)
    return init, goal, space, stats


def generate_grid_swap_device(n_agents, seed=0, dim=2, device=0, **params):
    """One scenario with ``generate_grid_swap``'s signature: (initial (N, dim), final (N, dim), space_dims) as numpy."""
    init, goal, space, _ = generate_grid_swap_batch(n_agents, [0 if seed is None else seed], dim=dim, device=device,
                                                    **params)
    return init[0].cpu().numpy(), goal[0].cpu().numpy(), [float(v) for v in space[0].cpu().numpy()]
