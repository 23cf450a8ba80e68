"""Staggered starts on the host: the fleet in which vehicle v starts delays[v] steps late.  Pure numpy; the device part (pair-lag
masks, greedy schedule) is scp_lag_conflicts / scp_schedule_starts (include/scp_hip.h)."""
import numpy as np


def staggered_fleet(pos, vel, acc, h, delays):
    """pos, vel, acc: (N, K, D) stored trajectories; delays: N whole numbers of steps (-1, an unplaced vehicle, counts as 0).
    Returns (pos, vel, acc) of shape (N, K + Dmax, D), Dmax the largest delay: in segment g vehicle v uses its record
    clamp(g - delays[v], -1, K) -- held at the start (p[0], 0, 0) before it leaves, parked at the goal (pK, 0, 0) after it has
    arrived, pK = p[K-1] + (h v[K-1] + (h^2/2) a[K-1]) with every product and every sum rounded on its own: the bits of the
    device records (scp_delay_margins), so the result is an ordinary input of scp_check_separation and scp_list_conflicts."""
    pos, vel, acc = (np.asarray(x, dtype=np.float64) for x in (pos, vel, acc))
    N, K, D = pos.shape
    d = np.maximum(np.asarray(delays, dtype=np.int64).reshape(N), 0)
    horizon = K + (int(d.max()) if N else 0)
    z = np.zeros_like(pos[:, :1])
    parked = pos[:, -1] + (h * vel[:, -1] + (0.5 * h * h) * acc[:, -1])
    P = np.concatenate([pos[:, :1], pos, parked[:, None]], axis=1)  # index r + 1 holds record r = -1 .. K
    V = np.concatenate([z, vel, z], axis=1)
    A = np.concatenate([z, acc, z], axis=1)
    idx = np.clip(np.arange(horizon)[None, :] - d[:, None], -1, K) + 1  # (N, horizon)
    take = lambda X: np.ascontiguousarray(np.take_along_axis(X, idx[:, :, None], axis=1))  # noqa: E731
    return take(P), take(V), take(A)


def delays_satisfy_masks(mask, delays):
    """Do the placed vehicles (delay >= 0) of a schedule keep to the (N, N) uint64 pair-lag masks?  For every ordered pair
    with d_a >= d_b bit d_a - d_b of mask[a][b] must be clear."""
    mask = np.asarray(mask, dtype=np.uint64)
    d = np.asarray(delays, dtype=np.int64)
    a, b = np.nonzero((d[:, None] >= d[None, :]) & (d[:, None] >= 0) & (d[None, :] >= 0) & ~np.eye(d.size, dtype=bool))
    lag = (d[a] - d[b]).astype(np.uint64)
    return not ((mask[a, b] >> lag) & np.uint64(1)).any()


def schedule_key(n_unplaced, max_delay, total_delay, objective):
    """the key of scp_schedule_starts_batch without its trailing candidate index, as a tuple of Python integers"""
    u, m, t = int(n_unplaced), int(max_delay), int(total_delay)
    return (u, m, t) if objective == "makespan" else (u, t, m)


def candidate_orders(N, B, rng, base=None):
    """(B, N) int32 candidate orders of a first search round: row 0 is `base` (None: 0 .. N-1), row 1 its reverse, every further
    row rng.permutation(N), drawn in sequence -- deterministic for a given numpy.random.Generator."""
    base = np.arange(N, dtype=np.int32) if base is None else np.asarray(base, dtype=np.int32).reshape(N)
    out = np.empty((B, N), dtype=np.int32)
    out[0] = base
    if B >= 2:
        out[1] = base[::-1]
    for b in range(2, B):
        out[b] = rng.permutation(N)
    return out


def refined_orders(best_order, delays, B, rng):
    """(B, N) int32 candidate orders derived from the best order so far and its delays (-1: unplaced); pos: the position of a
    vehicle in best_order.  Row 0: best_order; row 1: the unplaced vehicles by pos, then the placed ones by pos; row 2: the
    unplaced by pos, then the placed by ascending delay (ties by pos); row 3: the placed by descending delay (ties by pos), then
    the unplaced by pos; every further row: best_order after max(1, N // 16) transpositions of the positions
    rng.integers(0, N, 2), drawn in sequence.  B < 4: the first B rows."""
    best = np.asarray(best_order, dtype=np.int32).reshape(-1)
    N = best.size
    d = np.asarray(delays, dtype=np.int64).reshape(N)[best]  # by position
    pos = np.arange(N)
    unplaced, placed = pos[d < 0], pos[d >= 0]
    rows = [pos,
            np.concatenate([unplaced, placed]),
            np.concatenate([unplaced, placed[np.argsort(d[placed], kind="stable")]]),
            np.concatenate([placed[np.argsort(-d[placed], kind="stable")], unplaced])]
    out = np.empty((B, N), dtype=np.int32)
    for b in range(min(B, 4)):
        out[b] = best[rows[b]]
    for b in range(4, B):
        row = best.copy()
        for _ in range(max(1, N // 16)):
            i, j = (int(x) for x in rng.integers(0, N, 2))
            row[i], row[j] = row[j], row[i]
        out[b] = row
    return out
