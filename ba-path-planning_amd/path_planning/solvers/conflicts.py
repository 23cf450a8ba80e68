"""Conflict windows: the per-segment records of scp_list_conflicts (one per violating segment, include/scp_hip.h) merged
into one entry per pair and contiguous stretch of time.  Pure numpy, runs on the host: the records are a tiny fraction of the
K N (N - 1) / 2 segments the device pass has looked at."""
import numpy as np


def pairs_from_index(q, N):
    """Lexicographic pair indices (array) -> (i, j), i < j, in exact integer arithmetic"""
    q = np.asarray(q, dtype=np.int64)
    off = lambda a: a * (2 * N - a - 1) // 2  # noqa: E731
    i = (((2 * N - 1) - np.sqrt(((2 * N - 1) ** 2 - 8 * q).astype(np.float64))) // 2).astype(np.int64)
    i = np.clip(i, 0, max(N - 2, 0))
    while (off(i) > q).any():  # the square root is off by at most one
        i = np.where(off(i) > q, i - 1, i)
    while ((i < N - 2) & (off(i + 1) <= q)).any():
        i = np.where((i < N - 2) & (off(i + 1) <= q), i + 1, i)
    return i, q - off(i) + i + 1


def pair_from_index(q, N):
    """Lexicographic pair index -> (i, j), i < j (host helper, exact integer arithmetic)."""
    i, j = pairs_from_index(q, N)
    return int(i), int(j)


def conflict_windows(records, N, K, h):
    """records: structured array with the fields of scp_conflict (row = k * pairs + q, min_dist, t_min, t_enter, t_exit,
    pieces), any order.  Returns one dict per window, sorted by (t_start, i, j):

        {"vehicles": (i, j), "t_start", "t_end", "duration", "min_distance", "t_min_distance", "first_timestep",
         "n_segments", "pieces"}

    Times are absolute (k h + t).  Segments k and k + 1 of a pair form one window when the first ends inside the conflict
    (t_exit == h) and the second starts inside it (t_enter == 0): exact comparisons, these are the values the kernel
    writes for the two cases.  A segment that dips below the threshold twice (pieces == 2) contributes the hull
    [t_enter, t_exit]; a window's ``pieces`` is the number of separate stretches below the threshold inside it, so
    pieces > 1 says that [t_start, t_end] is a hull."""
    records = np.asarray(records)
    if records.size == 0:
        return []
    pairs = N * (N - 1) // 2
    row = records["row"].astype(np.int64)
    k, q = row // pairs, row % pairs
    if (k >= K).any():
        raise ValueError(f"conflict_windows: row {int(row.max())} outside K = {K} time steps of {pairs} pairs")
    order = np.lexsort((k, q))
    rec, k, q = records[order], k[order], q[order]
    # a record opens a window unless it continues the previous one
    cont = np.zeros(rec.size, dtype=bool)
    cont[1:] = ((q[1:] == q[:-1]) & (k[1:] == k[:-1] + 1) & (rec["t_exit"][:-1] == h) & (rec["t_enter"][1:] == 0.0))
    starts = np.nonzero(~cont)[0]
    ends = np.append(starts[1:], rec.size)
    vi, vj = pairs_from_index(q[starts], N)
    out = []
    for s, e, i, j in zip(starts, ends, vi, vj):
        m = s + int(np.argmin(rec["min_dist"][s:e]))  # the first of equal minima
        t0 = float(k[s] * h + rec["t_enter"][s])
        t1 = float(k[e - 1] * h + rec["t_exit"][e - 1])
        out.append({"vehicles": (int(i), int(j)), "t_start": t0, "t_end": t1, "duration": t1 - t0,
                    "min_distance": float(rec["min_dist"][m]), "t_min_distance": float(k[m] * h + rec["t_min"][m]),
                    "first_timestep": int(k[s]), "n_segments": int(e - s),
                    "pieces": int(rec["pieces"][s:e].astype(np.int64).sum() - (e - s - 1))})
    out.sort(key=lambda w: (w["t_start"],) + w["vehicles"])
    return out
