"""Reference of the staggered starts (scp_lag_conflicts, scp_schedule_starts), written from the rule in include/scp_hip.h (not
from the kernels): the pair-lag masks from the unpruned segment minima of tests/delay_ref.py, the greedy schedule in Python
integers, the staggered fleet from delay_ref.records.

  masks(...)              (N, N) Python-int lists -> uint64 array: bit s of mask[a][b] is set iff some global segment g < K + s of
                          lag s of (a, b) has sqrt(max(f, 0)) < R - 0.01;
  greedy(mask, S, order)  delays (list, -1: unplaced) and the stats of scp_start_schedule_stats;
  staggered(...)          the fleet of horizon K + Dmax in which v uses record clamp(g - d_v, -1, K);
  pair_conflicts(...)     does the ordered pair (a, b) conflict in the staggered fleet of two delays?  Every segment, by
                          separation_ref -- what the relative-lag statement is checked against;
  half_ring(...)          the end-to-end construction."""
import numpy as np

import delay_ref as dr
import separation_ref as sr


def masks_from_margins(ref, N, S):
    """the (N, N) uint64 masks of a delay_ref.margins result over all vehicles (its seg_f: every segment's f, +inf: none)"""
    out = np.zeros((N, N), dtype=np.uint64)
    thr = ref["thr"]
    for a, f in ref["seg_f"].items():  # f: (S + 1, K + S, N)
        viol = (np.sqrt(np.maximum(f, 0.0)) < thr).any(axis=1)  # (S + 1, N); +inf never violates
        for s in range(S + 1):
            out[a] |= viol[s].astype(np.uint64) << np.uint64(s)
    return out


def masks(pos, vel, acc, h, R, S):
    N = pos.shape[0]
    ref = dr.margins(pos, vel, acc, h, R, S)
    return masks_from_margins(ref, N, S), ref


def greedy(mask, S, order=None):
    """the rule of include/scp_hip.h in Python integers.  mask: (N, N) array-like of words -> (delays, stats)"""
    m = [[int(x) for x in row] for row in np.asarray(mask).tolist()]
    N = len(m)
    order = list(range(N)) if order is None else [int(v) for v in order]
    placed = []  # (u, d_u)
    delay = [None] * N
    first_unplaced = -1
    for v in order:
        found = -1
        for d in range(S + 1):
            ok = True
            for u, du in placed:
                bit = (m[v][u] >> (d - du)) & 1 if d >= du else (m[u][v] >> (du - d)) & 1
                if bit:
                    ok = False
                    break
            if ok:
                found = d
                break
        delay[v] = found
        if found >= 0:
            placed.append((v, found))
        elif first_unplaced < 0:
            first_unplaced = v
    good = [d for d in delay if d >= 0]
    stats = {"n_delayed": sum(d > 0 for d in good), "n_unplaced": N - len(good), "max_delay": max(good, default=0),
             "first_unplaced": first_unplaced, "total_delay": sum(good)}
    return delay, stats


def random_masks(N, S, density, seed, symmetric=True):
    """synthetic masks: every bit 0 .. S of every off-diagonal word set with probability `density`.  symmetric: bit 0 of
    mask[a][b] and mask[b][a] agree, as in every mask of trajectories; False: they do not, and a schedule shows whether it
    follows the rule to the letter (mask[v][u] for d >= d_u)"""
    rng = np.random.default_rng(seed)
    bits = rng.random((N, N, S + 1)) < density
    if symmetric:
        bits[:, :, 0] = np.triu(bits[:, :, 0], 1) | np.triu(bits[:, :, 0], 1).T
    m = np.zeros((N, N), dtype=np.uint64)
    for s in range(S + 1):
        m |= bits[:, :, s].astype(np.uint64) << np.uint64(s)
    m[np.arange(N), np.arange(N)] = 0
    return m


def satisfies(mask, delay):
    """every two PLACED vehicles keep to the masks"""
    m = np.asarray(mask).tolist()
    N = len(m)
    for a in range(N):
        for b in range(N):
            if a != b and delay[a] >= 0 and delay[b] >= 0 and delay[a] >= delay[b]:
                if (int(m[a][b]) >> (delay[a] - delay[b])) & 1:
                    return False
    return True


def staggered(pos, vel, acc, h, delays):
    """(P, V, A) of shape (N, K + Dmax, D) from delay_ref.records; an unplaced vehicle (-1) counts as 0"""
    N, K, D = pos.shape
    d = np.maximum(np.asarray(delays, dtype=np.int64), 0)
    H = K + int(d.max())
    rec = dr.records(pos, vel, acc, h)
    out = [np.empty((N, H, D)) for _ in range(3)]
    for v in range(N):
        idx = np.clip(np.arange(H) - d[v], -1, K) + 1
        for o, x in zip(out, rec):
            o[v] = x[v, idx]
    return tuple(out)


def pair_conflicts(pos, vel, acc, h, R, a, b, da, db):
    """does (a, b) have a violating segment in the fleet staggered by (da, db)?  -> (violates, smallest |sqrt(f) - thr| over
    the segments: how well the answer is determined)"""
    P, V, A = staggered(pos[[a, b]], vel[[a, b]], acc[[a, b]], h, [da, db])
    f, _ = sr.segment_minima(P[0] - P[1], V[0] - V[1], A[0] - A[1], h)
    dist = np.sqrt(np.maximum(f, 0.0))
    thr = R - 0.01
    return bool((dist < thr).any()), float(np.abs(dist - thr).min())


def half_ring(N, K, D, seed, h=0.2):
    """angle_i = pi (i + 0.25 u_i) / N, u uniform in [-1, 1); start on the circle of radius 5 around (10, 10), goal = start
    reflected through the centre; in 3-D z_start = 0.05 i and z_goal reversed; constant velocity, zero acceleration"""
    u = np.random.default_rng(seed).uniform(-1, 1, N)
    ang = np.pi * (np.arange(N) + 0.25 * u) / N
    start = np.zeros((N, D))
    goal = np.zeros((N, D))
    start[:, 0] = 10.0 + 5.0 * np.cos(ang)
    start[:, 1] = 10.0 + 5.0 * np.sin(ang)
    goal[:, 0] = 20.0 - start[:, 0]
    goal[:, 1] = 20.0 - start[:, 1]
    if D == 3:
        start[:, 2] = 0.05 * np.arange(N)
        goal[:, 2] = start[::-1, 2]
    v = (goal - start) / (K * h)
    t = h * np.arange(K)
    pos = start[:, None, :] + t[None, :, None] * v[:, None, :]
    vel = np.repeat(v[:, None, :], K, axis=1)
    return pos, vel, np.zeros_like(pos)
