"""numpy reference of the delay margins (scp_delay_margins), written from the definition in include/scp_hip.h (not from the
kernel): every vehicle has K + 2 records r = -1 .. K -- held at the start (p[0], 0, 0), the stored segments, parked at the goal
(pK, 0, 0) --; with vehicle a ALONE started s steps late the global segment g = 0 .. K+s-1 compares record g - s of a (-1 while
g < s) with record min(g, K) of every b != a.  The quartic of a segment is minimised by tests/separation_ref.py on EVERY segment
-- no pruning --, and entry (a, s) is the lexicographic minimum of (f, g, b).

margins() returns parallel arrays of shape (vehicles, S + 1): f (the smallest minimum of the quartic, not clamped, not rooted;
+inf: no pair), g, b (-1: none), t, second_f (the entry's second-smallest f: how well (g, b) is determined), n_violating
(sqrt(max(f, 0)) < R - 0.01), plus s_max (the largest |d| + h |w| + h^2/2 |b| over the segments), thr and seg_f: per vehicle an
array (S + 1, K + S, N) of every segment's f (+inf where there is no segment: b = a, g >= K + s)."""
import numpy as np

import separation_ref as sr


def parked(pos, vel, acc, h):
    """pK = p[K-1] + (h v[K-1] + (h^2/2) a[K-1]): every product and every sum rounded on its own"""
    return pos[:, -1] + (h * vel[:, -1] + (0.5 * h * h) * acc[:, -1])


def records(pos, vel, acc, h):
    """(P, V, A), each (N, K + 2, D): index r + 1 holds record r = -1 .. K"""
    z = np.zeros_like(pos[:, :1])
    P = np.concatenate([pos[:, :1], pos, parked(pos, vel, acc, h)[:, None]], axis=1)
    return P, np.concatenate([z, vel, z], axis=1), np.concatenate([z, acc, z], axis=1)


def shifted_fleet(pos, vel, acc, h, a, s):
    """the fleet of horizon K + s in which vehicle a has s held records followed by its plan and everybody else the plan
    followed by s parked records: an ordinary input of the clearance profile"""
    N, K, D = pos.shape
    P, V, A = records(pos, vel, acc, h)
    idx = np.minimum(np.arange(K + s), K) + 1               # everybody: record min(g, K)
    out = [x[:, idx].copy() for x in (P, V, A)]
    mine = np.maximum(np.arange(K + s) - s, -1) + 1         # a: record g - s, -1 while g < s
    for o, x in zip(out, (P, V, A)):
        o[a] = x[a, mine]
    return tuple(out)


def margins(pos, vel, acc, h, R, max_lag, a_begin=0, a_end=None):
    N, K, D = pos.shape
    S = max_lag
    a_end = N if a_end is None else a_end
    n_a = a_end - a_begin
    P, V, A = records(pos, vel, acc, h)
    thr = R - 0.01
    out = {"f": np.full((n_a, S + 1), np.inf), "g": np.full((n_a, S + 1), -1, dtype=np.int64),
           "b": np.full((n_a, S + 1), -1, dtype=np.int64), "t": np.zeros((n_a, S + 1)),
           "second_f": np.full((n_a, S + 1), np.inf), "n_violating": np.zeros((n_a, S + 1), dtype=np.int64),
           "s_max": 0.0, "thr": thr, "seg_f": {}}
    if N < 2:
        return out
    lag, seg = np.meshgrid(np.arange(S + 1), np.arange(K + S), indexing="ij")  # (S + 1, K + S)
    live = seg < K + lag
    ra = np.minimum(np.maximum(seg - lag, -1), K) + 1  # (beyond K + s: no segment, masked below)
    rb = np.minimum(seg, K) + 1
    for a in range(a_begin, a_end):
        others = np.delete(np.arange(N), a)
        # (S + 1, K + S, N - 1, D): record of a minus record of b -- g-major, then b ascending, the order of the ties
        dif = lambda X: X[a][ra][:, :, None, :] - X[others][:, rb].transpose(1, 2, 0, 3)  # noqa: E731
        d, w, b = dif(P), dif(V), dif(A)
        m = np.broadcast_to(live[:, :, None], d.shape[:3])
        f = np.full(d.shape[:3], np.inf)
        t = np.zeros(d.shape[:3])
        f[m], t[m] = sr.segment_minima(d[m], w[m], b[m], h)
        out["s_max"] = max(out["s_max"], float(sr.s_bound(d[m], w[m], b[m], h).max()))
        flat = f.reshape(S + 1, -1)
        order = np.argsort(flat, axis=1, kind="stable")  # stable: equal f keep the (g, b) order
        first = order[:, 0]
        e = a - a_begin
        rows = np.arange(S + 1)
        out["f"][e] = flat[rows, first]
        out["g"][e], bi = np.divmod(first, N - 1)
        out["b"][e] = others[bi]
        out["t"][e] = t.reshape(S + 1, -1)[rows, first]
        if flat.shape[1] > 1:
            out["second_f"][e] = flat[rows, order[:, 1]]
        out["n_violating"][e] = (m & (np.sqrt(np.maximum(f, 0.0)) < thr)).sum(axis=(1, 2))
        full = np.full((S + 1, K + S, N), np.inf)
        full[:, :, others] = f
        out["seg_f"][a] = full
    return out


# ---- the crossing case -----------------------------------------------------------------------------------------------------------
CROSS_H, CROSS_K, CROSS_R = 0.2, 12, 0.5


def crossing_case(N, D, pair):
    """Vehicle pair[0] flies p = (2 (t - 0.8), 0), vehicle pair[1] p = (0, 2 (t - 1.4)), both at constant velocity: they cross
    the origin 0.6 s = 3 steps apart, so the margin of pair[0] at lag s is 0.2 sqrt(2) |3 - s| (0 at s = 3) and its tolerance
    one step (R - 0.01 = 0.49: 0.566 at lag 1, 0.283 at lag 2).  Everybody else is at rest, 10 m apart and away from the two.
    -> pos, vel, acc (h = 0.2, K = 12; R = 0.5)"""
    K, h = CROSS_K, CROSS_H
    pos = np.zeros((N, K, D))
    vel = np.zeros((N, K, D))
    acc = np.zeros((N, K, D))
    pos[:, :, 0] = 10.0 * (1 + np.arange(N))[:, None]
    pos[:, :, D - 1] += 10.0
    t = h * np.arange(K)
    a, b = pair
    pos[a] = 0.0
    pos[b] = 0.0
    pos[a, :, 0] = 2.0 * (t - 0.8)
    pos[b, :, 1] = 2.0 * (t - 1.4)
    vel[a, :, 0] = 2.0
    vel[b, :, 1] = 2.0
    return pos, vel, acc


def crossing_margin(s):
    return 0.2 * np.sqrt(2.0) * abs(3 - s)
