"""numpy reference of the holds (scp_update_holds, scp_apply_holds), written from the rule in include/scp_hip.h: every product
and every sum is one numpy operation on float64 scalars (numpy never contracts), coordinates in ascending order, so a kernel
that follows the stated order reproduces these bits.

A table is a structured array (HOLD_DTYPE: row, eta[3], margin, reserved) sorted by row with unique rows; conflicts are a
structured array with at least the fields row, min_dist, t_min in ascending row order (what scp_list_conflicts returns)."""
import numpy as np

HOLD_DTYPE = np.dtype([("row", np.uint64), ("eta", np.float64, (3,)), ("margin", np.float64), ("reserved", np.uint64)])
EPS = np.finfo(np.float64).eps


def pair_indices(N):
    i, j = np.triu_indices(N, 1)
    return i.astype(np.int64), j.astype(np.int64)


def empty_table():
    return np.zeros(0, dtype=HOLD_DTYPE)


def direction(dp, dv, da, t):
    """the unit vector a conflict proposes: (dm / |dm|) at the closest approach, or the perpendicular of the relative velocity
    where the vehicles meet -> eta (3,), eta[2] = 0 in 2-D"""
    D = len(dp)
    f = np.float64
    t = f(t)
    ht = f(0.5) * t
    dm, w = [], []
    nn, ww = f(0.0), f(0.0)
    for d in range(D):
        tv = t * f(dv[d])
        ta = (ht * t) * f(da[d])
        dm.append(f(dp[d]) + (tv + ta))
        w.append(f(dv[d]) + t * f(da[d]))
        nn = nn + dm[d] * dm[d]
        ww = ww + w[d] * w[d]
    n, wn = np.sqrt(nn), np.sqrt(ww)
    eta = np.zeros(3)
    if n >= 1e-6:
        for d in range(D):
            eta[d] = dm[d] / n
    elif wn < 1e-12:
        eta[0] = 1.0
    elif D == 2:
        eta[0], eta[1] = -w[1] / wn, w[0] / wn
    else:
        m = 0
        for d in (1, 2):
            if abs(w[d]) < abs(w[m]):
                m = d
        x = [(f(0.0), w[2], -w[1]), (-w[2], f(0.0), w[0]), (w[1], -w[0], f(0.0))][m]  # w x e_m
        xx = f(0.0)
        for d in range(3):
            xx = xx + x[d] * x[d]
        xn = np.sqrt(xx)
        for d in range(3):
            eta[d] = x[d] / xn
    return eta


def candidates(pos, vel, acc, R, conflicts, pad, q_begin=0, q_end=None):
    """row -> (eta, s) of the winning proposal: the largest shortfall, ties to the proposal of the smaller conflict row"""
    N, K, D = pos.shape
    i, j = pair_indices(N)
    pairs = i.size
    q_end = pairs if q_end is None else q_end
    best = {}
    for c in conflicts:  # ascending conflict rows: a later proposal replaces an earlier one only with a LARGER shortfall
        row = int(c["row"])
        k, q = divmod(row, pairs)
        if not q_begin <= q < q_end:
            continue
        a, b = i[q], j[q]
        eta = direction(pos[a, k] - pos[b, k], vel[a, k] - vel[b, k], acc[a, k] - acc[b, k], c["t_min"])
        s = (np.float64(R) - np.float64(c["min_dist"])) + np.float64(pad)
        for r in ([row, row + pairs] if k + 1 < K else [row]):
            if r not in best or s > best[r][1]:
                best[r] = (eta, s)
    return best


def update(table, pos, vel, acc, R, conflicts, pad, q_begin=0, q_end=None):
    """the table after one pass: a held row takes the new direction and margin old + s, a new row enters with margin s"""
    best = candidates(pos, vel, acc, R, conflicts, pad, q_begin, q_end)
    rows = {int(t["row"]): (t["eta"].copy(), np.float64(t["margin"])) for t in table}
    for r, (eta, s) in best.items():
        rows[r] = (eta, rows[r][1] + s) if r in rows else (eta, s)
    out = np.zeros(len(rows), dtype=HOLD_DTYPE)
    for n, r in enumerate(sorted(rows)):
        out[n]["row"], out[n]["eta"], out[n]["margin"] = r, rows[r][0], rows[r][1]
    return out


def hold_bound(hold, N, D, h, R, p0, v0):
    """l_r = (R + c) - eta . ((p0_i - p0_j) + (k h)(v0_i - v0_j))"""
    i, j = pair_indices(N)
    k, q = divmod(int(hold["row"]), i.size)
    f = np.float64
    kh = f(k) * f(h)
    dot = f(0.0)
    for d in range(D):
        c = (f(p0[i[q], d]) - f(p0[j[q], d])) + kh * (f(v0[i[q], d]) - f(v0[j[q], d]))
        dot = dot + f(hold["eta"][d]) * c
    return (f(R) + f(hold["margin"])) - dot


def apply(table, N, K, D, h, R, p0, v0, eta_rows, l_rows, bitmap, q_begin=0, q_end=None):
    """eta_rows (K * nq, D), l_rows (K * nq,) and bitmap (uint32 words over the local rows) with the holds of the pair range
    written over them -> (eta_rows, l_rows, bitmap, new_rows): copies; new_rows = the global ids whose bit was clear, ascending"""
    pairs = N * (N - 1) // 2
    q_end = pairs if q_end is None else q_end
    nq = q_end - q_begin
    eta_rows, l_rows, bitmap = eta_rows.copy(), l_rows.copy(), bitmap.copy()
    new_rows = []
    for t in table:
        k, q = divmod(int(t["row"]), pairs)
        if not q_begin <= q < q_end:
            continue
        lr = k * nq + (q - q_begin)
        eta_rows[lr] = t["eta"][:D]
        l_rows[lr] = hold_bound(t, N, D, h, R, p0, v0)
        if not (int(bitmap[lr >> 5]) >> (lr & 31)) & 1:
            new_rows.append(int(t["row"]))
        bitmap[lr >> 5] |= np.uint32(1 << (lr & 31))
    return eta_rows, l_rows, bitmap, np.asarray(new_rows, dtype=np.int64)


def held_minimum(eta, d, w, b, h):
    """min over t in [0, h] of eta . (d + t w + t^2/2 b): the quadratic's value at 0, at h and at its vertex if inside"""
    a0, a1, a2 = float(eta @ d), float(eta @ w), 0.5 * float(eta @ b)
    g = lambda t: a0 + t * (a1 + t * a2)  # noqa: E731
    cand = [g(0.0), g(h)]
    if a2 > 0.0:
        tv = -a1 / (2.0 * a2)
        if 0.0 < tv < h:
            cand.append(g(tv))
    return min(cand)


# ---- the repair loop on the CPU oracle (tests/test_holds_cpu.py) -----------------------------------------------------------
def ring_scenario(N, rad, seed, random_angles=False):
    """start / goal positions of the issue's scenarios around the centre (10, 10)"""
    rng = np.random.default_rng(seed)
    if random_angles:
        ang = np.sort(rng.uniform(0, 2 * np.pi, N))
    else:
        ang = 2 * np.pi * np.arange(N) / N + rng.uniform(-0.1, 0.1, N)
    p0 = 10 + rad * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    pf = 10 - rad * np.stack([np.cos(ang + 0.3), np.sin(ang + 0.3)], axis=1)
    return p0, pf
