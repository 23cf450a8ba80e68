"""numpy reference of the continuous-time separation check, written from the kinematics alone (not from the kernel).

Over segment k vehicle i flies p_i[k] + t v_i[k] + t^2/2 a_i[k], t in [0, h].  For a pair, d = p_i - p_j, w = v_i - v_j,
b = a_i - a_j at sample k:

    f(t) = |d + t w + t^2/2 b|^2 = c0 + c1 t + c2 t^2 + c3 t^3 + c4 t^4
    c0 = d.d   c1 = 2 d.w   c2 = w.w + d.b   c3 = w.b   c4 = b.b / 4

and the segment minimum is at t = 0, t = h or a real root of f' in (0, h).  The roots of f' come from the eigenvalues of
its companion matrix (numpy.linalg.eigvals, batched) where f' is a cubic, from the quadratic formula / the linear equation
where leading coefficients vanish (b = 0 makes f a quadratic).  Every root is used through its real part clipped to [0, h]:
f at ANY point of [0, h] is an upper bound of the minimum, and a real root inside is kept as it is, so nothing is missed and
nothing needs a tolerance on imaginary parts (a double root of f' arrives as a conjugate pair).  Two Newton steps on f'
(accepted only where they lower f) remove the eigenvalue solver's residue; in `numpy.longdouble` the same steps give the
extended-precision value the float64 evaluation is pinned against.

S = |d| + h |w| + h^2/2 |b| bounds every term of f by S^2; tolerances on f are stated in units of eps S^2.
"""
import numpy as np

EPS = np.finfo(np.float64).eps


def pair_indices(N):
    """(i, j) of the lexicographic pairs, i < j: q = index into these arrays"""
    i, j = np.triu_indices(N, 1)
    return i.astype(np.int64), j.astype(np.int64)


def coefficients(d, w, b, dtype=np.float64):
    d, w, b = (np.asarray(x, dtype=dtype) for x in (d, w, b))
    dot = lambda x, y: (x * y).sum(-1)  # noqa: E731
    return dot(d, d), 2 * dot(d, w), dot(w, w) + dot(d, b), dot(w, b), dot(b, b) / 4


def s_bound(d, w, b, h):
    n = lambda x: np.sqrt((np.asarray(x, dtype=np.float64) ** 2).sum(-1))  # noqa: E731
    return n(d) + h * n(w) + 0.5 * h * h * n(b)


def _f(c, t):
    return c[0] + t * (c[1] + t * (c[2] + t * (c[3] + t * c[4])))


def _g(c, t):
    return c[1] + t * (2 * c[2] + t * (3 * c[3] + t * 4 * c[4]))


def _gp(c, t):
    return 2 * c[2] + t * (6 * c[3] + t * 12 * c[4])


def stationary_candidates(c, h):
    """(M, 3) candidate times from the roots of f' (float64), clipped to [0, h]; unused slots hold 0."""
    c = [np.asarray(x, dtype=np.float64) for x in c]
    M = c[0].shape[0]
    out = np.zeros((M, 3))
    a3, a2, a1, a0 = 4 * c[4], 3 * c[3], 2 * c[2], c[1]
    cubic = a3 != 0
    if cubic.any():
        k = np.nonzero(cubic)[0]
        comp = np.zeros((k.size, 3, 3))
        comp[:, 1, 0] = comp[:, 2, 1] = 1.0
        comp[:, 0, 2] = -a0[k] / a3[k]
        comp[:, 1, 2] = -a1[k] / a3[k]
        comp[:, 2, 2] = -a2[k] / a3[k]
        bad = ~np.isfinite(comp).all(axis=(1, 2))  # a3 so small that the quotients overflow: no root of this size in [0, h]
        comp[bad] = 0.0
        out[k] = np.linalg.eigvals(comp).real
    quad = ~cubic & (a2 != 0)
    if quad.any():
        k = np.nonzero(quad)[0]
        disc = a1[k] ** 2 - 4 * a2[k] * a0[k]
        ok = disc >= 0
        sq = np.sqrt(np.where(ok, disc, 0.0))
        out[k, 0] = np.where(ok, (-a1[k] + sq) / (2 * a2[k]), -a1[k] / (2 * a2[k]))
        out[k, 1] = np.where(ok, (-a1[k] - sq) / (2 * a2[k]), -a1[k] / (2 * a2[k]))
    lin = ~cubic & ~quad & (a1 != 0)
    if lin.any():
        k = np.nonzero(lin)[0]
        out[k, 0] = -a0[k] / a1[k]
    return np.clip(np.nan_to_num(out, nan=0.0, posinf=h, neginf=0.0), 0.0, h)


def segment_minima(d, w, b, h, dtype=np.float64):
    """Minimum of f over [0, h] for M segments (d, w, b: (M, D)) -> (m, t), m = min f (not clamped, not rooted).
    Ties go to the first of the candidates 0, h, stationary points."""
    c = coefficients(d, w, b, dtype)
    hh = dtype(h)
    cand = stationary_candidates(coefficients(d, w, b), h).astype(dtype)
    for _ in range(2):  # Newton on f', kept where it stays inside and lowers f
        gp = _gp(c, cand.T).T
        step = np.where(gp != 0, _g(c, cand.T).T / np.where(gp != 0, gp, 1), 0)
        new = np.clip(cand - step, 0, hh)
        better = _f(c, new.T).T < _f(c, cand.T).T
        cand = np.where(better, new, cand)
    M = cand.shape[0]
    ts = np.concatenate([np.zeros((M, 1), dtype), np.full((M, 1), hh, dtype), cand], axis=1)
    vals = _f(c, ts.T).T
    k = np.argmin(vals, axis=1)
    r = np.arange(M)
    return vals[r, k], ts[r, k]


def dense_minima(d, w, b, h, points=401):
    """min of f over `points` equidistant samples of every segment, and a bound of how far above the true minimum that can
    lie: |f'| <= 2 S (|w| + h |b|) and the nearest sample is at most h / (2 (points - 1)) away"""
    c = coefficients(d, w, b)
    t = np.linspace(0.0, h, points)
    vals = _f([x[:, None] for x in c], t[None, :])
    n = lambda x: np.sqrt((np.asarray(x, dtype=np.float64) ** 2).sum(-1))  # noqa: E731
    slack = 2 * s_bound(d, w, b, h) * (n(w) + h * n(b)) * h / (2 * (points - 1))
    return vals.min(axis=1), slack


def all_segments(pos, vel, acc):
    """d, w, b of every row (k-major, then the lexicographic pairs): (K * pairs, D) each"""
    N, K, D = pos.shape
    i, j = pair_indices(N)
    dif = lambda x: (x[i] - x[j]).transpose(1, 0, 2).reshape(K * i.size, D)  # noqa: E731
    return dif(pos), dif(vel), dif(acc)


def global_stats(pos, vel, acc, h, R, q_begin=0, q_end=None):
    """What scp_check_separation reports, for the rows k * pairs + q, q in [q_begin, q_end), plus what the comparison rules
    need.  Segments whose distance cannot come below max(R - 0.01, smallest sampled distance) -- lower bound
    |d| - h |w| - h^2/2 |b|, with a 1e-3 margin -- are not minimised: they are neither violations nor the minimum."""
    N, K, D = pos.shape
    i, j = pair_indices(N)
    pairs = i.size
    q_end = pairs if q_end is None else q_end
    i, j = i[q_begin:q_end], j[q_begin:q_end]
    thr = R - 0.01
    n = lambda x: np.sqrt((x ** 2).sum(-1))  # noqa: E731
    sample_min, s_max = np.inf, 0.0
    for k in range(K):
        dn = n(pos[i, k] - pos[j, k])
        sample_min = min(sample_min, float(dn.min())) if dn.size else sample_min
    T = max(thr, sample_min) * (1 + 1e-3) + 1e-3
    rows, ms, ts = [], [], []
    for k in range(K):
        d, w, b = pos[i, k] - pos[j, k], vel[i, k] - vel[j, k], acc[i, k] - acc[j, k]
        reach = h * n(w) + 0.5 * h * h * n(b)
        dn = n(d)
        s_max = max(s_max, float((dn + reach).max())) if dn.size else s_max
        near = np.nonzero(dn - reach <= T)[0]
        if near.size:
            m, t = segment_minima(d[near], w[near], b[near], h)
            rows.append(k * pairs + q_begin + near)
            ms.append(m)
            ts.append(t)
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    ms = np.concatenate(ms) if ms else np.zeros(0)
    ts = np.concatenate(ts) if ts else np.zeros(0)
    order = np.lexsort((rows, ms))  # by f, ties by row
    best = order[0]
    viol = np.sqrt(np.maximum(ms, 0.0)) < thr
    return {"min_f": float(ms[best]), "argmin_row": int(rows[best]), "argmin_t": float(ts[best]),
            "second_f": float(ms[order[1]]) if order.size > 1 else np.inf,
            "sample_min_dist": sample_min, "rows": rows, "f": ms, "t": ts, "violating": viol,
            "n_violating": int(viol.sum()), "first_violation": int(rows[viol].min()) if viol.any() else 2**64 - 1,
            "s_max": s_max, "n_segments": K * (q_end - q_begin), "thr": thr}


def kinematics(p0, v0, acc, h):
    """positions / velocities at the K samples from p0, v0 and per-step accelerations (N, K, D): the model the stored
    trajectories follow (exact arithmetic order is irrelevant here: the result is only an INPUT of the check)"""
    N, K, D = acc.shape
    pos, vel = np.empty_like(acc), np.empty_like(acc)
    p, v = p0.astype(np.float64).copy(), v0.astype(np.float64).copy()
    for k in range(K):
        pos[:, k], vel[:, k] = p, v
        p = p + h * v + 0.5 * h * h * acc[:, k]
        v = v + h * acc[:, k]
    return pos, vel


def random_case(N, K, D, seed, h=0.2, side=20.0):
    """Random kinematically consistent trajectories within the project's limits (|v| <= 2, |a| <= 15 per axis) in a
    side^D box, so that close approaches occur: p0, v0 random, accelerations random with the velocity kept inside its limits"""
    rng = np.random.default_rng(seed)
    p0 = rng.uniform(0.0, side, (N, D))
    v0 = rng.uniform(-2.0, 2.0, (N, D))
    acc = np.empty((N, K, D))
    v = v0.copy()
    for k in range(K):
        a = rng.uniform(-15.0, 15.0, (N, D))
        a = np.clip(a, (-2.0 - v) / h, (2.0 - v) / h)  # keeps |v| <= 2 at the next sample
        acc[:, k] = a
        v = v + h * a
    return p0, v0, acc
