"""numpy reference of the conflict list (scp_list_conflicts), written from the kinematics alone (not from the kernel): for
a segment with the quartic f of tests/separation_ref.py and the threshold thr, where f is below thr^2.

The real roots of g = f - thr^2 in (0, h) come from the eigenvalues of the companion matrix (numpy.roots), polished by
two Newton steps that are kept where they lower |g|.  Every root is used through its real part: a spurious split point
changes nothing, because what decides is the sign of g at the MIDDLE of every interval between consecutive points of
{0, roots, h} -- g has no root inside such an interval, so its sign there is the sign at the middle.  Intervals below the
threshold that touch are merged; t_enter / t_exit are the outer ends, pieces the number of merged runs."""
import numpy as np

import separation_ref as sr


def f_at(c, t):
    return c[0] + t * (c[1] + t * (c[2] + t * (c[3] + t * c[4])))


def window(c, h, thr):
    """c: the five coefficients of one segment -> (t_enter, t_exit, pieces, roots) or None when f is nowhere below thr^2"""
    c = [float(x) for x in c]
    g = [c[0] - thr * thr] + c[1:]
    poly = np.trim_zeros(g[::-1], "f")
    roots = np.roots(poly).real if len(poly) > 1 else np.zeros(0)
    gp = lambda t: c[1] + t * (2 * c[2] + t * (3 * c[3] + t * 4 * c[4]))  # noqa: E731
    for _ in range(2):
        d = gp(roots)
        new = roots - np.where(d != 0, f_at(g, roots) / np.where(d != 0, d, 1), 0)
        roots = np.where(np.abs(f_at(g, new)) < np.abs(f_at(g, roots)), new, roots)
    inner = np.sort(roots[(roots > 0) & (roots < h)])
    pts = np.concatenate([[0.0], inner, [h]])
    below = f_at(g, 0.5 * (pts[:-1] + pts[1:])) < 0
    if not below.any():
        return None
    k = np.nonzero(below)[0]
    pieces = 1 + int((np.diff(k) > 1).sum())
    return float(pts[k[0]]), float(pts[k[-1] + 1]), pieces, inner


def records(pos, vel, acc, h, R, q_begin=0, q_end=None):
    """The reference list of the rows k * pairs + q, q in [q_begin, q_end): sr.global_stats (rows, f, violating, s_max) plus,
    per violating row, the window -> dict with the arrays rows, f, t_min, t_enter, t_exit, pieces (violating rows only, in
    ascending row order) and `stats` (everything sr.global_stats returns, for the undecided rule)."""
    st = sr.global_stats(pos, vel, acc, h, R, q_begin, q_end)
    N, K, D = pos.shape
    i, j = sr.pair_indices(N)
    pairs = i.size
    order = np.argsort(st["rows"], kind="stable")
    out = {k: [] for k in ("rows", "f", "t_min", "t_enter", "t_exit", "pieces")}
    for e in order:
        if not st["violating"][e]:
            continue
        r = int(st["rows"][e])
        k, q = divmod(r, pairs)
        d, w, b = (x[i[q], k] - x[j[q], k] for x in (pos, vel, acc))
        c = sr.coefficients(d, w, b)
        win = window(c, h, st["thr"])
        if win is None:  # below the threshold by less than the root search resolves: the single point
            win = (float(st["t"][e]),) * 2 + (1, None)
        for key, v in zip(out, (r, st["f"][e], st["t"][e], win[0], win[1], win[2])):
            out[key].append(v)
    res = {k: np.asarray(v) for k, v in out.items()}
    res["stats"] = st
    return res


def segment_of_row(host, row):
    """(d, w, b) of one row of the host copies (pos, vel, acc)"""
    pos, vel, acc = host
    i, j = sr.pair_indices(pos.shape[0])
    k, q = divmod(int(row), i.size)
    return tuple(x[i[q], k] - x[j[q], k] for x in (pos, vel, acc))


def tunnelling_case(N, D, pair, K=8):
    """the construction of test_separation_gpu.test_tunnelling_pair: everybody far apart and at rest, except one pair whose
    relative position is 0.4 - 4 t along axis 0 in segment 3 (h = 0.2) -> pos, vel, acc, the row of that segment"""
    pos = np.zeros((N, K, D))
    vel = np.zeros((N, K, D))
    acc = np.zeros((N, K, D))
    pos[:, :, 0] = 100.0 * (1 + np.arange(N))[:, None]
    pos[:, :, D - 1] += 3.0 * np.arange(N)[:, None]
    i, j = pair
    rel = 0.4 + 0.8 * (3 - np.arange(K))
    pos[j] = pos[i]
    pos[i, :, 0] += 0.5 * rel
    pos[j, :, 0] -= 0.5 * rel
    vel[i, :, 0], vel[j, :, 0] = -2.0, 2.0
    q = [(a, b) for a in range(N) for b in range(a + 1, N)].index(pair)
    return pos, vel, acc, 3 * (N * (N - 1) // 2) + q


# relative motion (-0.3 + 3 t, -0.5 + 18 t - 90 t^2) over h = 0.2: a parabola around the origin; both arms pass within
# 0.2 m of it while the vertex (t = 0.1) is 0.4 m away -> (d, w, b)
TWO_PIECES = (np.array([-0.3, -0.5]), np.array([3.0, 18.0]), np.array([0.0, -180.0]))
