"""numpy reference of the clearance profile (scp_clearance_profile), written from the kinematics alone (not from the kernel):
the segment minima of tests/separation_ref.py on EVERY row of the pair range -- no pruning --, reduced per vehicle (all rows
whose pair contains it) and per time step, lexicographically by (f, row).

An entry is a set of parallel arrays: f (the smallest minimum of the quartic, not clamped, not rooted; +inf: no row), row
(2^64 - 1: none), t, second_f (the entry's second-smallest f: how well the row is determined), n_violating
(sqrt(max(f, 0)) < R - 0.01), sample (the smallest numpy norm of d over the entry's rows) and n_rows (rows it covers)."""
import numpy as np

import separation_ref as sr

NO_ROW = 2**64 - 1
FIELDS = ("f", "row", "t", "second_f", "n_violating", "sample", "n_rows")


def _reduce(ent, n_ent, f, rows, t, viol, dn):
    """ent: the entry of every item (items may repeat a row: once per vehicle of its pair)"""
    out = {"f": np.full(n_ent, np.inf), "row": np.full(n_ent, NO_ROW, dtype=np.uint64), "t": np.zeros(n_ent),
           "second_f": np.full(n_ent, np.inf), "n_violating": np.zeros(n_ent, dtype=np.int64),
           "sample": np.full(n_ent, np.inf), "n_rows": np.zeros(n_ent, dtype=np.int64)}
    if ent.size == 0:
        return out
    order = np.lexsort((rows, f, ent))  # by entry, then f, then row
    e_s = ent[order]
    first = np.nonzero(np.concatenate([[True], e_s[1:] != e_s[:-1]]))[0]
    who = e_s[first]
    out["f"][who], out["row"][who], out["t"][who] = f[order][first], rows[order][first].astype(np.uint64), t[order][first]
    second = first + 1
    ok = (second < e_s.size) & (e_s[np.minimum(second, e_s.size - 1)] == who)
    out["second_f"][who[ok]] = f[order][second[ok]]
    out["n_violating"] = np.bincount(ent, weights=viol, minlength=n_ent).astype(np.int64)
    out["n_rows"] = np.bincount(ent, minlength=n_ent).astype(np.int64)
    np.minimum.at(out["sample"], ent, dn)
    return out


def profile(pos, vel, acc, h, R, q_begin=0, q_end=None, skip_pairs=()):
    """-> {"vehicle": entry arrays of length N, "step": of length K, "s_max", "thr", "pairs", "rows", "f"}; rows k * pairs + q,
    q in [q_begin, q_end) without the pair indices in skip_pairs (the CPU tests remove a vehicle's nearest partner with it)"""
    N, K, D = pos.shape
    i, j = sr.pair_indices(N)
    pairs = i.size
    q_end = pairs if q_end is None else q_end
    d, w, b = sr.all_segments(pos, vel, acc)
    q = np.arange(q_begin, q_end)
    q = q[~np.isin(q, np.asarray(skip_pairs, dtype=np.int64))]
    rows = (np.arange(K)[:, None] * pairs + q[None, :]).reshape(-1)
    d, w, b = d[rows], w[rows], b[rows]
    if rows.size:
        f, t = sr.segment_minima(d, w, b, h)
    else:
        f, t = np.zeros(0), np.zeros(0)
    thr = R - 0.01
    viol = np.sqrt(np.maximum(f, 0.0)) < thr
    dn = np.sqrt((d ** 2).sum(-1))
    qi, qj = i[rows % pairs], j[rows % pairs]
    two = lambda x: np.concatenate([x, x])  # noqa: E731
    veh = _reduce(np.concatenate([qi, qj]), N, two(f), two(rows), two(t), two(viol), two(dn))
    step = _reduce(rows // pairs if pairs else rows, K, f, rows, t, viol, dn)
    return {"vehicle": veh, "step": step, "s_max": float(sr.s_bound(d, w, b, h).max()) if rows.size else 0.0, "thr": thr,
            "pairs": pairs, "rows": rows, "f": f}


def merge(parts):
    """entry arrays of disjoint shards -> those of their union"""
    out = {k: v.copy() for k, v in parts[0].items()}
    for p in parts[1:]:
        both = np.sort(np.stack([out["f"], out["second_f"], p["f"], p["second_f"]]), axis=0)
        better = (p["f"] < out["f"]) | ((p["f"] == out["f"]) & (p["row"] < out["row"]))
        for k in ("f", "row", "t"):
            out[k] = np.where(better, p[k], out[k])
        out["second_f"] = both[1]
        out["n_violating"] = out["n_violating"] + p["n_violating"]
        out["n_rows"] = out["n_rows"] + p["n_rows"]
        out["sample"] = np.minimum(out["sample"], p["sample"])
    return out


def equal(a, b):
    """per entry: are all fields of the two sets of entry arrays equal (bitwise for the floats)?"""
    same = np.ones(a["f"].size, dtype=bool)
    for k in FIELDS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        same &= (x == y) | ((x != x) & (y != y))
    return same
