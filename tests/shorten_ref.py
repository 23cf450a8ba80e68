"""numpy / plain-Python restatement of the shortening rules of include/scp_hip.h ("shortened reference paths"): visibility of
two lattice nodes, the kept nodes, the vertices, the lengths, the reference points by chord length and delta.  Integers
exactly; lengths and points bit for bit (numpy rounds every product, quotient, sum, difference and square root on its own).
Lattice, node ids, block centres and the summed-table range count are those of tests/reference_path_ref.py."""
import numpy as np

import reference_path_ref as rr

SHORTEN_INFO_DTYPE = np.dtype([("n_kept", np.int32), ("n_vertices", np.int32), ("length", np.float64),
                               ("length_before", np.float64)])


def clear_many(D, sat, stride, clearance, XA, XB):
    """clear(A, B) for M pairs of nodes at once: XA, XB (3, M) node coordinates -> bool (M,).  Every step of every pair is
    evaluated (no early exit: the answer is the same)."""
    nz, ny, nx = sat.shape
    dims = (nx, ny, nz)
    XA, XB = np.asarray(XA, dtype=np.int64).reshape(3, -1), np.asarray(XB, dtype=np.int64).reshape(3, -1)
    M = XA.shape[1]
    d = XB - XA
    n = np.abs(d[:D]).max(axis=0)
    pair = np.repeat(np.arange(M), n)                      # the pair of every step
    k = np.arange(pair.size) - np.repeat(np.cumsum(n) - n, n)  # and its number k = 0 .. n - 1
    npair = n[pair]
    a, b = [np.zeros(pair.size, dtype=np.int64)] * 3, [np.zeros(pair.size, dtype=np.int64)] * 3
    for q in range(D):
        u0 = XA[q, pair] * npair + d[q, pair] * k
        u1 = u0 + d[q, pair]
        assert (u0 >= 0).all() and (u1 >= 0).all()
        lo = np.minimum(u0, u1) // npair
        hi = (np.maximum(u0, u1) + npair - 1) // npair
        a[q] = np.maximum(lo * stride - clearance, 0)
        b[q] = np.minimum(hi * stride + stride - 1 + clearance, dims[q] - 1)
    occupied = rr.occupied_in(sat, a, b) != 0
    return np.bincount(pair[occupied], minlength=M) == 0


def clear(D, sat, L, stride, clearance, A, B):
    """clear(A, B) of two node ids"""
    XA, XB = np.array(rr.node_coords(L, A)).reshape(3, 1), np.array(rr.node_coords(L, B)).reshape(3, 1)
    return bool(clear_many(D, sat, stride, clearance, XA, XB)[0])


def kept_nodes(D, sat, L, stride, clearance, nodes):
    """the kept list t_0 < .. < t_{n-1} of a path (node ids): from every anchor the LARGEST later t it sees"""
    nodes = np.asarray(nodes, dtype=np.int64)
    m = nodes.size
    X = np.array(rr.node_coords(L, nodes))
    kept = [0]
    while kept[-1] < m - 1:
        t0 = kept[-1]
        sees = clear_many(D, sat, stride, clearance, np.repeat(X[:, t0:t0 + 1], m - 1 - t0, axis=1), X[:, t0 + 1:])
        assert sees[0], "the next node of a path is a neighbour over a set edge"
        kept.append(t0 + 1 + int(np.nonzero(sees)[0][-1]))
    return kept


def centre(origin, cell, L, stride, node, D):
    X = rr.node_coords(L, int(node))
    return np.array([np.float64(origin[d]) + np.float64(cell) * (np.float64(X[d] * stride) + np.float64(0.5) * np.float64(stride))
                     for d in range(D)])


def polyline_lengths(W):
    """(len_i, S_i) of the vertices W (nv, D): every square, sum, root rounded on its own, the sums in order from 0.0"""
    nv, D = W.shape
    lens = np.empty(nv - 1)
    S = np.zeros(nv)
    for i in range(nv - 1):
        acc = np.float64(0.0)
        for d in range(D):
            diff = np.float64(W[i + 1, d]) - np.float64(W[i, d])
            acc = acc + diff * diff
        lens[i] = np.sqrt(acc)
        S[i + 1] = S[i] + lens[i]
    return lens, S


def vertices(D, origin, cell, L, stride, p0, pf, nodes, kept):
    """W_0 .. W_{nv-1}: p0, the centres of the kept nodes other than the first and the last, pf"""
    n = len(kept)
    nv = max(n, 2)
    W = np.empty((nv, D))
    W[0] = np.asarray(p0, dtype=np.float64)[:D]
    W[nv - 1] = np.asarray(pf, dtype=np.float64)[:D]
    for i in range(1, n - 1):
        W[i] = centre(origin, cell, L, stride, nodes[kept[i]], D)
    return W


def lattice_vertices(D, origin, cell, L, stride, p0, pf, nodes):
    """V_0 .. V_{m+1} of scp_reference_paths: p0, every block centre, pf"""
    m = len(nodes)
    V = np.empty((m + 2, D))
    V[0] = np.asarray(p0, dtype=np.float64)[:D]
    V[m + 1] = np.asarray(pf, dtype=np.float64)[:D]
    for t, node in enumerate(nodes):
        V[t + 1] = centre(origin, cell, L, stride, node, D)
    return V


def points_by_chord_length(W, K):
    """(K + 1, D) reference points along the polyline W, (lens, S)"""
    nv, D = W.shape
    lens, S = polyline_lengths(W)
    length = S[nv - 1]
    out = np.empty((K + 1, D))
    out[0] = W[0]
    out[K] = W[nv - 1]
    for j in range(1, K):
        target = (np.float64(j) / np.float64(K)) * length
        i = int(np.nonzero(S[1:] >= target)[0][0])
        if lens[i] == 0.0:
            out[j] = W[i]
        else:
            w = min((target - S[i]) / lens[i], np.float64(1.0))
            out[j] = W[i] + w * (W[i + 1] - W[i])
    return out, lens, S


def delta_of(length, K, cell):
    """the largest difference, in cells per coordinate, between the cells of two consecutive reference points"""
    return np.floor(np.asarray(length, dtype=np.float64) / (np.float64(K) * np.float64(cell))).astype(np.int64) + 1


def shorten_paths(D, origin, cell, sat, stride, clearance, p0, pf, K, path, info, ref):
    """-> (ref (N, K + 1, D) with the rows of the found vehicles replaced, kept (N, max_path) int32, out SHORTEN_INFO_DTYPE (N,),
    W: the vertices of every found vehicle (None for the others))"""
    nz, ny, nx = sat.shape
    L = rr.lattice(D, (nx, ny, nz), stride)
    p0, pf = np.asarray(p0, dtype=np.float64), np.asarray(pf, dtype=np.float64)
    N, max_path = path.shape
    ref = np.array(ref, dtype=np.float64, copy=True)
    kept = np.full((N, max_path), -1, dtype=np.int32)
    out = np.zeros(N, dtype=SHORTEN_INFO_DTYPE)
    Ws = [None] * N
    for i in range(N):
        if info["status"][i] != 0:
            continue
        m = int(info["n_nodes"][i])
        nodes = path[i, :m]
        ks = kept_nodes(D, sat, L, stride, clearance, nodes)
        kept[i, :len(ks)] = ks
        W = vertices(D, origin, cell, L, stride, p0[i], pf[i], nodes, ks)
        ref[i], _, S = points_by_chord_length(W, K)
        _, Sb = polyline_lengths(lattice_vertices(D, origin, cell, L, stride, p0[i], pf[i], nodes))
        out[i] = (len(ks), W.shape[0], S[-1], Sb[-1])
        Ws[i] = W
    return ref, kept, out, Ws
