"""numpy restatement of the grid-swap-device family (the algorithm as include/scp_hip.h and DESIGN.md state it), for
the tests: scp_generate_grid_swap must reproduce it bit for bit.  Not part of the product."""
import numpy as np

_U = np.uint64
_GOLD, _C1, _C2 = _U(0x9E3779B97F4A7C15), _U(0xBF58476D1CE4E5B9), _U(0x94D049BB133111EB)
TAG_START, TAG_PERM, TAG_GOAL = 1, 2, 3
DEFAULTS = dict(pitch=2.0, jitter=0.2, block=4, layer_gap=2.0, min_sep=0.3, max_tries=8192, sweeps=20)


def mix(z):
    """SplitMix64 on uint64 arrays (wrapping arithmetic)"""
    z = np.asarray(z, dtype=_U) + _GOLD
    z = (z ^ (z >> _U(30))) * _C1
    z = (z ^ (z >> _U(27))) * _C2
    return z ^ (z >> _U(31))


def prefix(seed, tag, layer, block, sweep, rnd, cand):
    h = mix(np.asarray([int(seed) & ((1 << 64) - 1)], dtype=_U))
    for v in (tag, layer, block, sweep, rnd):
        h = mix(h ^ _U(v))
    return mix(h ^ np.asarray(cand, dtype=_U))


def coord(cell, h, pitch, jitter):
    u = (h >> _U(11)).astype(np.float64) * 2.0 ** -53
    return np.asarray(cell, dtype=np.float64) * pitch + (2.0 * u - 1.0) * jitter


def d2_plane(r0x, r0y, gx, gy):
    """squared closest approach, x terms before y terms, every product rounded"""
    drx, dry = gx - r0x, gy - r0y
    den = drx * drx + dry * dry
    s = np.clip(-(r0x * drx + r0y * dry) / np.where(den > 0, den, 1.0), 0.0, 1.0)
    cx, cy = r0x + s * drx, r0y + s * dry
    return cx * cx + cy * cy


def d2_space(r0, g):
    """the same in D coordinates, summed in coordinate order"""
    dr = g - r0
    den = dr[..., 0] * dr[..., 0] + dr[..., 1] * dr[..., 1]
    dot = r0[..., 0] * dr[..., 0] + r0[..., 1] * dr[..., 1]
    for d in range(2, r0.shape[-1]):
        den = den + dr[..., d] * dr[..., d]
        dot = dot + r0[..., d] * dr[..., d]
    s = np.clip(-dot / np.where(den > 0, den, 1.0), 0.0, 1.0)
    c = r0 + s[..., None] * dr
    out = c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]
    for d in range(2, r0.shape[-1]):
        out = out + c[..., d] * c[..., d]
    return out


def layout(N, dim, block):
    """(layers, per, side, blocks): blocks = list of (layer, owner id in the layer, member agent ids ascending)"""
    layers = 1
    if dim == 3:
        while layers ** 3 < N:
            layers += 1
    per = -(-N // layers)
    side = 1
    while side * side < per:
        side += 1
    stride = side // block + 1
    blocks = []
    base = 0
    for L in range(layers):
        if base >= N:
            break
        cnt = min(per, N - base)
        c = np.arange(cnt)
        key = (c // side // block) * stride + (c % side) // block
        for o, k in enumerate(np.unique(key)):
            blocks.append((L, o, base + np.nonzero(key == k)[0]))
        base += cnt
    return layers, per, side, blocks


def _cells(agents, per, side):
    c = agents % per
    return np.stack([c // side, c % side], axis=1)


def draw_block(seed, L, o, sweep, cells, a, p):
    """goal (m, 2) of one block draw and whether it met min_sep"""
    m = len(cells)
    thr = p["min_sep"] * p["min_sep"]
    t = np.arange(256)
    iu, ju = np.triu_indices(m, 1)
    best_d, best_g = -1.0, None
    for r in range(max(1, p["max_tries"] // 256)):
        pp = prefix(seed, TAG_PERM, L, o, sweep, r, t)
        perm = np.tile(np.arange(m), (256, 1))
        for i in range(m - 1, 0, -1):
            h = mix(pp ^ _U(i))
            j = (((h >> _U(32)) * _U(i + 1)) >> _U(32)).astype(np.int64)
            vi = perm[t, i].copy()
            perm[t, i] = perm[t, j]
            perm[t, j] = vi
        pg = prefix(seed, TAG_GOAL, L, o, sweep, r, t)
        h = mix(pg[:, None] ^ np.arange(2 * m, dtype=_U)[None, :])
        gx = coord(cells[perm, 0], h[:, 0::2], p["pitch"], p["jitter"])
        gy = coord(cells[perm, 1], h[:, 1::2], p["pitch"], p["jitter"])
        if m > 1:
            d2 = d2_plane((a[iu, 0] - a[ju, 0])[None], (a[iu, 1] - a[ju, 1])[None], gx[:, iu] - gx[:, ju],
                          gy[:, iu] - gy[:, ju])
            score = d2.min(axis=1)
        else:
            score = np.full(256, np.inf)
        ok = np.nonzero(score >= thr)[0]
        pick = int(ok[0]) if ok.size else int(np.argmax(score))
        if score[pick] > best_d:
            best_d, best_g = float(score[pick]), np.stack([gx[pick], gy[pick]], axis=1)
        if ok.size:
            break
    return best_g, best_d >= thr


def _pair_rows(xy, gxy, rows, cols):
    return d2_plane(xy[rows, 0][:, None] - xy[cols, 0][None], xy[rows, 1][:, None] - xy[cols, 1][None],
                    gxy[rows, 0][:, None] - gxy[cols, 0][None], gxy[rows, 1][:, None] - gxy[cols, 1][None])


def generate(N, seed, dim=2, **params):
    """(init (N, dim), goal (N, dim), space (2 dim,), stats dict) of scenario `seed`"""
    p = dict(DEFAULTS, **params)
    layers, per, side, blocks = layout(N, dim, p["block"])
    thr = p["min_sep"] * p["min_sep"]
    k = np.arange(N)
    L_of = k // per
    c = k - L_of * per
    xy = np.empty((N, 2))
    for L in range(layers):
        sel = np.nonzero(L_of == L)[0]
        if not sel.size:
            continue
        pre = prefix(seed, TAG_START, L, 0, 0, 0, 0)
        xy[sel, 0] = coord(c[sel] // side, mix(pre ^ (2 * c[sel]).astype(_U)), p["pitch"], p["jitter"])
        xy[sel, 1] = coord(c[sel] % side, mix(pre ^ (2 * c[sel] + 1).astype(_U)), p["pitch"], p["jitter"])
    gxy = np.empty((N, 2))
    owner = np.empty(N, dtype=np.int64)
    unmet = np.zeros(len(blocks), dtype=bool)

    def draw(bi, sweep):
        L, o, idx = blocks[bi]
        gxy[idx], met = draw_block(seed, L, o, sweep, _cells(idx, per, side), xy[idx], p)
        unmet[bi] = not met

    for bi, (L, o, idx) in enumerate(blocks):
        owner[idx] = bi
        draw(bi, 0)

    def cross_pairs():
        """(flagged blocks, conflicting pair count) over the cross-block pairs of every layer"""
        flagged, count = set(), 0
        for L in range(layers):
            ids = np.nonzero(L_of == L)[0]
            for s0 in range(0, ids.size, 512):
                rows = ids[s0:s0 + 512]
                d2 = _pair_rows(xy, gxy, rows, ids)
                bad = (d2 < thr) & (owner[rows][:, None] != owner[ids][None]) & (rows[:, None] < ids[None])
                rr, cc = np.nonzero(bad)
                count += rr.size
                flagged.update(np.maximum(owner[rows[rr]], owner[ids[cc]]).tolist())
        return flagged, count

    used = 0
    for s in range(1, p["sweeps"] + 1):
        flagged, _ = cross_pairs()
        if not flagged:
            break
        for bi in sorted(flagged):
            draw(bi, s)
        used = s
    _, conflicts = cross_pairs()
    if dim == 3:
        z = L_of.astype(np.float64) * p["layer_gap"]
        init = np.hstack([xy, z[:, None]])
        goal = np.hstack([gxy, z[:, None]])
    else:
        init, goal = xy.copy(), gxy.copy()
    dmin = np.inf
    for s0 in range(0, N, 512):
        rows = np.arange(s0, min(N, s0 + 512))
        d2 = d2_space(init[rows][:, None] - init[None], goal[rows][:, None] - goal[None])
        d2[rows[:, None] >= np.arange(N)[None]] = np.inf
        dmin = min(dmin, float(d2.min()))
    lo = np.minimum(init.min(axis=0), goal.min(axis=0)) - 2.0
    hi = np.maximum(init.max(axis=0), goal.max(axis=0)) + 2.0
    min_approach = float(np.sqrt(dmin))
    stats = dict(sweeps=used, unmet_blocks=int(unmet.sum()), conflicts=int(conflicts), min_approach=min_approach,
                 ok=bool(min_approach >= p["min_sep"]))
    return init, goal, np.concatenate([lo, hi]), stats


def blocks_of(N, dim, block=4):
    """member agent ids of every block (for the tests' permutation check)"""
    return [idx for _, _, idx in layout(N, dim, block)[3]]
