"""CPU checks of the staggered starts: header / exports / ctypes struct; the reference the GPU tests compare against
(tests/stagger_ref.py) -- the relative-lag statement under random delay vectors, the properties of the greedy schedule --; the
host helper staggered_fleet against delay_ref.shifted_fleet, bit for bit; the argument checks of SCP.stagger_starts need a GPU
object and live in tests/test_stagger_gpu.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delay_ref as dr  # noqa: E402
import separation_ref as sr  # noqa: E402
import stagger_ref as st  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scp_hip.h")
H = 0.2
RINGS = [(12, 25, 2, 1, 25), (16, 32, 3, 2, 32)]
_RINGS = {}


def ring(N, K, D, seed, S):
    """a half-ring case, its masks and its delay reference, made once"""
    key = (N, K, D, seed, S)
    if key not in _RINGS:
        host = st.half_ring(N, K, D, seed, H)
        mask, ref = st.masks(*host, H, 0.5, S)
        _RINGS[key] = (host, mask, ref)
    return _RINGS[key]


# ---- header, exports, struct mirror ------------------------------------------------------------------------------------------------
def test_header_exports_and_struct(tmp_path):
    from path_planning import _hip

    text = open(HEADER).read()
    for name in ("scp_lag_conflicts", "scp_ctx_last_lag_solved", "scp_schedule_starts"):
        assert name in _hip.EXPORTS and f"int {name}(" in text, name
    lib = ctypes.CDLL(_hip.library_path())
    assert all(hasattr(lib, n) for n in ("scp_lag_conflicts", "scp_ctx_last_lag_solved", "scp_schedule_starts"))
    fields = ["n_delayed", "n_unplaced", "max_delay", "first_unplaced", "total_delay", "reserved"]
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "scp_hip.h"', "int main(void) {",
           '  printf("%zu", sizeof(scp_start_schedule_stats));']
    src += [f'  printf(" %zu", offsetof(scp_start_schedule_stats, {f}));' for f in fields]
    src += ['  printf(" %d", SCP_ABI_VERSION);', "  return 0; }"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    cls = _hip.StartScheduleStats
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields] + [_hip.ABI_VERSION]
    assert got[0] == 48 and got[-1] == 7  # additive: the ABI version stays
    assert _hip.MAX_LAG == 63 and _hip.SCHEDULE_MAX_N == 16384


# ---- the relative-lag statement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,D,seed,S", RINGS)
def test_only_the_relative_lag_matters(N, K, D, seed, S):
    """d_a >= d_b: the pair conflicts in the fleet staggered by (d_a, d_b) iff bit d_a - d_b of mask[a][b] is set -- on every
    pair of random delay vectors, by the segments of the staggered pair themselves.  The answer is asked only where it is
    determined: no segment of the staggered pair within 1e-9 of the threshold (asserted: none here)."""
    host, mask, _ = ring(N, K, D, seed, S)
    rng = np.random.default_rng(100 + seed)
    checked = set_bits = 0
    for _ in range(6 if N == 12 else 5):
        d = rng.integers(0, S + 1, N)
        for a in range(N):
            for b in range(N):
                if a == b or d[a] < d[b] or (d[a] == d[b] and a > b):
                    continue
                viol, gap = st.pair_conflicts(*host, H, 0.5, a, b, int(d[a]), int(d[b]))
                assert gap > 1e-9, (a, b, d[a], d[b], gap)
                bit = (int(mask[a, b]) >> int(d[a] - d[b])) & 1
                assert viol == bool(bit), (a, b, int(d[a]), int(d[b]))
                checked += 1
                set_bits += bit
    print(f"half ring {N}x{K}x{D}: {checked} pairs under random delays, {set_bits} in conflict, no mismatch")
    assert checked >= 300 and 0 < set_bits < checked


def test_mask_structure_of_the_reference():
    host, mask, ref = ring(*RINGS[0])
    N, S = 12, 25
    assert (np.diag(mask) == 0).all() and (mask >> np.uint64(S + 1) == 0).all()
    assert ((mask & np.uint64(1)) == (mask.T & np.uint64(1))).all()  # bit 0 is symmetric
    for a in range(N):  # OR over b of bit s <=> entry (a, s) of the delay margins counts something
        anyb = np.bitwise_or.reduce(mask[a])
        assert [(int(anyb) >> s) & 1 for s in range(S + 1)] == (ref["n_violating"][a] > 0).astype(int).tolist()


@pytest.mark.parametrize("N,D,pair", [(2, 2, (0, 1)), (6, 2, (2, 4)), (7, 3, (3, 6))])
def test_crossing_case_mask(N, D, pair):
    """analytic: the margin of pair[0] at lag s is 0.2 sqrt(2) |3 - s| against 0.49 -> lags 2, 3, 4"""
    mask, _ = st.masks(*dr.crossing_case(N, D, pair), dr.CROSS_H, dr.CROSS_R, 8)
    want = np.zeros((N, N), dtype=np.uint64)
    want[pair[0], pair[1]] = 0x1C
    assert (mask == want).all()
    assert [s for s in range(9) if dr.crossing_margin(s) < 0.49] == [2, 3, 4]


# ---- the greedy schedule ----------------------------------------------------------------------------------------------------------
random_masks = st.random_masks  # (bit 0 symmetric, as in every mask of trajectories: `satisfies` reads ties both ways)


@pytest.mark.parametrize("N,S,density", [(1, 5, 0.5), (2, 0, 0.9), (9, 5, 0.3), (30, 63, 0.05), (30, 63, 0.5), (40, 5, 0.2)])
def test_greedy_properties(N, S, density):
    m = random_masks(N, S, density, 7 * N + S)
    rng = np.random.default_rng(N)
    for order in (None, rng.permutation(N)):
        delay, stats = st.greedy(m, S, order)
        assert all(-1 <= d <= S for d in delay) and st.satisfies(m, delay)
        placed = [v for v in range(N) if delay[v] >= 0]
        assert stats["n_unplaced"] == N - len(placed) and stats["total_delay"] == sum(delay[v] for v in placed)
        seq = list(range(N)) if order is None else [int(v) for v in order]
        assert delay[seq[0]] == 0  # nobody before it
        unplaced = [v for v in seq if delay[v] < 0]
        assert stats["first_unplaced"] == (unplaced[0] if unplaced else -1)
        # minimality: every smaller delay of a placed vehicle conflicts with somebody placed BEFORE it
        for t, v in enumerate(seq):
            before = [u for u in seq[:t] if delay[u] >= 0]
            for d in range(delay[v] if delay[v] >= 0 else S + 1):
                trial = {u: delay[u] for u in before}
                trial[v] = d
                sub = [trial.get(u, -1) for u in range(N)]
                assert not st.satisfies(m, sub), (v, d)
        # an unplaced vehicle takes no part later: the schedule of the others alone is the same
        if unplaced:
            keep = [v for v in seq if delay[v] >= 0]
            sub = m[np.ix_(keep, keep)]
            d2, s2 = st.greedy(sub, S)
            assert d2 == [delay[v] for v in keep] and s2["n_unplaced"] == 0


def test_greedy_without_lag_0_conflicts_is_all_zeros():
    m = random_masks(25, 20, 0.4, 3) & ~np.uint64(1)
    delay, stats = st.greedy(m, 20, np.random.default_rng(0).permutation(25))
    assert delay == [0] * 25 and stats == {"n_delayed": 0, "n_unplaced": 0, "max_delay": 0, "first_unplaced": -1, "total_delay": 0}


@pytest.mark.parametrize("N,K,D,seed,S", RINGS)
def test_half_ring_schedule(N, K, D, seed, S):
    host, mask, _ = ring(N, K, D, seed, S)
    delay, stats = st.greedy(mask, S)
    assert delay == list(range(0, 2 * N, 2)) and stats["n_unplaced"] == 0


# ---- the host helper ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,D,seed", [(7, 13, 3, 12), (5, 4, 2, 1)])
def test_staggered_fleet_is_the_shifted_fleet_bit_for_bit(N, K, D, seed):
    from path_planning.solvers.stagger import delays_satisfy_masks, staggered_fleet

    p0, v0, acc = sr.random_case(N, K, D, seed)
    pos, vel = sr.kinematics(p0, v0, acc, H)
    for a in range(N):
        for s in (0, 1, K // 2, K):
            d = np.zeros(N, dtype=np.int64)
            d[a] = s
            got = staggered_fleet(pos, vel, acc, H, d)
            want = dr.shifted_fleet(pos, vel, acc, H, a, s)
            assert all(g.shape == (N, K + s, D) and g.tobytes() == w.tobytes() for g, w in zip(got, want)), (a, s)
    d = np.random.default_rng(seed).integers(-1, K + 1, N)  # several at once, with unplaced ones: the reference's fleet
    got, want = staggered_fleet(pos, vel, acc, H, d), st.staggered(pos, vel, acc, H, d)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    m = random_masks(N, 5, 0.3, seed)
    for order in (None, np.random.default_rng(1).permutation(N)):
        delay, _ = st.greedy(m, 5, order)
        assert delays_satisfy_masks(m, delay) and st.satisfies(m, delay)
    bad = m.copy()
    bad[1, 0] |= np.uint64(1)
    bad[0, 1] |= np.uint64(1)
    assert not delays_satisfy_masks(bad, np.zeros(N, dtype=np.int64))
