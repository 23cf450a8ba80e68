"""GPU tests of the staggered starts -- scp_lag_conflicts, scp_schedule_starts, SCP.stagger_starts and the two CLIs -- against the
reference of tests/stagger_ref.py (pinned on the CPU by tests/test_stagger_cpu.py), against scp_delay_margins on the same device
tensors with no tolerance, and, end to end, against scp_check_separation on the staggered fleet.

A mask bit is a yes / no about segments, so the comparison with the reference is exact wherever the inputs decide it: the
conditions -- no segment within TOL = 32 eps S_max^2 of the threshold (the rule of tests/test_delay_gpu.py) -- are asserted on
the reference before anything is asked of a kernel.  The schedule is integer only: equality throughout."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delay_ref as dr  # noqa: E402
import separation_ref as sr  # noqa: E402
import stagger_ref as st  # noqa: E402

pytestmark = pytest.mark.gpu

H = 0.2
RANDOM = [(2, 9, 2, 11, 9), (7, 13, 3, 12, 13), (65, 7, 2, 17, 7), (129, 7, 2, 17, 3), (130, 9, 3, 21, 4), (65, 50, 3, 16, 5)]
NONZERO = [0, 0, 95, 340, 35, 35]   # non-zero mask words of the six cases (reference)
UNPLACED = [0, 0, 19, 58, 4, 5]     # vehicles the reference's schedule leaves unplaced: random starts closer than R
RINGS = [(12, 25, 2, 1, 25, list(range(0, 24, 2)), 328), (16, 32, 3, 2, 32, list(range(0, 32, 2)), 750)]
_CASES = {}


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def device(ctx, host):
    return tuple(ctx.tensor(np.ascontiguousarray(x)) for x in host)


def random_case(ctx, N, K, D, seed, S=None, R=0.8):
    """separation_ref.random_case as it is: host arrays, device copies and (with S) the reference masks, made once"""
    key = (N, K, D, seed)
    if key not in _CASES:
        p0, v0, acc = sr.random_case(N, K, D, seed)
        pos, vel = sr.kinematics(p0, v0, acc, H)
        host = (pos, vel, acc)
        _CASES[key] = (device(ctx, host), host, {})
    dev, host, refs = _CASES[key]
    if S is not None and (R, S) not in refs:
        mask, ref = st.masks(*host, H, R, S)
        refs[(R, S)] = (mask, ref)
    return dev, host, refs.get((R, S))


def run(ctx, dev, R, S, a0=0, a1=None, h=H):
    pos, vel, acc = dev
    N, K, D = pos.shape
    return ctx.lag_conflicts(N, K, D, h, R, pos, vel, acc, S, a0, a1)


def near_threshold(ref, tol):
    return sum(int((np.abs(f - ref["thr"] ** 2) <= tol).sum()) for f in ref["seg_f"].values())


def total_segments(N, K, S):
    return N * (N - 1) * sum(K + s for s in range(S + 1))


# ---- 1. masks against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(RANDOM)))
def test_masks_vs_reference(ctx, case):
    N, K, D, seed, S = RANDOM[case]
    dev, host, (want, ref) = random_case(ctx, N, K, D, seed, S)
    tol = 32 * sr.EPS * ref["s_max"] ** 2
    near = near_threshold(ref, tol)  # a condition on the INPUTS
    print(f"random {N}x{K}x{D} S={S}: segments within TOL of the threshold {near}, non-zero words {int((want != 0).sum())}")
    assert near == 0 and int((want != 0).sum()) == NONZERO[case]
    got = run(ctx, dev, 0.8, S)
    assert got.shape == (N, N) and got.dtype == np.uint64
    assert (got == want).all(), np.argwhere(got != want)[:5]
    solved = ctx.last_lag_solved()
    print(f"random {N}x{K}x{D} S={S}: {solved} of {total_segments(N, K, S)} segments reached the quartic")
    assert 0 <= solved <= total_segments(N, K, S) and (solved > 0 or NONZERO[case] == 0)
    assert run(ctx, dev, 0.8, S).tobytes() == got.tobytes()  # a second run: the same bytes


# ---- 2. against scp_delay_margins, no tolerance ----------------------------------------------------------------------------------------
def assert_masks_are_the_margins(ctx, dev, R, S, label):
    pos, vel, acc = dev
    N, K, D = pos.shape
    mask = run(ctx, dev, R, S)
    margins = ctx.delay_margins(N, K, D, H, R, pos, vel, acc, S)
    anyb = np.bitwise_or.reduce(mask, axis=1)
    bits = ((anyb[:, None] >> np.arange(S + 1, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    assert (bits == (margins["n_violating"] > 0)).all(), label
    return mask, margins


@pytest.mark.parametrize("N,K,D,seed,S", RANDOM)
def test_masks_are_the_delay_margins_counts(ctx, N, K, D, seed, S):
    dev, _, _ = random_case(ctx, N, K, D, seed)
    assert_masks_are_the_margins(ctx, dev, 0.8, S, (N, K, D))


@pytest.mark.parametrize("N,K,D", [(300, 4, 2), (200, 3, 3)])
def test_coincident_vehicles_in_interior_tiles(ctx, N, K, D):
    """vehicles at rest on a 10 m grid, some pairs at distance 0 (and some close, moving ones) in the middle of the fleet"""
    R, S = 0.8, 2
    pos = np.zeros((N, K, D))
    vel = np.zeros((N, K, D))
    acc = np.zeros((N, K, D))
    side = int(np.ceil(np.sqrt(N)))
    pos[:, :, 0] = 10.0 * (np.arange(N) % side)[:, None]
    pos[:, :, 1] = 10.0 * (np.arange(N) // side)[:, None]
    e0 = np.zeros(D)
    e0[0] = 1.0
    a = N // 2 + 3
    pos[a + 1] = pos[a]                                          # coincident throughout
    pos[a + 70] = pos[a + 2]                                     # coincident, the partner in another tile
    pos[a + 5] = pos[a + 4] + 1.0 * e0; vel[a + 5] = -1.5 * e0   # approaches and passes: f' linear
    pos[a + 7] = pos[a + 6] + 0.9 * e0                           # at rest and clear
    mask, margins = assert_masks_are_the_margins(ctx, device(ctx, (pos, vel, acc)), R, S, (N, K, D))
    full = np.uint64((1 << (S + 1)) - 1)
    for v, w in ((a, a + 1), (a + 2, a + 70)):
        assert mask[v, w] == full and mask[w, v] == full
    assert mask[a + 6, a + 7] == 0 and mask[a + 4, a + 5] != 0
    assert int((mask != 0).sum()) == 6 and (margins["min_dist"][[a, a + 1, a + 2, a + 70]] == 0.0).all()


# ---- 3. structure --------------------------------------------------------------------------------------------------------------------
def test_structure(ctx):
    for N, K, D, seed, S in RANDOM[2:]:
        dev, _, _ = random_case(ctx, N, K, D, seed)
        m = run(ctx, dev, 0.8, S)
        assert (np.diag(m) == 0).all() and ((m & np.uint64(1)) == (m.T & np.uint64(1))).all()  # bit 0 is symmetric
        assert S == 63 or (m >> np.uint64(S + 1) == 0).all()                                   # bits above max_lag
        m0 = run(ctx, dev, 0.8, 0)                                                             # max_lag = 0
        assert (m0 == (m & np.uint64(1))).all() and (m0 != 0).any()
    dev, _, _ = random_case(ctx, 7, 13, 3, 12)
    one = run(ctx, tuple(x[:1].contiguous() for x in dev), 0.8, 5)  # N = 1
    assert one.shape == (1, 1) and one[0, 0] == 0
    # K = 65, S = 63: bit 63.  Vehicle 1 stands beside the START of vehicle 0, which leaves at once: 0 conflicts with 1 while it
    # is held, at every lag >= 1; vehicle 3 stands where 2 ARRIVES: with 3 late nothing changes (it never moves), a conflict
    # at every lag both ways; vehicle 4 is far away
    N, K, D, S = 5, 65, 2, 63
    pos = np.zeros((N, K, D))
    vel = np.zeros((N, K, D))
    t = H * np.arange(K)
    vel[0, :, 0] = 2.0
    pos[0, :, 0] = 2.0 * t
    pos[1, :, 1] = 0.5   # in conflict with the held 0 and with its first segment
    pos[2, :, 0] = 100.0 + 2.0 * t
    vel[2, :, 0] = 2.0
    pos[3, :, 0] = 100.0 + 2.0 * H * K
    pos[3, :, 1] = 0.5
    pos[4] = (50.0, 50.0)
    host = (pos, vel, np.zeros_like(pos))
    want, ref = st.masks(*host, H, 0.8, S)
    assert near_threshold(ref, 32 * sr.EPS * ref["s_max"] ** 2) == 0
    m = run(ctx, device(ctx, host), 0.8, S)
    assert (m == want).all()
    assert m[0, 1] == np.uint64(2**64 - 1) and m[2, 3] == np.uint64(2**64 - 1) and (m[4] == 0).all() and (m[:, 4] == 0).all()
    assert int(m[1, 0]) & 1 and int(m[3, 2]) >> 63 == 1


# ---- 4. the crossing case ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,pair", [(2, 2, (0, 1)), (6, 2, (2, 4)), (7, 3, (3, 6))])
def test_crossing_case(ctx, N, D, pair):
    host = dr.crossing_case(N, D, pair)
    S, R = 8, dr.CROSS_R
    want, ref = st.masks(*host, dr.CROSS_H, R, S)
    assert near_threshold(ref, 32 * sr.EPS * ref["s_max"] ** 2) == 0
    got = run(ctx, device(ctx, host), R, S, h=dr.CROSS_H)
    analytic = np.zeros((N, N), dtype=np.uint64)
    analytic[pair[0], pair[1]] = 0x1C  # 0.2 sqrt(2) |3 - s| < 0.49: s = 2, 3, 4
    assert (want == analytic).all() and (got == analytic).all()


# ---- 5. cut independence -------------------------------------------------------------------------------------------------------------
def test_cuts_do_not_show(ctx):
    import torch

    N, K, D, seed, S = 129, 7, 2, 17, 3
    dev, _, _ = random_case(ctx, N, K, D, seed)
    full = run(ctx, dev, 0.8, S)
    parts = [run(ctx, dev, 0.8, S, x, y) for x, y in ((0, 63), (63, 64), (64, 129))]
    assert [p.shape for p in parts] == [(63, N), (1, N), (65, N)]
    assert b"".join(p.tobytes() for p in parts) == full.tobytes()
    assert run(ctx, dev, 0.8, S, 64, 64).shape == (0, N)
    poison = torch.full((64,), 0xA5, dtype=torch.uint8, device=ctx.tdev)
    pos, vel, acc = dev
    for a in (5, N):
        assert ctx.lib.scp_lag_conflicts(ctx.h, N, K, D, H, 0.8, a, a, S, pos.data_ptr(), vel.data_ptr(), acc.data_ptr(),
                                         poison.data_ptr()) == 0
    assert (poison.cpu().numpy() == 0xA5).all() and ctx.last_lag_solved() == 0  # an empty range writes nothing
    N2, K2, D2, seed2, S2 = 130, 9, 3, 21, 4
    dev2, _, _ = random_case(ctx, N2, K2, D2, seed2)
    full2 = run(ctx, dev2, 0.8, S2)
    try:
        for lc, gc in ((3, 5), (5, 1), (1, 13), (2, 4), (1, 1)):
            ctx.set_option("lagc_lag_chunk", lc)
            ctx.set_option("lagc_time_chunk", gc)
            assert run(ctx, dev2, 0.8, S2).tobytes() == full2.tobytes(), (lc, gc)
            assert 0 < ctx.last_lag_solved() <= total_segments(N2, K2, S2)
            assert run(ctx, dev2, 0.8, S2, 63, 65).tobytes() == np.ascontiguousarray(full2[63:65]).tobytes(), (lc, gc)
            assert run(ctx, dev, 0.8, S).tobytes() == full.tobytes(), (lc, gc)
    finally:
        ctx.set_option("lagc_lag_chunk", 0)
        ctx.set_option("lagc_time_chunk", 0)
    assert run(ctx, dev2, 0.8, S2).tobytes() == full2.tobytes()


# ---- 6. the schedule kernel on synthetic masks -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 65, 130, 1025])
@pytest.mark.parametrize("S", [0, 5, 63])
def test_schedule_on_synthetic_masks(ctx, N, S):
    """densities per pair and lag from sparse to dense: with the dense ones delays reach S and vehicles stay unplaced.  Bit 0 is
    NOT symmetric here, so the schedule must read mask[v][u] for d >= d_u and mask[u][v] for d < d_u, as the rule says."""
    top = unplaced = 0
    densities = (0.0, 0.5, 0.9) if N <= 2 else (0.0, 0.3 / N, 2.0 / N, 0.2 if N < 1000 else 0.02)
    cases = [st.random_masks(N, S, density, 1000 * N + 10 * S + i, symmetric=False) for i, density in enumerate(densities)]
    # everybody conflicts with everybody on schedule (plus a little noise): the t-th vehicle gets delay t, up to S
    cases.append(st.random_masks(N, S, 0.2 / N, N + S) | (np.ones((N, N), dtype=np.uint64) - np.eye(N, dtype=np.uint64)))
    for i, m in enumerate(cases):
        orders = (None, np.random.default_rng(N + S + i).permutation(N))
        for order in orders if N < 1000 else orders[i % 2:][:1]:  # (the Python greedy takes seconds at N = 1025: one order each)
            want, wstats = st.greedy(m, S, order)
            got, gstats = ctx.schedule_starts(m, S, order)
            assert got.dtype == np.int32 and got.tolist() == want, (N, S, i)
            assert gstats == wstats, (N, S, i)
            top, unplaced = max(top, wstats["max_delay"]), unplaced + wstats["n_unplaced"]
    print(f"schedule N={N} S={S}: largest delay {top}, unplaced vehicles {unplaced}")
    if N >= 65:
        assert top == S and unplaced > 0


def test_schedule_rejects_a_non_permutation(ctx):
    import torch

    from path_planning import _hip

    N, S = 130, 5
    m = st.random_masks(N, S, 0.01, 5)
    good = np.random.default_rng(1).permutation(N)
    for bad in (np.where(good == 7, 8, good), np.where(good == 7, N, good), np.where(good == 7, -1, good)):
        with pytest.raises(_hip.HipError) as err:
            ctx.schedule_starts(m, S, bad)
        assert err.value.code == -1 and "permutation" in str(err.value)
    want, wstats = st.greedy(m, S, good)  # the context is still usable
    got, gstats = ctx.schedule_starts(m, S, good)
    assert got.tolist() == want and gstats == wstats
    dm = torch.as_tensor(m.view(np.int64)).to(ctx.tdev)
    delay = torch.zeros(N, dtype=torch.int32, device=ctx.tdev)
    stats = torch.zeros(48, dtype=torch.uint8, device=ctx.tdev)
    call = ctx.lib.scp_schedule_starts
    assert call(ctx.h, N, S, dm.data_ptr(), None, delay.data_ptr(), stats.data_ptr()) == 0
    assert call(ctx.h, N, 64, dm.data_ptr(), None, delay.data_ptr(), stats.data_ptr()) == -1
    assert call(ctx.h, N, -1, dm.data_ptr(), None, delay.data_ptr(), stats.data_ptr()) == -1
    assert call(ctx.h, 0, S, dm.data_ptr(), None, delay.data_ptr(), stats.data_ptr()) == -1
    assert call(ctx.h, 16385, S, dm.data_ptr(), None, delay.data_ptr(), stats.data_ptr()) == -1
    assert "scp_schedule_starts" in ctx.lib.scp_last_error(ctx.h).decode()
    for ptrs in ((None, delay.data_ptr(), stats.data_ptr()), (dm.data_ptr(), None, stats.data_ptr()), (dm.data_ptr(), delay.data_ptr(), None)):
        assert call(ctx.h, N, S, ptrs[0], None, ptrs[1], ptrs[2]) == -1
    assert call(None, N, S, dm.data_ptr(), None, delay.data_ptr(), stats.data_ptr()) == -1


# ---- 7. the schedule of the kernel's own masks -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(RANDOM)))
def test_schedule_of_the_kernels_masks(ctx, case):
    N, K, D, seed, S = RANDOM[case]
    dev, host, (want_mask, _) = random_case(ctx, N, K, D, seed, S)
    pos, vel, acc = dev
    mask = ctx.lag_conflicts(N, K, D, H, 0.8, pos, vel, acc, S, device=True)
    want, wstats = st.greedy(want_mask, S)
    assert wstats["n_unplaced"] == UNPLACED[case]
    got, gstats = ctx.schedule_starts(mask, S)
    assert got.tolist() == want and gstats == wstats
    if case == 0:  # a conflict-free case: all zeros
        assert got.tolist() == [0] * N and gstats["n_delayed"] == 0


# ---- 8. end to end on a half ring ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,D,seed,S,delays,before", RINGS)
def test_half_ring_end_to_end(ctx, N, K, D, seed, S, delays, before):
    from path_planning.solvers.stagger import staggered_fleet

    R = 0.5
    host = st.half_ring(N, K, D, seed, H)
    want_mask, ref = st.masks(*host, H, R, S)
    assert near_threshold(ref, 32 * sr.EPS * ref["s_max"] ** 2) == 0
    want, wstats = st.greedy(want_mask, S)
    assert want == delays and wstats["n_unplaced"] == 0
    dev = device(ctx, host)
    mask = ctx.lag_conflicts(N, K, D, H, R, *dev, S, device=True)
    assert (mask.cpu().numpy().view(np.uint64) == want_mask).all()
    got, gstats = ctx.schedule_starts(mask, S)
    assert got.tolist() == delays and gstats == wstats and gstats["n_unplaced"] == 0
    fleet = staggered_fleet(*host, H, got)
    assert fleet[0].shape == (N, K + max(delays), D)
    after = ctx.check_separation(N, K + max(delays), D, H, R, *device(ctx, fleet))
    stored = ctx.check_separation(N, K, D, H, R, *dev)
    print(f"half ring {N}x{K}x{D}: violating segments {stored['n_violating']} -> {after['n_violating']}, minimum distance "
          f"{stored['min_dist']:.4f} -> {after['min_dist']:.4f}")
    assert after["n_violating"] == 0 and stored["n_violating"] == before
    assert ctx.list_conflicts(N, K + max(delays), D, H, R, *device(ctx, fleet)).size == 0


# ---- 9. argument errors ---------------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    import torch

    from path_planning import _hip

    lib, hnd = ctx.lib, ctx.h
    N, K, D, R, S = 5, 4, 2, 0.8, 2
    dev, _, _ = random_case(ctx, N, K, D, 1)
    pp, vp, ap = (x.data_ptr() for x in dev)
    out = torch.zeros(N * N, dtype=torch.int64, device=ctx.tdev)
    o = out.data_ptr()
    call = lambda *x: lib.scp_lag_conflicts(*x)  # noqa: E731
    assert call(hnd, N, K, D, H, R, 0, N, S, pp, vp, ap, o) == 0
    assert call(hnd, N, K, D, H, R, 0, N, S, pp, vp, ap, None) == -1
    assert "scp_lag_conflicts" in lib.scp_last_error(hnd).decode()
    assert call(hnd, N, K, 4, H, R, 0, N, S, pp, vp, ap, o) == -1
    for a0, a1 in ((0, N + 1), (-1, N), (3, 2)):
        assert call(hnd, N, K, D, H, R, a0, a1, S, pp, vp, ap, o) == -1
        msg = lib.scp_last_error(hnd).decode()
        assert "scp_lag_conflicts" in msg and "bad vehicle range" in msg
    for lag in (-1, K + 1, 64):
        assert call(hnd, N, K, D, H, R, 0, N, lag, pp, vp, ap, o) == -1
        msg = lib.scp_last_error(hnd).decode()
        assert "scp_lag_conflicts" in msg and "bad lag range" in msg
    big = tuple(ctx.tensor(np.zeros((2, 70, 2))) for _ in range(3))  # K = 70: max_lag = 64 is within K but not within a word
    bp, bv, ba = (x.data_ptr() for x in big)
    assert call(hnd, 2, 70, 2, H, R, 0, 2, 64, bp, bv, ba, o) == -1 and "bad lag range" in lib.scp_last_error(hnd).decode()
    assert call(hnd, 2, 70, 2, H, R, 0, 2, 63, bp, bv, ba, o) == 0
    for ptrs in ((None, vp, ap), (pp, None, ap), (pp, vp, None)):
        assert call(hnd, N, K, D, H, R, 0, N, S, *ptrs, o) == -1
    for h in (0.0, float("inf"), float("nan")):
        assert call(hnd, N, K, D, h, R, 0, N, S, pp, vp, ap, o) == -1
    assert call(None, N, K, D, H, R, 0, N, S, pp, vp, ap, o) == -1
    assert call(hnd, N, K, D, H, R, 0, N, K, pp, vp, ap, o) == 0  # the context is still usable
    assert call(hnd, 1, K, D, H, R, 0, 1, S, pp, vp, ap, o) == 0  # N = 1: one zero word
    assert int(out.cpu().numpy()[0]) == 0
    ctx.lib.scp_ctx_synchronize(hnd)
    assert ctx.last_pair_ms() >= 0.0
    c = _hip.Context(0)
    try:
        with pytest.raises(_hip.HipError) as err:
            c.last_lag_solved()
        assert err.value.code == -4  # SCP_ERR_STATE: the call has not run on this context
    finally:
        c.close()


# ---- 10. the Python surface and the CLIs --------------------------------------------------------------------------------------------------
def ring_problem(N):
    ang = np.pi * np.arange(N) / N
    p0 = np.stack([10.0 + 5.0 * np.cos(ang), 10.0 + 5.0 * np.sin(ang)], axis=1)
    return p0, 20.0 - p0


def test_stagger_starts_surface():
    from path_planning.solvers.scp import SCP
    from path_planning.solvers.stagger import delays_satisfy_masks

    N = 8
    p0, pf = ring_problem(N)
    s = SCP(n_vehicles=N, time_horizon=10.0, time_step=0.5, min_distance=0.8, space_dims=[0, 0, 20, 20], device=0, verbose=False)
    with pytest.raises(ValueError):
        s.stagger_starts(3)  # no trajectories yet
    s.set_initial_states(p0)
    s.set_final_states(pf)
    s.generate_trajectories(max_iterations=0)  # QP#0: everybody straight through the centre
    stored = {k: v.copy() for k, v in s.trajectories.items()}
    S = min(s.K, 63)
    info = s.stagger_starts(S)
    assert info is s.last_info["stagger"]
    assert list(info) == ["delays", "scheduled", "n_delayed", "n_unplaced", "max_delay", "total_delay", "conflicts_before",
                          "conflicts_after", "min_distance_after", "horizon_steps", "lag_conflicts_ms", "schedule_ms", "time_sec"]
    print({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in info.items()})
    d = info["delays"]
    assert d.shape == (N,) and d.dtype == np.int64 and ((d >= -1) & (d <= S)).all()
    assert info["conflicts_before"] > 0 and info["n_delayed"] == int((d > 0).sum()) and info["n_unplaced"] == int((d < 0).sum())
    assert info["scheduled"] == (info["n_unplaced"] == 0) and info["max_delay"] == int(d.max())
    assert info["total_delay"] == int(d[d >= 0].sum()) and info["horizon_steps"] == s.K + max(int(d.max()), 0)
    if info["scheduled"]:
        assert info["conflicts_after"] == 0 and info["min_distance_after"] >= s.R - 0.01
    dev = tuple(s._ctx.tensor(stored[k]) for k in ("positions", "velocities", "accelerations"))
    mask = s._ctx.lag_conflicts(N, s.K, s.D, s.h, s.R, *dev, S)
    assert delays_satisfy_masks(mask, d) and st.satisfies(mask, d.tolist())
    assert d.tolist() == st.greedy(mask, S)[0]
    assert all(s.staggered[k].shape == (N, info["horizon_steps"], s.D) for k in ("positions", "velocities", "accelerations"))
    assert (s.staggered["delays"] == d).all()
    assert all(s.trajectories[k].tobytes() == stored[k].tobytes() for k in stored)  # the plans are left as they are
    order = np.arange(N)[::-1].copy()
    rev = s.stagger_starts(S, order=order)
    assert rev["delays"].tolist() == st.greedy(mask, S, order)[0] and rev["delays"][N - 1] == 0
    for bad in (-1, S + 1, 64, 2.0, True):
        with pytest.raises(ValueError):
            s.stagger_starts(bad)
    with pytest.raises(ValueError):
        s.stagger_starts(2, order=[0] * N)
    assert s.stagger_starts(0)["max_delay"] == 0


def test_batch_cli_stagger_starts(tmp_path):
    from path_planning.cli import compute_trajectories_batch as ctb

    def records(extra):
        out = tmp_path / ("with" if extra else "without")
        ctb.main(["--Ns", "4", "--trials", "2", "--seed", "5", "--results-dir", str(out)] + extra)
        return json.load(open(next(out.glob("*.json"))))["runs"]

    without, with_ = records([]), records(["--stagger-starts", "3"])
    fixed = ("N", "status", "error", "K", "T", "h", "seed", "trial_index")  # what does not depend on the run
    extra = ["stagger_max_delay", "stagger_n_delayed", "stagger_n_unplaced", "stagger_conflicts_after"]
    for a, b in zip(without, with_):
        assert a["status"] == b["status"] == "success"
        assert not any(k.startswith("stagger") for k in a)
        assert list(b) == list(a) + extra  # exactly the four fields, at the end
        assert all(a[k] == b[k] for k in fixed)
        assert all(isinstance(b[k], int) for k in extra) and 0 <= b["stagger_max_delay"] <= 3
        assert b["stagger_n_unplaced"] > 0 or b["stagger_conflicts_after"] == 0


def test_compute_trajectories_cli_stagger_starts(capsys):
    from path_planning.cli import compute_trajectories as ct

    args = ["--n-agents", "4", "--time-horizon", "10", "--time-step", "0.5", "--space", "0", "0", "20", "20", "--seed", "1",
            "--no-plots"]
    assert ct.main(args) is not None
    assert "Staggered starts:" not in capsys.readouterr().out
    solver = ct.main(args + ["--stagger-starts", "5"])
    out = capsys.readouterr().out
    line = [x for x in out.split("\n") if x.startswith("Staggered starts: ")]
    info = solver.last_info["stagger"]
    assert len(line) == 1 and f"{info['n_delayed']} of 4 vehicles delayed" in line[0]
    assert f"conflicting segments {info['conflicts_before']} -> {info['conflicts_after']}" in line[0]
    assert out.count(" steps (") - line[0].count(" steps (") == info["n_delayed"]  # one line per delayed vehicle
