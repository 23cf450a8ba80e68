"""GPU tests of the delay margins (scp_delay_margins) through the C-ABI and of their Python surface, against the numpy reference
of tests/delay_ref.py (pinned on the CPU by tests/test_delay_cpu.py) and, bit for bit, against scp_clearance_profile -- at lag 0
on the same device tensors, at every lag on the fleet shifted by hand.

Comparison rules, those of tests/test_clearance_gpu.py:
  TOL = 32 eps S_max^2 on f, S_max the largest |d| + h |w| + h^2/2 |b| over the tested segments, from the reference;
  per entry (a, s): |min_dist^2 - max(ref f, 0)| <= TOL; n_violating the reference's, where no segment of the entry has its
  reference f within TOL of (R - 0.01)^2.
A delay puts a kink into a trajectory at the instant the vehicle starts or parks, and a closest approach exactly at a kink
appears in two adjacent segments with values a rounding apart, so tied entries are part of the feature:
  DECIDED entries (the reference's two smallest minima more than TOL apart): (segment, partner) are the reference's, t_min within
  1e-6 h or f at both times within TOL;
  UNDECIDED entries: f at the reported (partner, segment, t_min) within TOL of the reference minimum.
The random cases keep the undecided entries below 6 % and have NO segment within TOL of the threshold (both asserted on the
reference before anything is asked of the kernel)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delay_ref as dr  # noqa: E402
import separation_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

H = 0.2
NONE32 = 2**32 - 1
RANDOM = [(2, 9, 2, 11, 9), (7, 13, 3, 12, 13), (65, 7, 2, 17, 7), (129, 7, 2, 17, 3), (130, 9, 3, 21, 4), (65, 50, 3, 16, 5)]
_CASES = {}


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def device(ctx, host):
    return tuple(ctx.tensor(np.ascontiguousarray(x)) for x in host)


def random_case(ctx, N, K, D, seed):
    """separation_ref.random_case as it is: host arrays, their device copies and a cache of references"""
    key = (N, K, D, seed)
    if key not in _CASES:
        p0, v0, acc = sr.random_case(N, K, D, seed)
        pos, vel = sr.kinematics(p0, v0, acc, H)
        host = (pos, vel, acc)
        _CASES[key] = (device(ctx, host), host, {})
    return _CASES[key]


def reference(case, R, S):
    dev, host, refs = case
    if (R, S) not in refs:
        refs[(R, S)] = dr.margins(*host, H, R, S)
    return refs[(R, S)]


def run(ctx, dev, R, S, a0=0, a1=None, h=H):
    pos, vel, acc = dev
    N, K, D = pos.shape
    return ctx.delay_margins(N, K, D, h, R, pos, vel, acc, S, a0, a1)


def total_segments(N, K, S, n_a=None):
    return (N if n_a is None else n_a) * (N - 1) * sum(K + s for s in range(S + 1))


def is_empty(e):
    return (np.isposinf(e["min_dist"]) & (e["t_min"] == 0.0) & (e["partner"] == NONE32) & (e["segment"] == NONE32)
            & (e["n_violating"] == 0))


def near_threshold(ref, tol):
    """(a, s, g, b) of every segment whose reference f lies within tol of (R - 0.01)^2"""
    out = []
    for a, f in ref["seg_f"].items():
        out += [(a, int(s), int(g), int(b)) for s, g, b in zip(*np.nonzero(np.abs(f - ref["thr"] ** 2) <= tol))]
    return out


def compare(got, ref, host, label, undecided=(), h=H):
    """the (vehicles, S + 1) result against the reference by the rules of the module docstring; `undecided`: the (a, s, g, b) of
    segments within TOL of the threshold -- their entries get the range of counts instead.  -> the number of undecided entries"""
    pos = host[0]
    N, K, D = pos.shape
    n_a, lags = got.shape
    tol = 32 * sr.EPS * ref["s_max"] ** 2
    P, V, A = dr.records(*host, h)

    def f_at(a, s, b, g, t):
        ra, rb = max(g - s, -1) + 1, min(g, K) + 1
        d, w, bb = P[a, ra] - P[b, rb], V[a, ra] - V[b, rb], A[a, ra] - A[b, rb]
        return float(((d + t * w + 0.5 * t * t * bb) ** 2).sum())

    err = np.abs(got["min_dist"] ** 2 - np.maximum(ref["f"], 0.0))
    print(f"{label}: {got.size} entries, max |min_dist^2 - ref| = {err.max() / max(sr.EPS * ref['s_max'] ** 2, 1e-300):.2f} "
          f"eps S_max^2 (bound 32), violating entries {int((got['n_violating'] > 0).sum())}")
    und = np.zeros(got.shape, dtype=np.int64)
    for a, s, _, _ in undecided:
        und[a, s] += 1
    tied = 0
    for a in range(n_a):
        for s in range(lags):
            e = got[a, s]
            assert err[a, s] <= tol, (label, a, s)
            g, b, t = int(e["segment"]), int(e["partner"]), float(e["t_min"])
            assert 0 <= g < K + s and 0 <= b < N and b != a and 0.0 <= t <= h, (label, a, s)  # the structure
            if ref["second_f"][a, s] - ref["f"][a, s] > tol:
                assert (g, b) == (int(ref["g"][a, s]), int(ref["b"][a, s])), (label, a, s)
                if abs(t - ref["t"][a, s]) > 1e-6 * h:  # a flat f: the values decide
                    assert abs(f_at(a, s, b, g, t) - ref["f"][a, s]) <= tol, (label, a, s)
            else:
                tied += 1
                assert abs(f_at(a, s, b, g, t) - ref["f"][a, s]) <= tol, (label, a, s)
            if und[a, s]:
                lo, hi = int(ref["n_violating"][a, s]) - int(und[a, s]), int(ref["n_violating"][a, s]) + int(und[a, s])
                assert lo <= int(e["n_violating"]) <= hi, (label, a, s)
            else:
                assert int(e["n_violating"]) == int(ref["n_violating"][a, s]), (label, a, s)
    return tied


# ---- 1. random trajectories against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,D,seed,S", RANDOM)
def test_random_trajectories_vs_reference(ctx, N, K, D, seed, S):
    R = 0.8
    case = random_case(ctx, N, K, D, seed)
    dev, host, _ = case
    ref = reference(case, R, S)
    tol = 32 * sr.EPS * ref["s_max"] ** 2
    # conditions on the INPUTS, not on the kernel
    tied = int((ref["second_f"] - ref["f"] <= tol).sum())
    near = near_threshold(ref, tol)
    print(f"random {N}x{K}x{D} S={S}: undecided entries {tied} of {ref['f'].size} ({int((ref['second_f'][:, 0] - ref['f'][:, 0] <= tol).sum())} at "
          f"lag 0), segments within TOL of the threshold {len(near)}, violating (b, g) {int(ref['n_violating'].sum())}")
    assert tied <= 0.06 * ref["f"].size and not near
    got = run(ctx, dev, R, S)
    assert got.shape == (N, S + 1)
    assert compare(got, ref, host, f"delay {N}x{K}x{D} S={S}") == tied
    solved = ctx.last_delay_solved()
    print(f"random {N}x{K}x{D} S={S}: {solved} of {total_segments(N, K, S)} segments reached the quartic")
    assert 0 < solved <= total_segments(N, K, S)
    assert run(ctx, dev, R, S).tobytes() == got.tobytes()  # a second run: the same bytes


# ---- 2. lag 0 is the clearance profile, bit for bit ---------------------------------------------------------------------------------
def row_of(N, a, b, g):
    i, j = min(a, b), max(a, b)
    return g * (N * (N - 1) // 2) + i * N - i * (i + 1) // 2 + (j - i - 1)


def assert_entry_is_clearance(e, a, veh, N, label):
    """one delay entry of vehicle a against the clearance entry of the same fleet: the values as bytes, (segment, partner)
    folded through the row"""
    bits = lambda x: np.float64(x).tobytes()  # noqa: E731
    assert (bits(e["min_dist"]), bits(e["t_min"]), int(e["n_violating"])) == (
        bits(veh["min_dist"]), bits(veh["t_min"]), int(veh["n_violating"])), label
    assert row_of(N, a, int(e["partner"]), int(e["segment"])) == int(veh["row"]), label


@pytest.mark.parametrize("N,K,D,seed", [(129, 7, 2, 17), (65, 50, 3, 16)])
def test_lag_0_is_the_clearance_profile_bit_for_bit(ctx, N, K, D, seed):
    R = 0.8
    dev, host, _ = random_case(ctx, N, K, D, seed)
    got = run(ctx, dev, R, 2)
    veh, _ = ctx.clearance_profile(N, K, D, H, R, *dev)
    for a in range(N):
        assert_entry_is_clearance(got[a, 0], a, veh[a], N, (N, K, D, a))
    assert int(got["n_violating"][:, 0].sum()) > 0  # the counts are not trivially equal


# ---- 3. a delay is a shifted fleet, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,D,seed,vehicles", [(7, 13, 3, 12, None), (65, 7, 2, 17, (0, 63, 64, 64)), (130, 9, 3, 21, (0, 63, 64, 129))])
def test_delay_is_the_clearance_profile_of_the_shifted_fleet(ctx, N, K, D, seed, vehicles):
    R = 0.8
    dev, host, _ = random_case(ctx, N, K, D, seed)
    got = run(ctx, dev, R, K)
    pos, vel, acc = host
    pK = pos[:, K - 1] + (H * vel[:, K - 1] + (0.5 * H * H) * acc[:, K - 1])  # the header's formula
    checked = 0
    for a in sorted(set(range(N) if vehicles is None else vehicles)):
        for s in range(K + 1):
            fleet = [np.concatenate([x, np.repeat(tail[:, None], s, axis=1)], axis=1)
                     for x, tail in ((pos, pK), (vel, np.zeros_like(pK)), (acc, np.zeros_like(pK)))]
            fleet[0][a] = np.concatenate([np.repeat(pos[a, :1], s, axis=0), pos[a]])
            fleet[1][a] = np.concatenate([np.zeros((s, D)), vel[a]])
            fleet[2][a] = np.concatenate([np.zeros((s, D)), acc[a]])
            veh, _ = ctx.clearance_profile(N, K + s, D, H, R, *device(ctx, fleet))
            assert_entry_is_clearance(got[a, s], a, veh[a], N, (N, K, D, a, s))
            checked += 1
    print(f"shifted fleet {N}x{K}x{D}: {checked} entries equal to the clearance profile bit for bit")
    assert checked == (N if vehicles is None else len(set(vehicles))) * (K + 1)


# ---- 4. the crossing case -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,pair", [(2, 2, (0, 1)), (6, 2, (2, 4)), (7, 3, (3, 6))])
def test_crossing_case(ctx, N, D, pair):
    host = dr.crossing_case(N, D, pair)
    h, R, S = dr.CROSS_H, dr.CROSS_R, 6
    a, b = pair
    ref = dr.margins(*host, h, R, S)
    tol = 32 * sr.EPS * ref["s_max"] ** 2
    assert not near_threshold(ref, tol)
    got = run(ctx, device(ctx, host), R, S, h=h)
    print(f"crossing N={N} D={D}: margins {got['min_dist'][a]}, counts {got['n_violating'][a]}")
    for s in range(S + 1):
        e = got[a, s]
        assert abs(e["min_dist"] - dr.crossing_margin(s)) <= 1e-12
        assert int(e["partner"]) == b and int(e["n_violating"]) == int(ref["n_violating"][a, s])
        assert abs(int(e["segment"]) * h + e["t_min"] - (1.1 + 0.1 * s)) <= 1e-6  # halfway between the two passages
        assert abs(got["min_dist"][b, s] - 0.2 * np.sqrt(2.0) * (3 + s)) <= 1e-12 and int(got["partner"][b, s]) == a
    assert (got["n_violating"][a] > 0).tolist() == [False, False, True, True, True, False, False]
    compare(got, ref, host, f"crossing N={N} D={D}", h=h)  # partner and segment wherever the reference decides them


# ---- 5. degenerate records in interior tiles --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,D", [(300, 4, 2), (200, 3, 3)])
def test_degenerate_records_in_interior_tiles(ctx, N, K, D):
    """the construction of test_clearance_gpu.test_degenerate_segments_in_interior_tiles, delayed by up to two steps.  Most
    vehicles are at rest throughout: their held, stored and parked records coincide, and the equal distances of the grid tie
    bitwise -- such ties, and the exact zeros of the coincident pair, go to the smallest (g, b).  The pair touching exactly at
    the threshold is undecided by construction: its segments are the only ones within TOL of the threshold (asserted)."""
    R, S = 0.8, 2
    pos = np.zeros((N, K, D))
    vel = np.zeros((N, K, D))
    acc = np.zeros((N, K, D))
    side = int(np.ceil(np.sqrt(N)))
    pos[:, :, 0] = 10.0 * (np.arange(N) % side)[:, None]
    pos[:, :, 1] = 10.0 * (np.arange(N) // side)[:, None]
    e0 = np.zeros(D); e0[0] = 1.0
    e1 = np.zeros(D); e1[1] = 1.0
    a = N // 2 + 3
    pos[a + 1] = pos[a]                                             # coincident throughout: d = w = b = 0
    pos[a + 3] = pos[a + 2] + 1.0 * e0; vel[a + 3] = -1.5 * e0      # b = 0: f' linear
    pos[a + 5] = pos[a + 4] + 0.9 * e0 + 0.25 * e1                  # b = w = 0: f constant
    pos[a + 7] = pos[a + 6] + 1.0 * e0; acc[a + 7] = 8.0 * e0       # b parallel to d, w = 0: root of f' exactly at t = 0
    pos[a + 9] = pos[a + 8] + 1.0 * e0; vel[a + 9] = -1.0 * e0; acc[a + 9] = (1.0 / H) * e0  # w + h b = 0: root exactly at t = h
    pos[a + 11] = pos[a + 10] + (R - 0.01) * e0                     # touching exactly at the threshold, at rest
    pos[a + 13] = pos[a + 12] + 0.85 * e0; vel[a + 13] = -0.5 * e0; acc[a + 13] = 2.5 * e0  # b parallel to w: dips to 0.8 and back
    host = (pos, vel, acc)
    ref = dr.margins(*host, H, R, S)
    tol = 32 * sr.EPS * ref["s_max"] ** 2
    undecided = near_threshold(ref, tol)
    touching = [(x, s, g, y) for x, y in ((a + 10, a + 11), (a + 11, a + 10)) for s in range(S + 1) for g in range(K + s)]
    assert sorted(undecided) == sorted(touching)
    got = run(ctx, device(ctx, host), R, S)
    for v, w in ((a, a + 1), (a + 1, a)):
        for s in range(S + 1):
            e = got[v, s]
            assert e["min_dist"] == 0.0 and e["t_min"] == 0.0 and (int(e["segment"]), int(e["partner"])) == (0, w)
            assert int(e["n_violating"]) >= K + s
    compare(got, ref, host, f"delay degenerate {N}x{K}x{D}", undecided)
    grid_tie = (ref["f"] == 100.0) & (ref["second_f"] == 100.0)  # at rest on the grid, two neighbours 10 m away
    assert grid_tie[:, 0].sum() > N // 2 and grid_tie[70].all()  # vehicle 70's smallest partner lies in another tile
    assert (got["segment"][grid_tie] == 0).all() and (got["partner"][grid_tie] == ref["b"][grid_tie]).all()
    assert (got["min_dist"][grid_tie] == 10.0).all() and (got["t_min"][grid_tie] == 0.0).all()


# ---- 6. vehicle ranges ------------------------------------------------------------------------------------------------------------------
def raw_call(ctx, dev, R, S, a0, a1, out, h=H):
    pos, vel, acc = dev
    N, K, D = pos.shape
    return ctx.lib.scp_delay_margins(ctx.h, N, K, D, h, R, a0, a1, S, pos.data_ptr(), vel.data_ptr(), acc.data_ptr(),
                                     out.data_ptr() if out is not None else None)


def test_vehicle_ranges_concatenate_to_the_full_result(ctx):
    import torch

    N, K, D, seed, S, R = 130, 9, 3, 21, 4, 0.8
    dev, host, _ = random_case(ctx, N, K, D, seed)
    full = run(ctx, dev, R, S)
    cuts = [0, 1, 63, 64, 65, 129, 130]
    parts = [run(ctx, dev, R, S, x, y) for x, y in zip(cuts[:-1], cuts[1:])]
    assert [p.shape for p in parts] == [(y - x, S + 1) for x, y in zip(cuts[:-1], cuts[1:])]
    assert b"".join(p.tobytes() for p in parts) == full.tobytes()
    assert run(ctx, dev, R, S, 64, 64).shape == (0, S + 1)
    poison = torch.full((64,), 0xA5, dtype=torch.uint8, device=ctx.tdev)
    assert raw_call(ctx, dev, R, S, 5, 5, poison) == 0 and raw_call(ctx, dev, R, S, N, N, poison) == 0
    assert (poison.cpu().numpy() == 0xA5).all()  # an empty range writes nothing
    assert ctx.last_delay_solved() == 0
    assert run(ctx, dev, R, 0).tobytes() == np.ascontiguousarray(full[:, :1]).tobytes()
    whole = run(ctx, dev, R, K)
    assert whole.shape == (N, K + 1) and np.ascontiguousarray(whole[:, :S + 1]).tobytes() == full.tobytes()
    assert not is_empty(whole).any() and (whole["segment"] < K + np.arange(K + 1)[None, :]).all()
    # how the call cuts lags and segments into workgroups does not show either
    run(ctx, dev, R, S)
    n_auto = ctx.last_delay_solved()
    try:
        for lc, gc in ((3, 5), (5, 1), (1, 13), (2, 4)):
            ctx.set_option("delay_lag_chunk", lc)
            ctx.set_option("delay_time_chunk", gc)
            assert run(ctx, dev, R, S).tobytes() == full.tobytes(), (lc, gc)
            assert 0 < ctx.last_delay_solved() <= total_segments(N, K, S)
            assert run(ctx, dev, R, S, 63, 65).tobytes() == np.ascontiguousarray(full[63:65]).tobytes(), (lc, gc)
    finally:
        ctx.set_option("delay_lag_chunk", 0)
        ctx.set_option("delay_time_chunk", 0)
    assert run(ctx, dev, R, S).tobytes() == full.tobytes() and ctx.last_delay_solved() == n_auto


# ---- 7. argument errors -----------------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    import torch

    from path_planning import _hip

    lib, hnd = ctx.lib, ctx.h
    N, K, D, R, S = 5, 4, 2, 0.8, 2
    dev, _, _ = random_case(ctx, N, K, D, 1)
    pp, vp, ap = (x.data_ptr() for x in dev)
    out = torch.zeros(N * (K + 1) * 32, dtype=torch.uint8, device=ctx.tdev)
    o = out.data_ptr()
    call = lambda *x: lib.scp_delay_margins(*x)  # noqa: E731
    assert call(hnd, N, K, D, H, R, 0, N, S, pp, vp, ap, o) == 0
    assert call(hnd, N, K, D, H, R, 0, N, S, pp, vp, ap, None) == -1
    assert "scp_delay_margins" in lib.scp_last_error(hnd).decode()
    assert call(hnd, N, K, 4, H, R, 0, N, S, pp, vp, ap, o) == -1
    for a0, a1 in ((0, N + 1), (-1, N), (3, 2)):
        assert call(hnd, N, K, D, H, R, a0, a1, S, pp, vp, ap, o) == -1
        msg = lib.scp_last_error(hnd).decode()
        assert "scp_delay_margins" in msg and "bad vehicle range" in msg
    for lag in (-1, K + 1):
        assert call(hnd, N, K, D, H, R, 0, N, lag, pp, vp, ap, o) == -1
        msg = lib.scp_last_error(hnd).decode()
        assert "scp_delay_margins" in msg and "bad lag range" in msg
    for ptrs in ((None, vp, ap), (pp, None, ap), (pp, vp, None)):
        assert call(hnd, N, K, D, H, R, 0, N, S, *ptrs, o) == -1
    for h in (0.0, float("inf"), float("nan")):
        assert call(hnd, N, K, D, h, R, 0, N, S, pp, vp, ap, o) == -1
    assert call(None, N, K, D, H, R, 0, N, S, pp, vp, ap, o) == -1
    assert call(hnd, N, K, D, H, R, 0, N, K, pp, vp, ap, o) == 0  # the context is still usable
    assert not is_empty(out.cpu().numpy().view(_hip.DELAY_DTYPE)).any()
    assert call(hnd, 1, K, D, H, R, 0, 1, S, pp, vp, ap, o) == 0    # N = 1: no pair, every entry empty
    assert is_empty(out.cpu().numpy().view(_hip.DELAY_DTYPE)[:S + 1]).all()
    ctx.lib.scp_ctx_synchronize(hnd)
    assert ctx.last_pair_ms() >= 0.0
    c = _hip.Context(0)
    try:
        with pytest.raises(_hip.HipError) as err:
            c.last_delay_solved()
        assert err.value.code == -4  # SCP_ERR_STATE: the call has not run on this context
    finally:
        c.close()


# ---- 8. the Python surface ----------------------------------------------------------------------------------------------------------------
def test_validate_solution_delay(tmp_path):
    from path_planning.solvers.scp import SCP
    from path_planning.viz.plot_trajectories import plot_delay_margin

    p0, pf = np.array([[2.0, 10.0], [18.0, 10.0]]), np.array([[18.0, 10.0], [2.0, 10.0]])
    s = SCP(n_vehicles=2, time_horizon=10.0, time_step=0.5, min_distance=0.8, space_dims=[0, 0, 20, 20], device=0, verbose=False)
    s.set_initial_states(p0)
    s.set_final_states(pf)
    s.generate_trajectories(max_iterations=15)
    S = 6
    plain = s.validate_solution(continuous=True)
    rep = s.validate_solution(continuous=True, delay=S)
    assert list(rep) == list(plain) + ["delay_margin", "delay_tolerance", "least_tolerant_vehicle"]
    assert {k: rep[k] for k in plain} == plain
    assert s.validate_solution(continuous=True, delay=None) == plain
    dm, dt, lt = rep["delay_margin"], rep["delay_tolerance"], rep["least_tolerant_vehicle"]
    assert list(dm) == ["min_distance", "time", "partner", "n_violating_segments"]
    assert list(dt) == ["steps", "seconds", "limited_by"]
    assert all(dm[k].shape == (s.N, S + 1) for k in dm) and all(dt[k].shape == (s.N,) for k in dt)
    both = s.validate_solution(continuous=True, clearance=True, delay=S)
    assert list(both) == list(plain) + ["vehicle_clearance", "step_clearance", "most_exposed_vehicle", "delay_margin",
                                        "delay_tolerance", "least_tolerant_vehicle"]
    assert dm["min_distance"][:, 0].tobytes() == both["vehicle_clearance"]["min_distance"].tobytes()  # lag 0, bit for bit
    assert (dm["time"][:, 0] == both["vehicle_clearance"]["time"]).all()
    assert dm["partner"].tolist() == [[1] * (S + 1), [0] * (S + 1)]
    print(dm["min_distance"], dt, lt)
    for v in range(s.N):  # steps is consistent with the counts
        bad = dm["n_violating_segments"][v] > 0
        steps = int(dt["steps"][v])
        assert -1 <= steps <= S and not bad[:steps + 1].any() and (steps == S or bad[steps + 1])
        assert dt["seconds"][v] == steps * s.h
        assert int(dt["limited_by"][v]) == (-1 if steps == S else 1 - v)
    assert list(lt) == ["vehicle", "steps", "seconds", "partner", "time", "distance"]
    v = lt["vehicle"]
    assert v == int(np.argmin(dt["steps"])) and lt["steps"] == int(dt["steps"][v]) and lt["seconds"] == lt["steps"] * s.h
    at = min(lt["steps"] + 1, S)
    assert (lt["partner"], lt["time"], lt["distance"]) == (1 - v, float(dm["time"][v, at]), float(dm["min_distance"][v, at]))
    for kw in ({"delay": 2}, {"continuous": False, "delay": 2}):
        with pytest.raises(ValueError):
            s.validate_solution(**kw)
    for bad in (-1, s.K + 1, 2.0, True):
        with pytest.raises(ValueError):
            s.validate_solution(continuous=True, delay=bad)
    assert s.validate_solution(continuous=True, delay=s.K)["delay_margin"]["min_distance"].shape == (2, s.K + 1)
    path = str(tmp_path / "delay.pdf")
    plot_delay_margin(s, S, path)
    assert os.path.getsize(path) > 0


def test_batch_cli_delay_tolerance(tmp_path):
    import json

    from path_planning.cli import compute_trajectories_batch as ctb

    def records(extra):
        out = tmp_path / ("with" if extra else "without")
        ctb.main(["--Ns", "4", "--trials", "2", "--seed", "5", "--results-dir", str(out)] + extra)
        return json.load(open(next(out.glob("*.json"))))["runs"]

    without, with_ = records([]), records(["--delay-tolerance", "3"])
    fixed = ("N", "status", "error", "K", "T", "h", "seed", "trial_index")  # what does not depend on the run
    for a, b in zip(without, with_):
        assert a["status"] == b["status"] == "success"
        extra = ["delay_tolerance_steps", "min_delay_tolerance_steps"]
        assert list(b) == list(a) + extra  # exactly the two fields, at the end
        print({k: (a[k], b[k]) for k in a if a[k] != b[k]})  # wall clock and the solver's last bits
        assert all(a[k] == b[k] for k in fixed)
        steps = b["delay_tolerance_steps"]
        assert len(steps) == b["N"] and all(isinstance(x, int) and -1 <= x <= 3 for x in steps)
        assert isinstance(b["min_delay_tolerance_steps"], int) and b["min_delay_tolerance_steps"] == min(steps)


def test_compute_trajectories_cli_delay_tolerance(capsys, tmp_path):
    from path_planning.cli import compute_trajectories as ct

    args = ["--n-agents", "4", "--time-horizon", "10", "--time-step", "0.5", "--space", "0", "0", "20", "20", "--seed", "1"]
    prefix0 = str(tmp_path / "plain")
    assert ct.main(args + ["--save-prefix", prefix0]) is not None
    assert "Delay tolerance:" not in capsys.readouterr().out and not os.path.exists(prefix0 + "_delay.pdf")
    solver = ct.main(args + ["--no-plots", "--delay-tolerance", "5"])
    out = capsys.readouterr().out
    lt = solver.validate_solution(continuous=True, delay=5)["least_tolerant_vehicle"]
    line = [x for x in out.split("\n") if x.startswith("Delay tolerance: ")]
    assert len(line) == 1 and "Continuous-time check: minimum distance" in out  # implies --continuous-check
    assert f"vehicle {lt['vehicle']} " in line[0] and f"vehicle {lt['partner']} " in line[0]
    assert f"{lt['distance']:.4f} m" in line[0] and f"t = {lt['time']:.4f} s" in line[0]
    if lt["steps"] >= 0:
        assert f"{lt['steps']} steps ({lt['seconds']:.2f} s)" in line[0]
    prefix = str(tmp_path / "demo")
    assert ct.main(args + ["--delay-tolerance", "5", "--save-prefix", prefix]) is not None
    assert os.path.getsize(prefix + "_delay.pdf") > 0
