"""GPU tests of the clearance profile (scp_clearance_profile) through the C-ABI and of its Python surface, against the numpy
reference of tests/clearance_ref.py (pinned on the CPU by tests/test_clearance_cpu.py) and, bit for bit, against
scp_check_separation, scp_check_avoidance and scp_list_conflicts on the same device data.

Comparison rules, those of tests/test_separation_gpu.py (TOL is derived there):
  TOL = 32 eps S_max^2 on f, S_max the largest |d| + h |w| + h^2/2 |b| over the tested segments, from the reference;
  per entry: |min_dist^2 - max(ref f, 0)| <= TOL; the reference's row where its two smallest minima are more than TOL apart;
  t_min within 1e-6 h, or f at both times within TOL; n_violating the reference's, where no segment of the entry has its
  reference f within TOL of (R - 0.01)^2; sample_min_dist within 8 eps (relative) of numpy's norm -- both sides make at most
  D <= 3 rounded additions and one root.
The random cases are chosen so that NO entry has its two smallest minima within TOL and NO segment is within TOL of the
threshold (asserted on the reference before anything is asked of the kernel): there every row and every count is exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clearance_ref as clr  # noqa: E402
import conflicts_ref as cr  # noqa: E402
import separation_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

H = 0.2
NO_ROW = 2**64 - 1
RANDOM = [(2, 9, 2, 11), (7, 13, 3, 12), (65, 50, 3, 16), (129, 7, 2, 17), (300, 4, 2, 31), (200, 50, 2, 32)]
_CASES = {}


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def random_case(ctx, N, K, D, seed):
    """device tensors (through scp_kinematics, as the separation tests), their host copies and a cache of references"""
    key = (N, K, D, seed)
    if key not in _CASES:
        p0, v0, acc = sr.random_case(N, K, D, seed)
        a = ctx.tensor(acc)
        pos, vel = ctx.kinematics(N, K, D, H, a, ctx.tensor(p0), ctx.tensor(v0))
        _CASES[key] = ((pos, vel, a), (pos.cpu().numpy(), vel.cpu().numpy(), acc), {})
    return _CASES[key]


def reference(case, R):
    dev, host, refs = case
    if R not in refs:
        refs[R] = clr.profile(*host, H, R)
    return refs[R]


def device(ctx, host):
    return tuple(ctx.tensor(x) for x in host)


def run(ctx, dev, R, q0=0, q1=None):
    pos, vel, acc = dev
    N, K, D = pos.shape
    return ctx.clearance_profile(N, K, D, H, R, pos, vel, acc, q0, q1)


def is_empty(e):
    return (np.isposinf(e["min_dist"]) & (e["t_min"] == 0.0) & (e["row"] == NO_ROW) & np.isposinf(e["sample_min_dist"])
            & (e["n_violating"] == 0) & (e["reserved"] == 0))


def f_at(host, row, t):
    d, w, b = cr.segment_of_row(host, row)
    return float(((d + t * w + 0.5 * t * t * b) ** 2).sum())


def compare(got, ref_e, ref, host, label, undecided_rows=()):
    """one profile (structured array) against the reference's entry arrays, by the rules of the module docstring; entries
    that cover a row of `undecided_rows` (reference f within TOL of the threshold) get the range of counts instead"""
    tol = 32 * sr.EPS * ref["s_max"] ** 2
    pairs = ref["pairs"]
    N = host[0].shape[0]
    i, j = sr.pair_indices(N)
    by_vehicle = got.size == N and label.startswith("vehicle")
    err = np.abs(got["min_dist"] ** 2 - np.maximum(ref_e["f"], 0.0))
    covered = ref_e["n_rows"] > 0
    print(f"{label}: {got.size} entries ({int(covered.sum())} cover rows), max |min_dist^2 - ref| = "
          f"{(err[covered].max() if covered.any() else 0.0) / max(sr.EPS * ref['s_max'] ** 2, 1e-300):.2f} eps S_max^2 (bound 32), "
          f"violating entries {int((got['n_violating'] > 0).sum())}")
    assert is_empty(got[~covered]).all()
    assert (got["reserved"] == 0).all()
    und = np.zeros(got.size, dtype=np.int64)
    for r in undecided_rows:
        k, q = divmod(int(r), pairs)
        if by_vehicle:
            und[i[q]] += 1
            und[j[q]] += 1
        else:
            und[k] += 1
    for e in np.nonzero(covered)[0]:
        g = got[e]
        assert err[e] <= tol, (label, e)
        row = int(g["row"])
        k, q = divmod(row, pairs)
        assert (e in (i[q], j[q])) if by_vehicle else (k == e), (label, e, row)  # the structure
        assert 0.0 <= g["t_min"] <= H
        if ref_e["second_f"][e] - ref_e["f"][e] > tol:
            assert row == int(ref_e["row"][e]), (label, e)
            if abs(g["t_min"] - ref_e["t"][e]) > 1e-6 * H:  # a flat f: the values decide
                assert abs(f_at(host, row, g["t_min"]) - ref_e["f"][e]) <= tol, (label, e)
        else:
            assert abs(f_at(host, row, g["t_min"]) - ref_e["f"][e]) <= tol, (label, e)
        if und[e]:
            viol_lo = int(ref_e["n_violating"][e]) - int(und[e])
            assert viol_lo <= int(g["n_violating"]) <= int(ref_e["n_violating"][e]) + int(und[e]), (label, e)
        else:
            assert int(g["n_violating"]) == int(ref_e["n_violating"][e]), (label, e)
        assert abs(g["sample_min_dist"] - ref_e["sample"][e]) <= 8 * sr.EPS * ref_e["sample"][e], (label, e)
        assert g["min_dist"] <= g["sample_min_dist"] * (1 + 4 * sr.EPS)  # sqrt(d.d) and pair_geom's root: an ulp apart


# ---- 1. the tunnelling pair ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,pair", [(2, 2, (0, 1)), (6, 2, (2, 4)), (7, 3, (3, 6))])
def test_tunnelling_pair(ctx, N, D, pair):
    pos, vel, acc, row = cr.tunnelling_case(N, D, pair)
    veh, step = run(ctx, device(ctx, (pos, vel, acc)), 0.3)
    print(f"tunnel N={N} D={D}: vehicles {veh}\nsteps {step}")
    tol = 32 * sr.EPS * 1.2 ** 2  # S = 0.4 + h 4
    for v, partner in (pair, pair[::-1]):
        g = veh[v]
        assert abs(g["sample_min_dist"] - 0.4) < 1e-12 and g["min_dist"] ** 2 <= tol and g["n_violating"] == 1
        assert int(g["row"]) == row and abs(g["t_min"] - 0.1) <= 1e-6 * H  # segment 3, against the partner
    others = np.setdiff1d(np.arange(N), pair)
    assert (veh["n_violating"][others] == 0).all()
    # The other vehicles are at rest, but the two of the pair keep moving: a vehicle whose nearest neighbour is one of them
    # has its closest approach at the END of the last segment, which is no sample.  So: everything against the reference,
    # and min_dist equal to sample_min_dist (to the ulp between sqrt and pair_geom's root) where the reference's closest
    # approach is at a sample
    host = (pos, vel, acc)
    ref = clr.profile(pos, vel, acc, H, 0.3)
    compare(veh, ref["vehicle"], ref, host, f"vehicle tunnel N={N}")
    compare(step, ref["step"], ref, host, f"step tunnel N={N}")
    at_sample = others[ref["vehicle"]["t"][others] == 0.0]
    assert N == 2 or at_sample.size > 0
    assert (np.abs(veh["min_dist"][at_sample] - veh["sample_min_dist"][at_sample]) <= 4 * sr.EPS * veh["sample_min_dist"][at_sample]).all()
    assert step["n_violating"].tolist() == [1 if k == 3 else 0 for k in range(step.size)]
    assert int(step["row"][3]) == row and step["min_dist"][3] ** 2 <= tol
    assert (step["min_dist"][np.arange(step.size) != 3] >= 0.4 - 1e-12).all()


# ---- 2. random trajectories against the reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,D,seed", RANDOM)
def test_random_trajectories_vs_reference(ctx, N, K, D, seed):
    R = 0.8
    case = random_case(ctx, N, K, D, seed)
    dev, host, _ = case
    ref = reference(case, R)
    tol = 32 * sr.EPS * ref["s_max"] ** 2
    # conditions on the INPUTS, not on the kernel: every row and every count of the reference is decided
    close = sum(int((e["second_f"] - e["f"] <= tol).sum()) for e in (ref["vehicle"], ref["step"]))
    near_thr = int((np.abs(ref["f"] - ref["thr"] ** 2) <= tol).sum())
    print(f"random {N}x{K}x{D}: entries with two minima within TOL {close}, segments within TOL of the threshold {near_thr}, "
          f"violations {int(ref['step']['n_violating'].sum())}")
    assert close == 0 and near_thr == 0
    veh, step = run(ctx, dev, R)
    compare(veh, ref["vehicle"], ref, host, f"vehicle {N}x{K}x{D}")
    compare(step, ref["step"], ref, host, f"step {N}x{K}x{D}")
    solved = ctx.last_clearance_solved()
    print(f"random {N}x{K}x{D}: {solved} of {K * N * (N - 1) // 2} segments reached the quartic")
    assert 0 < solved <= K * N * (N - 1) // 2
    veh2, step2 = run(ctx, dev, R)
    assert veh2.tobytes() == veh.tobytes() and step2.tobytes() == step.tobytes()  # a second run: the same bytes


# ---- 3. exact ties to the existing entry points, on the same device data ----------------------------------------------------------
def lexmin(e):
    k = np.lexsort((e["row"], e["min_dist"]))[0]
    return e[k]


@pytest.mark.parametrize("N,K,D,seed", [(129, 7, 2, 17), (65, 50, 3, 16)])
def test_bitwise_ties_to_check_avoidance_and_list(ctx, N, K, D, seed):
    R = 0.8
    dev, host, _ = random_case(ctx, N, K, D, seed)
    pos, vel, acc = dev
    pairs = N * (N - 1) // 2
    veh, step = run(ctx, dev, R)
    st = ctx.check_separation(N, K, D, H, R, pos, vel, acc)
    smin = ctx.check_avoidance(N, K, D, R, pos)[0]
    recs = ctx.list_conflicts(N, K, D, H, R, pos, vel, acc)
    bits = lambda x: np.float64(x).tobytes()  # noqa: E731
    for e in (veh, step):
        best = lexmin(e)
        assert bits(best["min_dist"]) == bits(st["min_dist"]) and int(best["row"]) == st["argmin_row"]
        assert bits(best["t_min"]) == bits(st["argmin_t"])
        assert bits(e["sample_min_dist"].min()) == bits(st["sample_min_dist"]) == bits(smin)
    assert int(step["n_violating"].sum()) == st["n_violating"] and int(veh["n_violating"].sum()) == 2 * st["n_violating"]
    assert recs.size == st["n_violating"] and recs.size > 0
    i, j = sr.pair_indices(N)
    rk, rq = np.divmod(recs["row"].astype(np.int64), pairs)
    checked = 0
    for e, members in ((veh, lambda v: (i[rq] == v) | (j[rq] == v)), (step, lambda k: rk == k)):
        for x in range(e.size):
            mine = recs[members(x)]
            assert int(e["n_violating"][x]) == mine.size
            if mine.size:
                best = mine[np.lexsort((mine["row"], mine["min_dist"]))[0]]
                assert (bits(e["min_dist"][x]), int(e["row"][x]), bits(e["t_min"][x])) == (
                    bits(best["min_dist"]), int(best["row"]), bits(best["t_min"]))
                checked += 1
    print(f"ties {N}x{K}x{D}: {recs.size} records, {checked} entries equal to their smallest record bit for bit")
    assert checked > 0


# ---- 4. degenerate segments in interior tiles -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,D", [(300, 4, 2), (200, 3, 3)])
def test_degenerate_segments_in_interior_tiles(ctx, N, K, D):
    """the construction of test_separation_gpu.test_degenerate_segments_in_interior_workgroups.  The pair touching exactly at
    the threshold is undecided by construction: its K segments are the only ones within TOL of the threshold (asserted), and
    only the entries they belong to -- its two vehicles, by up to K, and the steps, by one -- may differ in n_violating."""
    R = 0.8
    pos = np.zeros((N, K, D))
    vel = np.zeros((N, K, D))
    acc = np.zeros((N, K, D))
    side = int(np.ceil(np.sqrt(N)))
    pos[:, :, 0] = 10.0 * (np.arange(N) % side)[:, None]
    pos[:, :, 1] = 10.0 * (np.arange(N) // side)[:, None]
    e0 = np.zeros(D); e0[0] = 1.0
    e1 = np.zeros(D); e1[1] = 1.0
    a = N // 2 + 3  # vehicles in the middle of the triangle: interior tiles, not the first workgroup
    pos[a + 1] = pos[a]                                             # coincident throughout: d = w = b = 0
    pos[a + 3] = pos[a + 2] + 1.0 * e0; vel[a + 3] = -1.5 * e0      # b = 0: f' linear
    pos[a + 5] = pos[a + 4] + 0.9 * e0 + 0.25 * e1                  # b = w = 0: f constant
    pos[a + 7] = pos[a + 6] + 1.0 * e0; acc[a + 7] = 8.0 * e0       # b parallel to d, w = 0: root of f' exactly at t = 0
    pos[a + 9] = pos[a + 8] + 1.0 * e0; vel[a + 9] = -1.0 * e0; acc[a + 9] = (1.0 / H) * e0  # w + h b = 0: root exactly at t = h
    pos[a + 11] = pos[a + 10] + (R - 0.01) * e0                     # touching exactly at the threshold, at rest
    pos[a + 13] = pos[a + 12] + 0.85 * e0; vel[a + 13] = -0.5 * e0; acc[a + 13] = 2.5 * e0  # b parallel to w: dips to 0.8 and back
    host = (pos, vel, acc)
    veh, step = run(ctx, device(ctx, host), R)
    i, j = sr.pair_indices(N)
    pairs = i.size
    q = int(np.nonzero((i == a) & (j == a + 1))[0][0])
    for v in (a, a + 1):
        g = veh[v]
        assert g["min_dist"] == 0.0 and g["t_min"] == 0.0 and int(g["row"]) == q and g["n_violating"] >= K
    assert step["min_dist"][0] == 0.0 and int(step["row"][0]) == q  # ties of exact zeros go to the smallest row
    ref = clr.profile(pos, vel, acc, H, R)
    tol = 32 * sr.EPS * ref["s_max"] ** 2
    undecided = ref["rows"][np.abs(ref["f"] - ref["thr"] ** 2) <= tol]
    q_touch = int(np.nonzero((i == a + 10) & (j == a + 11))[0][0])
    assert sorted(undecided.tolist()) == [k * pairs + q_touch for k in range(K)]
    compare(veh, ref["vehicle"], ref, host, f"vehicle degenerate {N}x{K}x{D}", undecided)
    compare(step, ref["step"], ref, host, f"step degenerate {N}x{K}x{D}", undecided)


# ---- 5. shards ------------------------------------------------------------------------------------------------------------------
def merge_entries(parts):
    out = parts[0].copy()
    for p in parts[1:]:
        better = (p["min_dist"] < out["min_dist"]) | ((p["min_dist"] == out["min_dist"]) & (p["row"] < out["row"]))
        for f in ("min_dist", "row", "t_min"):
            out[f] = np.where(better, p[f], out[f])
        out["sample_min_dist"] = np.minimum(out["sample_min_dist"], p["sample_min_dist"])
        out["n_violating"] = out["n_violating"] + p["n_violating"]
    return out


def raw_call(ctx, dev, R, q0, q1, want_vehicle=True, want_step=True):
    import torch

    from path_planning import _hip

    pos, vel, acc = dev
    N, K, D = pos.shape
    size = _hip.CLEARANCE_DTYPE.itemsize
    veh = torch.zeros(N * size, dtype=torch.uint8, device=ctx.tdev)
    step = torch.zeros(K * size, dtype=torch.uint8, device=ctx.tdev)
    rc = ctx.lib.scp_clearance_profile(ctx.h, N, K, D, H, R, q0, q1, pos.data_ptr(), vel.data_ptr(), acc.data_ptr(),
                                       veh.data_ptr() if want_vehicle else None, step.data_ptr() if want_step else None)
    return rc, veh.cpu().numpy().view(_hip.CLEARANCE_DTYPE), step.cpu().numpy().view(_hip.CLEARANCE_DTYPE)


def test_shards_merge_to_the_full_profile(ctx):
    N, K, D, seed, R = 130, 9, 3, 21, 0.8
    dev, host, _ = random_case(ctx, N, K, D, seed)
    pairs = N * (N - 1) // 2
    veh, step = run(ctx, dev, R)
    cuts = sorted({0, 1, 63, 64, 2017, pairs // 3 + 1, pairs // 2 - 7, pairs - N - 5, pairs - 1, pairs})
    cuts = [c for c in cuts if c <= pairs]
    parts = [run(ctx, dev, R, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    assert merge_entries([p[0] for p in parts]).tobytes() == veh.tobytes()
    assert merge_entries([p[1] for p in parts]).tobytes() == step.tobytes()
    i, j = sr.pair_indices(N)
    for (a, b), (pv, ps) in zip(zip(cuts[:-1], cuts[1:]), parts):
        present = np.zeros(N, dtype=bool)
        present[i[a:b]] = present[j[a:b]] = True
        assert is_empty(pv[~present]).all() and not is_empty(pv[present]).any()  # a vehicle without a pair in the shard
        assert not is_empty(ps).any()
    assert cuts[:2] == [0, 1] and is_empty(parts[0][0][2:]).all()  # the shard [0, 1): the pair (0, 1) only
    ev, es = run(ctx, dev, R, 5, 5)
    assert is_empty(ev).all() and is_empty(es).all() and ev.size == N and es.size == K
    rc, v_only, untouched = raw_call(ctx, dev, R, 0, pairs, want_step=False)
    assert rc == 0 and v_only.tobytes() == veh.tobytes() and not untouched.view(np.uint8).any()
    rc, untouched, s_only = raw_call(ctx, dev, R, 0, pairs, want_vehicle=False)
    assert rc == 0 and s_only.tobytes() == step.tobytes() and not untouched.view(np.uint8).any()


def test_solved_counts_outlive_the_other_passes():
    """the two cost figures belong to the context, not to a workspace: each getter reports its own call's latest run whatever
    ran in between -- the other passes, a list call, a profile that grows the shared workspace -- and SCP_ERR_STATE only on a
    context on which that call never ran"""
    from path_planning import _hip

    c = _hip.Context(0)
    try:
        for getter in (c.last_separation_solved, c.last_clearance_solved):
            with pytest.raises(_hip.HipError) as err:
                getter()
            assert err.value.code == -4  # SCP_ERR_STATE
        (pos, vel, acc), _, _ = random_case(c, 65, 7, 2, 17)
        R = 0.8
        c.check_separation(65, 7, 2, H, R, pos, vel, acc)
        n_check = c.last_separation_solved()
        with pytest.raises(_hip.HipError) as err:
            c.last_clearance_solved()
        assert err.value.code == -4
        c.clearance_profile(65, 7, 2, H, R, pos, vel, acc)
        n_profile = c.last_clearance_solved()
        print(f"solved: check {n_check}, profile {n_profile} of {7 * 65 * 64 // 2} segments")
        assert 0 < n_check <= 7 * 65 * 64 // 2 and 0 < n_profile <= 7 * 65 * 64 // 2
        c.check_separation(65, 7, 2, H, R, pos, vel, acc)
        c.list_conflicts(65, 7, 2, H, R, pos, vel, acc, capacity=0)
        c.clearance_profile(65, 7, 2, H, R, pos, vel, acc)
        assert (c.last_separation_solved(), c.last_clearance_solved()) == (n_check, n_profile)
        big, _, _ = random_case(c, 130, 9, 3, 21)
        c.clearance_profile(130, 9, 3, H, R, *big)  # grows the shared workspace
        assert c.last_separation_solved() == n_check and 0 < c.last_clearance_solved() <= 9 * 130 * 129 // 2
    finally:
        c.close()


# ---- 6. argument errors -----------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    import torch

    lib, hnd = ctx.lib, ctx.h
    N, K, D, R = 5, 4, 2, 0.8
    dev, _, _ = random_case(ctx, N, K, D, 1)
    pp, vp, ap = (x.data_ptr() for x in dev)
    out = torch.zeros((N + K) * 48, dtype=torch.uint8, device=ctx.tdev)
    ov, os_ = out.data_ptr(), out.data_ptr() + N * 48
    pairs = N * (N - 1) // 2
    call = lambda *x: lib.scp_clearance_profile(*x)  # noqa: E731
    assert call(hnd, N, K, D, H, R, 0, pairs, pp, vp, ap, ov, os_) == 0
    assert call(hnd, N, K, D, H, R, 0, pairs, pp, vp, ap, None, None) == -1
    assert "clearance_profile" in lib.scp_last_error(hnd).decode()
    assert call(hnd, N, K, 4, H, R, 0, pairs, pp, vp, ap, ov, os_) == -1
    assert call(hnd, N, K, D, H, R, 0, pairs + 1, pp, vp, ap, ov, os_) == -1
    assert "bad pair range" in lib.scp_last_error(hnd).decode()
    for ptrs in ((None, vp, ap), (pp, None, ap), (pp, vp, None)):
        assert call(hnd, N, K, D, H, R, 0, pairs, *ptrs, ov, os_) == -1
    for h in (0.0, float("inf"), float("nan")):
        assert call(hnd, N, K, D, h, R, 0, pairs, pp, vp, ap, ov, os_) == -1
    assert call(None, N, K, D, H, R, 0, pairs, pp, vp, ap, ov, os_) == -1
    assert call(hnd, N, K, D, H, R, 0, pairs, pp, vp, ap, ov, os_) == 0  # the context is still usable
    assert call(hnd, 1, K, D, H, R, 0, 0, pp, vp, ap, ov, os_) == 0     # N = 1: no pair, every entry empty
    from path_planning import _hip
    assert is_empty(out.cpu().numpy().view(_hip.CLEARANCE_DTYPE)[:1]).all()
    ctx.lib.scp_ctx_synchronize(hnd)
    assert ctx.last_pair_ms() >= 0.0


# ---- 7. the Python surface ----------------------------------------------------------------------------------------------------------
def test_validate_solution_clearance():
    from path_planning.solvers.scp import SCP

    p0, pf = np.array([[2.0, 10.0], [18.0, 10.0]]), np.array([[18.0, 10.0], [2.0, 10.0]])
    s = SCP(n_vehicles=2, time_horizon=10.0, time_step=0.5, min_distance=0.8, space_dims=[0, 0, 20, 20], device=0, verbose=False)
    s.set_initial_states(p0)
    s.set_final_states(pf)
    s.generate_trajectories(max_iterations=15)
    plain = s.validate_solution(continuous=True)
    rep = s.validate_solution(continuous=True, clearance=True)
    assert list(rep) == list(plain) + ["vehicle_clearance", "step_clearance", "most_exposed_vehicle"]
    assert {k: rep[k] for k in plain} == plain
    vc, sc = rep["vehicle_clearance"], rep["step_clearance"]
    assert list(vc) == ["min_distance", "time", "timestep", "partner", "sample_min_distance", "n_violating_segments"]
    assert list(sc) == ["min_distance", "time", "vehicles", "sample_min_distance", "n_violating_segments"]
    assert all(len(vc[k]) == s.N for k in vc) and all(len(sc[k]) == s.K for k in sc) and sc["vehicles"].shape == (s.K, 2)
    assert vc["partner"].tolist() == [1, 0]
    me = rep["most_exposed_vehicle"]
    print(me, sc["min_distance"])
    assert me["vehicle"] in (0, 1) and me["partner"] == 1 - me["vehicle"]
    assert me["distance"] == vc["min_distance"].min() == rep["min_pair_distance_continuous"]
    assert me["time"] == rep["closest_approach"]["time"]
    assert sc["min_distance"].min() == rep["min_pair_distance_continuous"]
    assert sc["sample_min_distance"].min() == rep["min_pair_distance"]
    assert int(sc["n_violating_segments"].sum()) == rep["n_violating_segments"]
    with pytest.raises(ValueError):
        s.validate_solution(clearance=True)
    with pytest.raises(ValueError):
        s.validate_solution(continuous=False, clearance=True)

    from path_planning.viz.plot_trajectories import plot_clearance
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "clearance.pdf")
        plot_clearance(s, path)
        assert os.path.getsize(path) > 0


def test_batch_cli_clearance(tmp_path):
    import json

    from path_planning.cli import compute_trajectories_batch as ctb

    def records(extra):
        out = tmp_path / ("with" if extra else "without")
        ctb.main(["--Ns", "4", "--trials", "2", "--seed", "5", "--results-dir", str(out)] + extra)
        return json.load(open(next(out.glob("*.json"))))["runs"]

    without, with_ = records([]), records(["--clearance"])
    for a, b in zip(without, with_):
        assert a["status"] == b["status"] == "success"
        extra = ["clearance_per_vehicle", "clearance_per_step", "n_vehicles_in_conflict"]
        assert [k for k in b if k not in extra] == list(a) and [k for k in b if k in extra] == extra
        assert not any(k in a for k in extra)
        assert len(b["clearance_per_vehicle"]) == b["N"] and len(b["clearance_per_step"]) == b["K"]
        assert all(isinstance(x, float) for x in b["clearance_per_vehicle"] + b["clearance_per_step"])
        assert isinstance(b["n_vehicles_in_conflict"], int) and 0 <= b["n_vehicles_in_conflict"] <= b["N"]


def test_compute_trajectories_cli_clearance(capsys, tmp_path):
    from path_planning.cli import compute_trajectories as ct

    args = ["--n-agents", "4", "--time-horizon", "10", "--time-step", "0.5", "--space", "0", "0", "20", "20", "--seed", "1"]
    assert ct.main(args + ["--no-plots"]) is not None
    assert "Clearance:" not in capsys.readouterr().out
    solver = ct.main(args + ["--no-plots", "--clearance"])
    out = capsys.readouterr().out
    rep = solver.validate_solution(continuous=True, clearance=True)
    me = rep["most_exposed_vehicle"]
    line = [x for x in out.split("\n") if x.startswith("Clearance: ")]
    assert len(line) == 1 and "Continuous-time check: minimum distance" in out  # implies --continuous-check
    assert f"most exposed vehicle {me['vehicle']} " in line[0] and f"{me['distance']:.4f} m" in line[0]
    assert f"{int((rep['vehicle_clearance']['n_violating_segments'] > 0).sum())} of 4 vehicles in conflict" in line[0]
    prefix = str(tmp_path / "demo")
    assert ct.main(args + ["--clearance", "--save-prefix", prefix]) is not None
    assert os.path.getsize(prefix + "_clearance.pdf") > 0
