"""GPU tests of the continuous-time separation check (scp_check_separation) through the C-ABI, against the numpy
reference of tests/separation_ref.py, and of its Python surface (validate_solution(continuous=True), the batch CLI).

Comparison rules (the kernel's per-segment squared distance f is not observable, only the reductions are):
  TOL = 32 eps S_max^2 on f, S_max the largest |d| + h |w| + h^2/2 |b| over the tested segments -- the evaluation of f is a
  dozen rounded operations on terms bounded by S^2 (1.3 eps S^2 between float64 and long double in the reference,
  test_separation_cpu.py); the factor covers FMA contraction, another evaluation order and the residue of the root search,
  which is second order in f because f' = 0 there;
  min_dist^2 vs the reference's minimum of f: within TOL; sample_min_dist: bitwise scp_check_avoidance's min_dist;
  argmin_row: the reference's unless its two smallest minima lie within TOL of each other; argmin_t: within 1e-6 h, or f at
  both times within TOL (flat f); n_violating / first_violation: the reference's once segments whose reference f lies within
  TOL of (R - 0.01)^2 are left undecided -- at most 0.1 % of a case's segments may be."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import separation_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

NO_ROW = 2**64 - 1


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def device_trajectories(ctx, p0, v0, acc, h):
    """random accelerations pushed through scp_kinematics: device tensors and their host copies"""
    N, K, D = acc.shape
    a = ctx.tensor(acc)
    pos, vel = ctx.kinematics(N, K, D, h, a, ctx.tensor(p0), ctx.tensor(v0))
    return (pos, vel, a), (pos.cpu().numpy(), vel.cpu().numpy(), acc)


def run(ctx, dev, h, R, q0=0, q1=None):
    pos, vel, acc = dev
    N, K, D = pos.shape
    return ctx.check_separation(N, K, D, h, R, pos, vel, acc, q0, q1)


def f_at(host, h, row, t):
    pos, vel, acc = host
    N, K, D = pos.shape
    i, j = sr.pair_indices(N)
    k, q = divmod(int(row), i.size)
    d, w, b = (x[i[q], k] - x[j[q], k] for x in (pos, vel, acc))
    return float(((d + t * w + 0.5 * t * t * b) ** 2).sum())


def compare(st, host, h, R, q0=0, q1=None, label=""):
    """the rules of the module docstring; prints every figure before it asserts"""
    pos, vel, acc = host
    ref = sr.global_stats(pos, vel, acc, h, R, q0, q1)
    tol = 32 * sr.EPS * ref["s_max"] ** 2
    for v in (st["min_dist"], st["sample_min_dist"], st["argmin_t"]):
        assert np.isfinite(v), st
    err = abs(st["min_dist"] ** 2 - max(ref["min_f"], 0.0))
    undecided = np.abs(ref["f"] - ref["thr"] ** 2) <= tol if ref["thr"] > 0 else np.zeros(ref["f"].size, bool)
    print(f"{label}: |min_dist^2 - ref| = {err:.3e} = {err / (sr.EPS * ref['s_max'] ** 2):.2f} eps S_max^2 (bound 32), "
          f"min_dist {st['min_dist']:.6f} sampled {st['sample_min_dist']:.6f}, violating {st['n_violating']} (ref "
          f"{ref['n_violating']}), undecided {int(undecided.sum())} of {ref['n_segments']} segments")
    assert err <= tol
    assert 0.0 <= st["argmin_t"] <= h
    if ref["second_f"] - ref["min_f"] > tol:
        assert st["argmin_row"] == ref["argmin_row"]
        if abs(st["argmin_t"] - ref["argmin_t"]) > 1e-6 * h:  # a flat f: the values decide
            assert abs(f_at(host, h, ref["argmin_row"], st["argmin_t"]) - ref["min_f"]) <= tol
    else:
        assert abs(f_at(host, h, st["argmin_row"], st["argmin_t"]) - ref["min_f"]) <= tol
    assert undecided.sum() <= 1e-3 * ref["n_segments"]
    sure = ref["violating"] & ~undecided
    n_lo, n_hi = int(sure.sum()), int(sure.sum() + undecided.sum())
    assert n_lo <= st["n_violating"] <= n_hi
    if not undecided.any():
        assert st["first_violation"] == ref["first_violation"]
    elif sure.any():
        assert st["first_violation"] <= int(ref["rows"][sure].min())
    assert st["min_dist"] <= st["sample_min_dist"]
    return ref


def sampled(ctx, dev, R, q0=0, q1=None):
    pos = dev[0]
    N, K, D = pos.shape
    return ctx.check_avoidance(N, K, D, R, pos, q0, q1)


# ---- 1. the tunnelling pair: what the sampled check cannot see ------------------------------------------------------------
@pytest.mark.parametrize("N,D,pair", [(2, 2, (0, 1)), (2, 3, (0, 1)), (6, 2, (2, 4)), (7, 3, (3, 6))])
def test_tunnelling_pair(ctx, N, D, pair):
    h, R, K = 0.2, 0.3, 8
    pos = np.zeros((N, K, D))
    vel = np.zeros((N, K, D))
    acc = np.zeros((N, K, D))
    pos[:, :, 0] = 100.0 * (1 + np.arange(N))[:, None]  # everybody far apart, at rest ...
    pos[:, :, D - 1] += 3.0 * np.arange(N)[:, None]
    i, j = pair                                          # ... except one pair: relative speed 4 m/s along a line
    rel = 0.4 + 0.8 * (3 - np.arange(K))                 # ..., +1.2, +0.4, -0.4, -1.2, ...: samples never closer than 0.4
    pos[j] = pos[i]
    pos[i, :, 0] += 0.5 * rel
    pos[j, :, 0] -= 0.5 * rel
    vel[i, :, 0], vel[j, :, 0] = -2.0, 2.0
    dev = tuple(ctx.tensor(x) for x in (pos, vel, acc))
    smin, sfirst, _, _ = sampled(ctx, dev, R)
    assert sfirst == NO_ROW and abs(smin - 0.4) < 1e-12  # the sampled check: collision free, minimum 0.4
    st = run(ctx, dev, h, R)
    pairs = N * (N - 1) // 2
    q = [(a, b) for a in range(N) for b in range(a + 1, N)].index(pair)
    row = 3 * pairs + q  # the segment from +0.4 to -0.4
    ref = compare(st, (pos, vel, acc), h, R, label=f"tunnel N={N} D={D}")
    assert ref["argmin_row"] == row
    assert st["argmin_row"] == row and abs(st["argmin_t"] - 0.1) <= 1e-6 * h
    assert st["first_violation"] == row and st["n_violating"] == 1
    assert st["min_dist"] ** 2 <= 32 * sr.EPS * ref["s_max"] ** 2
    assert st["sample_min_dist"] == smin


# ---- 2. parity with the reference on random kinematically consistent trajectories --------------------------------------------
RANDOM = [(2, 9, 2, 11), (7, 13, 3, 12), (30, 1, 2, 13), (65, 50, 3, 16), (129, 7, 2, 17), (1024, 50, 2, 18), (1300, 12, 2, 19),
          (1100, 3, 3, 20)]


@pytest.mark.parametrize("N,K,D,seed", RANDOM)
def test_random_trajectories_vs_reference(ctx, N, K, D, seed):
    h, R = 0.2, 0.8
    p0, v0, acc = sr.random_case(N, K, D, seed)
    dev, host = device_trajectories(ctx, p0, v0, acc, h)
    st = run(ctx, dev, h, R)
    smin = sampled(ctx, dev, R)[0]
    assert st["sample_min_dist"] == smin  # bitwise
    compare(st, host, h, R, label=f"random {N}x{K}x{D}")
    solved = ctx.last_separation_solved()
    print(f"random {N}x{K}x{D}: {solved} of {K * N * (N - 1) // 2} segments reached the quartic")
    assert run(ctx, dev, h, R) == st  # a second run: bitwise equal


# ---- 3. degenerate segments in interior workgroups ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,D", [(300, 4, 2), (1100, 3, 2), (200, 3, 3)])
def test_degenerate_segments_in_interior_workgroups(ctx, N, K, D):
    h, R = 0.2, 0.8
    pos = np.zeros((N, K, D))
    vel = np.zeros((N, K, D))
    acc = np.zeros((N, K, D))
    side = int(np.ceil(np.sqrt(N)))
    pos[:, :, 0] = 10.0 * (np.arange(N) % side)[:, None]
    pos[:, :, 1] = 10.0 * (np.arange(N) // side)[:, None]
    e0 = np.zeros(D); e0[0] = 1.0
    e1 = np.zeros(D); e1[1] = 1.0
    base = N // 2 + 3  # vehicles in the middle of the triangle: interior tiles, not the first workgroup
    a = base
    pos[a + 1] = pos[a]                                             # coincident throughout: d = w = b = 0
    pos[a + 3] = pos[a + 2] + 1.0 * e0; vel[a + 3] = -1.5 * e0      # b = 0: f' linear
    pos[a + 5] = pos[a + 4] + 0.9 * e0 + 0.25 * e1                  # b = w = 0: f constant
    pos[a + 7] = pos[a + 6] + 1.0 * e0; acc[a + 7] = 8.0 * e0       # b parallel to d, w = 0: root of f' exactly at t = 0
    pos[a + 9] = pos[a + 8] + 1.0 * e0; vel[a + 9] = -1.0 * e0; acc[a + 9] = (1.0 / h) * e0  # w + h b = 0: root exactly at t = h
    pos[a + 11] = pos[a + 10] + (R - 0.01) * e0                     # touching exactly at the threshold, at rest
    pos[a + 13] = pos[a + 12] + 0.85 * e0; vel[a + 13] = -0.5 * e0; acc[a + 13] = 2.5 * e0  # b parallel to w: dips to 0.8 and back
    dev = tuple(ctx.tensor(x) for x in (pos, vel, acc))
    st = run(ctx, dev, h, R)
    assert st["min_dist"] == 0.0 and st["argmin_t"] == 0.0
    i, j = sr.pair_indices(N)
    q = int(np.nonzero((i == a) & (j == a + 1))[0][0])
    assert st["argmin_row"] == q  # k = 0: ties of exact zeros go to the smallest row
    assert st["sample_min_dist"] == sampled(ctx, dev, R)[0] == 0.0
    ref = compare(st, (pos, vel, acc), h, R, label=f"degenerate {N}x{K}x{D}")
    # the coincident pair violates in all K segments; the touching pair (exactly R - 0.01) is undecided by construction
    assert ref["n_violating"] >= K


# ---- 4. pair-range shards with odd cuts tile the full pass bit for bit --------------------------------------------------------
@pytest.mark.parametrize("N,K,D,seed", [(1024, 50, 2, 18), (1300, 12, 2, 19), (130, 9, 3, 21)])
def test_pair_range_shards_tile_the_full_pass(ctx, N, K, D, seed):
    h, R = 0.2, 0.8
    p0, v0, acc = sr.random_case(N, K, D, seed)
    dev, host = device_trajectories(ctx, p0, v0, acc, h)
    pairs = N * (N - 1) // 2
    full = run(ctx, dev, h, R)
    assert run(ctx, dev, h, R) == full
    cuts = sorted({0, 1, 63, 64, 2017, pairs // 3 + 1, pairs // 2 - 7, pairs - N - 5, pairs - 1, pairs})
    parts = [run(ctx, dev, h, R, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    best = min((p["min_dist"], p["argmin_row"]) for p in parts)
    assert best == (full["min_dist"], full["argmin_row"])
    winner = [p for p in parts if (p["min_dist"], p["argmin_row"]) == best][0]
    assert winner["argmin_t"] == full["argmin_t"]
    assert min(p["first_violation"] for p in parts) == full["first_violation"]
    assert sum(p["n_violating"] for p in parts) == full["n_violating"]
    assert min(p["sample_min_dist"] for p in parts) == full["sample_min_dist"]
    for (a, b), p in zip(zip(cuts[:-1], cuts[1:]), parts):
        assert p["sample_min_dist"] == sampled(ctx, dev, R, a, b)[0]
    # one shard against the reference restricted to its rows
    a, b = cuts[5], cuts[6]
    compare(parts[5], host, h, R, a, b, label=f"shard [{a}, {b}) of {N}x{K}")
    empty = run(ctx, dev, h, R, 5, 5)
    assert empty["min_dist"] == np.inf and empty["argmin_row"] == NO_ROW and empty["n_violating"] == 0
    assert empty["first_violation"] == NO_ROW


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------
BASE_KEYS = ["min_pair_distance", "collision_free", "first_violation", "acc_violation", "jerk_violation", "vel_violation",
             "pos_violation", "final_position_error", "final_velocity_error"]
EXTRA_KEYS = ["min_pair_distance_continuous", "collision_free_continuous", "n_violating_segments",
              "first_violation_continuous", "closest_approach"]


def solved(case):
    from path_planning.scenarios.position_generator import generate_positions
    from path_planning.solvers.scp import SCP

    if case[0] == "swap":
        h = case[1]
        p0, pf = np.array([[2.0, 10.0], [18.0, 10.0]]), np.array([[18.0, 10.0], [2.0, 10.0]])
        n = 2
    else:
        h = 0.2
        p0, pf = generate_positions(10, 0.8, seed=7)
        n = 10
    s = SCP(n_vehicles=n, time_horizon=10.0, time_step=h, min_distance=0.8, space_dims=[0, 0, 20, 20], device=0, verbose=False)
    s.set_initial_states(np.asarray(p0))
    s.set_final_states(np.asarray(pf))
    s.generate_trajectories(max_iterations=15)
    return s


@pytest.mark.parametrize("case", [("swap", 0.5), ("swap", 0.2), ("generator", 0.2)], ids=["swap_h0.5", "swap_h0.2", "gen10_s7"])
def test_validate_solution_continuous(ctx, case):
    s = solved(case)
    plain = s.validate_solution()
    assert list(plain) == BASE_KEYS
    rep = s.validate_solution(continuous=True)
    assert list(rep) == BASE_KEYS + EXTRA_KEYS
    assert {k: rep[k] for k in BASE_KEYS} == plain
    tr = s.trajectories
    host = tuple(np.ascontiguousarray(tr[k], dtype=np.float64) for k in ("positions", "velocities", "accelerations"))
    st = {"min_dist": rep["min_pair_distance_continuous"], "sample_min_dist": rep["min_pair_distance"],
          "n_violating": rep["n_violating_segments"]}
    ca = rep["closest_approach"]
    pairs = s.N * (s.N - 1) // 2
    i, j = sr.pair_indices(s.N)
    q = int(np.nonzero((i == ca["vehicles"][0]) & (j == ca["vehicles"][1]))[0][0])
    st["argmin_row"] = ca["timestep"] * pairs + q
    st["argmin_t"] = ca["time"] - ca["timestep"] * s.h
    st["argmin_t"] = min(max(st["argmin_t"], 0.0), s.h)  # (k h + t) - k h: the last bits
    fv = rep["first_violation_continuous"]
    st["first_violation"] = NO_ROW if fv is None else fv["timestep"] * pairs + int(
        np.nonzero((i == fv["vehicles"][0]) & (j == fv["vehicles"][1]))[0][0])
    ref = compare(st, host, s.h, s.R, label=f"solve {case}")
    print(f"solve {case}: sampled {rep['min_pair_distance']:.4f} continuous {rep['min_pair_distance_continuous']:.4f} "
          f"violating segments {rep['n_violating_segments']} closest {ca}")
    assert rep["min_pair_distance_continuous"] <= rep["min_pair_distance"]
    assert rep["collision_free_continuous"] == (rep["n_violating_segments"] == 0)
    assert ca["distance"] == rep["min_pair_distance_continuous"]
    if fv is not None:
        assert abs(fv["distance"] ** 2 - max(ref["f"][ref["rows"] == st["first_violation"]][0], 0.0)) <= 64 * sr.EPS * ref["s_max"] ** 2
        assert fv["distance"] < s.R - 0.01 + 1e-9


def test_batch_cli_continuous_check(tmp_path):
    import json

    from path_planning.cli import compute_trajectories_batch as ctb

    def records(extra):
        out = tmp_path / ("with" if extra else "without")
        ctb.main(["--Ns", "4", "--trials", "2", "--seed", "5", "--results-dir", str(out)] + extra)
        return json.load(open(next(out.glob("*.json"))))["runs"]

    without, with_ = records([]), records(["--continuous-check"])
    for a, b in zip(without, with_):
        assert a["status"] == b["status"] == "success"
        extra = ["min_pair_distance_continuous", "n_violating_segments"]
        assert [k for k in b if k not in extra] == list(a) and [k for k in b if k in extra] == extra
        assert "min_pair_distance_continuous" not in a and "n_violating_segments" not in a
        assert np.isfinite(b["min_pair_distance_continuous"]) and b["n_violating_segments"] >= 0


def test_compute_trajectories_cli_prints_the_line(capsys):
    from path_planning.cli import compute_trajectories as ct

    args = ["--n-agents", "4", "--time-horizon", "10", "--time-step", "0.5", "--space", "0", "0", "20", "20", "--seed", "1",
            "--no-plots"]
    assert ct.main(args) is not None
    assert "Continuous-time check" not in capsys.readouterr().out
    assert ct.main(args + ["--continuous-check"]) is not None
    out = capsys.readouterr().out
    assert "Continuous-time check: minimum distance" in out and "between vehicles" in out and "at t =" in out


# ---- 6. argument errors: the codes of scp_check_avoidance ---------------------------------------------------------------------
def test_argument_errors(ctx):
    lib, hnd = ctx.lib, ctx.h
    N, K, D, h, R = 5, 4, 2, 0.2, 0.8
    p0, v0, acc = sr.random_case(N, K, D, 1)
    (pos, vel, a), _ = device_trajectories(ctx, p0, v0, acc, h)
    st = ctx.empty(6)
    pp, vp, ap, sp = pos.data_ptr(), vel.data_ptr(), a.data_ptr(), st.data_ptr()
    pairs = N * (N - 1) // 2
    sep = lambda *x: lib.scp_check_separation(*x)  # noqa: E731
    chk = lambda *x: lib.scp_check_avoidance(*x)  # noqa: E731
    assert sep(hnd, N, K, D, h, R, 0, pairs, pp, vp, ap, sp) == 0
    for bad in ((N, K, 4, 0, pairs), (N, K, 1, 0, pairs), (N, K, D, -1, pairs), (N, K, D, 3, 2), (N, K, D, 0, pairs + 1),
                (0, K, D, 0, 0), (N, 0, D, 0, pairs)):
        n, k, d, q0, q1 = bad
        assert sep(hnd, n, k, d, h, R, q0, q1, pp, vp, ap, sp) == chk(hnd, n, k, d, R, q0, q1, pp, sp) == -1, bad
    for ptrs in ((None, vp, ap, sp), (pp, None, ap, sp), (pp, vp, None, sp), (pp, vp, ap, None)):
        assert sep(hnd, N, K, D, h, R, 0, pairs, *ptrs) == -1
    assert chk(hnd, N, K, D, R, 0, pairs, None, sp) == chk(hnd, N, K, D, R, 0, pairs, pp, None) == -1
    assert sep(None, N, K, D, h, R, 0, pairs, pp, vp, ap, sp) == chk(None, N, K, D, R, 0, pairs, pp, sp) == -1
    assert sep(hnd, N, K, D, 0.0, R, 0, pairs, pp, vp, ap, sp) == -1
    assert "check_separation" in lib.scp_last_error(hnd).decode()
    assert sep(hnd, N, K, D, h, R, 0, pairs, pp, vp, ap, sp) == 0  # the context is still usable
    ctx.lib.scp_ctx_synchronize(hnd)
    assert ctx.last_pair_ms() >= 0.0
