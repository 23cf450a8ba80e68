"""GPU tests of the conflict list (scp_list_conflicts) through the C-ABI and its Python surface, against the numpy reference of
tests/conflicts_ref.py (pinned on the CPU by tests/test_conflicts_cpu.py).

Comparison rules, in the language of tests/test_separation_gpu.py:
  TOL = 32 eps S_max^2 on f, S_max the largest |d| + h |w| + h^2/2 |b| over the tested segments, taken from the reference;
  a segment whose reference minimum of f lies within TOL of thr^2 = (R - 0.01)^2 is UNDECIDED: it may or may not be listed --
  at most 0.1 % of a case's segments may be;
  per record: min_dist^2 within TOL of the reference's minimum of f; 0 <= t_enter <= t_exit <= h; f(t_min) < thr^2 + TOL;
  an interior end lies on the threshold: |f(t) - thr^2| <= TOL + 2 S (|w| + h |b|) h 2^-48 (the bisection's resolution
  times the bound of |f'|, S of that row); 401 samples of [0, t_enter) and of (t_exit, h] stay >= thr^2 - TOL;
  against scp_check_separation on the same inputs, bit for bit: the length is n_violating, the first row is first_violation,
  the record of argmin_row carries the stats' min_dist and argmin_t; a second call returns the same bytes."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conflicts_ref as cr  # noqa: E402
import separation_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

H = 0.2
RANDOM = [(2, 9, 2, 11), (65, 50, 3, 16), (129, 7, 2, 17), (130, 9, 3, 21)]
_CASES = {}


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def random_case(ctx, N, K, D, seed):
    """device tensors and host copies of a random case (through scp_kinematics, as the separation tests), made once"""
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
        refs[R] = cr.records(*host, H, R)
    return refs[R]


def listing(ctx, dev, R, q0=0, q1=None, capacity=None):
    pos, vel, acc = dev
    N, K, D = pos.shape
    return ctx.list_conflicts(N, K, D, H, R, pos, vel, acc, q0, q1, capacity)


def device(ctx, host):
    return tuple(ctx.tensor(x) for x in host)


def compare(got, host, ref, R, label):
    """the rules of the module docstring; prints every figure before it asserts"""
    st = ref["stats"]
    thr2 = st["thr"] ** 2
    tol = 32 * sr.EPS * st["s_max"] ** 2
    undecided = set(st["rows"][np.abs(st["f"] - thr2) <= tol].tolist())
    rows = got["row"].astype(np.int64)
    by_row = {int(r): e for e, r in enumerate(ref["rows"])}
    err_m = max([abs(g["min_dist"] ** 2 - max(ref["f"][by_row[int(g["row"])]], 0.0)) for g in got if int(g["row"]) in by_row],
                default=0.0)
    print(f"{label}: {got.size} records (reference {ref['rows'].size}, undecided {len(undecided)} of {st['n_segments']} segments), "
          f"two-piece records {int((got['pieces'] == 2).sum())}, max |min_dist^2 - ref| = {err_m / (sr.EPS * st['s_max'] ** 2):.2f} "
          f"eps S_max^2 (bound 32)")
    assert len(undecided) <= 1e-3 * st["n_segments"]
    assert (np.diff(rows) > 0).all()
    assert sorted(set(rows.tolist()) - undecided) == sorted(set(ref["rows"].tolist()) - undecided)
    assert (got["reserved"] == 0).all() and np.isin(got["pieces"], (1, 2)).all()
    n = lambda x: float(np.sqrt((x ** 2).sum()))  # noqa: E731
    worst_end = 0.0
    for g in got:
        row = int(g["row"])
        d, w, b = cr.segment_of_row(host, row)
        c = sr.coefficients(d, w, b)
        if row in by_row:
            assert abs(g["min_dist"] ** 2 - max(ref["f"][by_row[row]], 0.0)) <= tol
        assert 0.0 <= g["t_enter"] <= g["t_exit"] <= H and 0.0 <= g["t_min"] <= H
        assert cr.f_at(c, g["t_min"]) < thr2 + tol
        end_tol = tol + 2 * float(sr.s_bound(d, w, b, H)) * (n(w) + H * n(b)) * H * 2.0 ** -48
        for end, inside in ((g["t_enter"], g["t_enter"] > 0.0), (g["t_exit"], g["t_exit"] < H)):
            if inside:
                worst_end = max(worst_end, abs(cr.f_at(c, end) - thr2) / end_tol)
                assert abs(cr.f_at(c, end) - thr2) <= end_tol
        # 401 samples of [0, t_enter) and of (t_exit, h]; a segment that starts (ends) inside has an empty interval there
        if g["t_enter"] > 0.0:
            before = np.linspace(0.0, g["t_enter"], 401, endpoint=False)
            assert (cr.f_at(c, before) >= thr2 - tol).all()
        if g["t_exit"] < H:
            after = g["t_exit"] + (H - g["t_exit"]) * np.arange(1, 402) / 401.0
            assert (cr.f_at(c, np.minimum(after, H)) >= thr2 - tol).all()
    print(f"{label}: worst interior end at {worst_end:.3f} of its bound")


def against_the_check(ctx, dev, R, got, q0=0, q1=None):
    pos, vel, acc = dev
    N, K, D = pos.shape
    st = ctx.check_separation(N, K, D, H, R, pos, vel, acc, q0, q1)
    assert got.size == st["n_violating"]
    if got.size:
        assert int(got["row"][0]) == st["first_violation"]
    hit = got[got["row"] == st["argmin_row"]]
    if hit.size:
        assert hit["min_dist"].tobytes() == np.float64(st["min_dist"]).tobytes()
        assert hit["t_min"].tobytes() == np.float64(st["argmin_t"]).tobytes()
    return st


# ---- 1. the tunnelling pair ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,pair", [(2, 2, (0, 1)), (7, 3, (3, 6))])
def test_tunnelling_pair(ctx, N, D, pair):
    pos, vel, acc, row = cr.tunnelling_case(N, D, pair)
    got = listing(ctx, device(ctx, (pos, vel, acc)), 0.3)
    print(f"tunnel N={N} D={D}: {got}")
    assert got.size == 1
    g = got[0]
    assert int(g["row"]) == row and g["pieces"] == 1 and g["reserved"] == 0
    assert abs(g["t_min"] - 0.1) <= 1e-6 * H
    # |0.4 - 4 t| = 0.29; the bisection resolves h 2^-48 and |f'| is about 2.3 there
    assert abs(g["t_enter"] - 0.0275) <= 1e-9 and abs(g["t_exit"] - 0.1725) <= 1e-9
    assert g["min_dist"] ** 2 <= 32 * sr.EPS * 1.2 ** 2  # S = 0.4 + h 4
    against_the_check(ctx, device(ctx, (pos, vel, acc)), 0.3, got)


# ---- 2. a run across segments ---------------------------------------------------------------------------------------------------
def test_run_across_segments(ctx):
    """two vehicles approach at 0.2 m/s from 0.32 m and pass through each other: closer than 0.29 m from t = 0.15 s to
    t = 3.05 s, segments 0 .. 15 of 20"""
    from path_planning.solvers.conflicts import conflict_windows

    N, K, D, R = 3, 20, 2, 0.3
    pos = np.zeros((N, K, D))
    vel = np.zeros((N, K, D))
    acc = np.zeros((N, K, D))
    pos[2, :, 1] = 50.0
    pos[1, :, 0] = 0.32 - 0.2 * H * np.arange(K)
    vel[1, :, 0] = -0.2
    got = listing(ctx, device(ctx, (pos, vel, acc)), R)
    print(got)
    assert got["row"].tolist() == [k * 3 + 0 for k in range(16)] and (got["pieces"] == 1).all()
    assert abs(got["t_enter"][0] - 0.15) <= 1e-9 and abs(got["t_exit"][15] - 0.05) <= 1e-9
    assert (got["t_enter"][1:] == 0.0).all() and (got["t_exit"][:15] == H).all()  # exactly: what conflict_windows merges on
    (w,) = conflict_windows(got, N, K, H)
    assert w["vehicles"] == (0, 1) and w["n_segments"] == 16 and w["first_timestep"] == 0 and w["pieces"] == 1
    assert abs(w["t_start"] - 0.15) <= 1e-9 and abs(w["t_end"] - 3.05) <= 1e-9
    assert w["min_distance"] <= 1e-7 and abs(w["t_min_distance"] - 1.6) <= 1e-6


# ---- 3. two pieces in one segment -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
def test_two_pieces_in_one_segment(ctx, D):
    N, K, R = 3, 2, 0.3
    d, w, b = cr.TWO_PIECES
    win = cr.window(sr.coefficients(d, w, b), H, R - 0.01)
    assert win[2] == 2 and len(win[3]) == 4  # four real roots of g in (0, h)
    pos = np.zeros((N, K, D))
    vel = np.zeros((N, K, D))
    acc = np.zeros((N, K, D))
    pos[:, :, 0] = 50.0 * np.arange(N)[:, None]
    pos[2, 1, :2], vel[2, 1, :2], acc[2, 1, :2] = pos[1, 1, :2] - d, -w, -b  # pair (1, 2), segment 1: i - j = (d, w, b)
    got = listing(ctx, device(ctx, (pos, vel, acc)), R)
    print(got, win)
    assert got.size == 1 and int(got["row"][0]) == 1 * 3 + 2 and got["pieces"][0] == 2
    assert abs(got["t_enter"][0] - win[0]) <= 1e-9 and abs(got["t_exit"][0] - win[1]) <= 1e-9
    from path_planning.solvers.conflicts import conflict_windows

    assert conflict_windows(got, N, K, H)[0]["pieces"] == 2


# ---- 4. random trajectories against the reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,D,seed", RANDOM)
def test_random_trajectories_vs_reference(ctx, N, K, D, seed):
    R = 0.8
    case = random_case(ctx, N, K, D, seed)
    dev, host, _ = case
    got = listing(ctx, dev, R)
    compare(got, host, reference(case, R), R, f"random {N}x{K}x{D}")
    against_the_check(ctx, dev, R, got)
    assert listing(ctx, dev, R).tobytes() == got.tobytes()  # a second call: the same bytes


# ---- 5. shards --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,D,seed", [(130, 9, 3, 21), (129, 7, 2, 17)])
def test_shards_merge_to_the_full_list(ctx, N, K, D, seed):
    R = 0.8
    dev, host, _ = random_case(ctx, N, K, D, seed)
    pairs = N * (N - 1) // 2
    full = listing(ctx, dev, R)
    cuts = [0, 70, 70, pairs // 2 - 7, pairs]  # inside the first tile row, an empty shard, an odd cut in the middle
    parts = [listing(ctx, dev, R, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    print(f"shards {N}x{K}x{D}: {[p.size for p in parts]} of {full.size}")
    assert parts[1].size == 0 and full.size > 1
    merged = np.concatenate(parts)
    merged = merged[np.argsort(merged["row"], kind="stable")]
    assert merged.tobytes() == full.tobytes()
    for (a, b), p in zip(zip(cuts[:-1], cuts[1:]), parts):
        against_the_check(ctx, dev, R, p, a, b)


# ---- 6. capacity --------------------------------------------------------------------------------------------------------------------
def raw_call(ctx, dev, R, capacity):
    import torch

    from path_planning import _hip

    pos, vel, acc = dev
    N, K, D = pos.shape
    out = torch.zeros(max(capacity, 1) * 48, dtype=torch.uint8, device=ctx.tdev)
    n = torch.full((1,), -1, dtype=torch.int64, device=ctx.tdev)
    rc = ctx.lib.scp_list_conflicts(ctx.h, N, K, D, H, R, 0, N * (N - 1) // 2, pos.data_ptr(), vel.data_ptr(), acc.data_ptr(),
                                    out.data_ptr(), capacity, n.data_ptr())
    return rc, int(n.item()), out.cpu().numpy().view(_hip.CONFLICT_DTYPE)


def test_capacity_protocol(ctx):
    R = 0.8
    dev, host, _ = random_case(ctx, 130, 9, 3, 21)
    full = listing(ctx, dev, R)
    n = full.size
    assert n > 1
    for cap in (n - 1, 0):
        rc, found, _ = raw_call(ctx, dev, R, cap)
        assert rc == 0 and found == n
    rc, found, out = raw_call(ctx, dev, R, n)
    assert rc == 0 and found == n and out[:n].tobytes() == full.tobytes()
    assert listing(ctx, dev, R, capacity=1).tobytes() == full.tobytes()  # the binding's repetition
    assert listing(ctx, dev, R, capacity=0).tobytes() == full.tobytes()
    none = listing(ctx, dev, 0.05)
    assert none.size == 0 and none.dtype == full.dtype
    assert raw_call(ctx, dev, 0.05, 0)[:2] == (0, 0)


def test_long_list_leaves_the_one_workgroup_sort(ctx):
    """the 129-vehicle case with R raised until the list is longer than the 1024 records one workgroup sorts"""
    case = random_case(ctx, 129, 7, 2, 17)
    dev, host, _ = case
    N, K, D = dev[0].shape
    for R in (1.5, 2.0, 3.0, 4.0):
        if ctx.check_separation(N, K, D, H, R, *dev)["n_violating"] > 2 * 1024:
            break
    got = listing(ctx, dev, R)
    print(f"long list: R = {R}: {got.size} records (one-workgroup sort: up to 1024)")
    assert got.size > 2 * 1024  # the sort runs over 4096 slots: global steps of two stages
    against_the_check(ctx, dev, R, got)
    compare(got, host, reference(case, R), R, f"long list R={R}")
    assert listing(ctx, dev, R, capacity=got.size + 1500).tobytes() == got.tobytes()
    pairs = N * (N - 1) // 2
    parts = [listing(ctx, dev, R, a, b) for a, b in ((0, 100), (100, pairs // 2 + 3), (pairs // 2 + 3, pairs))]
    merged = np.concatenate(parts)
    assert merged[np.argsort(merged["row"], kind="stable")].tobytes() == got.tobytes()


# ---- 7. the surface -------------------------------------------------------------------------------------------------------------------
def test_validate_solution_lists_the_tunnelling_conflict():
    from path_planning.solvers.scp import SCP

    N, D, K = 2, 2, 8
    pos, vel, acc, row = cr.tunnelling_case(N, D, (0, 1), K)
    s = SCP(n_vehicles=N, time_horizon=K * H + 1e-9, time_step=H, min_distance=0.3, space_dims=[-1000, -1000, 1000, 1000],
            device=0, verbose=False)
    assert s.K == K
    s.set_initial_states(pos[:, 0])
    s.set_final_states(pos[:, K - 1])
    s.trajectories = {"positions": pos, "velocities": vel, "accelerations": acc}
    plain = s.validate_solution(continuous=True)
    assert s.validate_solution(continuous=True, conflicts=False) == plain and "conflicts" not in plain
    rep = s.validate_solution(continuous=True, conflicts=True)
    assert list(rep) == list(plain) + ["conflicts", "n_conflicts"] and {k: rep[k] for k in plain} == plain
    assert rep["n_conflicts"] == 1 and rep["n_violating_segments"] == 1
    (w,) = rep["conflicts"]
    print(w)
    assert w["vehicles"] == (0, 1) and w["first_timestep"] == 3 and w["n_segments"] == 1 and w["pieces"] == 1
    assert abs(w["t_start"] - (3 * H + 0.0275)) <= 1e-9 and abs(w["t_end"] - (3 * H + 0.1725)) <= 1e-9
    assert abs(w["duration"] - 0.145) <= 2e-9 and abs(w["t_min_distance"] - (3 * H + 0.1)) <= 1e-6 * H
    assert w["min_distance"] == rep["min_pair_distance_continuous"]
    with pytest.raises(ValueError):
        s.validate_solution(conflicts=True)
    with pytest.raises(ValueError):
        s.validate_solution(continuous=False, conflicts=True)


def test_batch_cli_list_conflicts(tmp_path):
    import json

    from path_planning.cli import compute_trajectories_batch as ctb

    def records(extra):
        out = tmp_path / ("with" if extra else "without")
        ctb.main(["--Ns", "4", "--trials", "2", "--seed", "5", "--results-dir", str(out)] + extra)
        return json.load(open(next(out.glob("*.json"))))["runs"]

    without, with_ = records([]), records(["--list-conflicts"])
    for a, b in zip(without, with_):
        assert a["status"] == b["status"] == "success"
        extra = ["conflicts", "n_conflicts"]
        assert [k for k in b if k not in extra] == list(a) and [k for k in b if k in extra] == extra
        assert "conflicts" not in a and "n_conflicts" not in a
        assert isinstance(b["conflicts"], list) and b["n_conflicts"] == len(b["conflicts"])
        for w in b["conflicts"]:
            assert set(w) == {"vehicles", "t_start", "t_end", "duration", "min_distance", "t_min_distance", "first_timestep",
                              "n_segments", "pieces"}


def test_compute_trajectories_cli_lists_conflicts(capsys):
    from path_planning.cli import compute_trajectories as ct

    args = ["--n-agents", "4", "--time-horizon", "10", "--time-step", "0.5", "--space", "0", "0", "20", "20", "--seed", "1",
            "--no-plots"]
    assert ct.main(args) is not None
    out = capsys.readouterr().out
    assert "Continuous-time check" not in out and "conflict:" not in out
    solver = ct.main(args + ["--list-conflicts"])
    out = capsys.readouterr().out
    assert solver is not None and "Continuous-time check: minimum distance" in out  # implies --continuous-check
    rep = solver.validate_solution(continuous=True, conflicts=True)
    lines = [x for x in out.split("\n") if x.startswith("  conflict: vehicles ")]
    assert len(lines) == rep["n_conflicts"]
    for line, w in zip(lines, rep["conflicts"]):
        assert f"vehicles {w['vehicles'][0]} and {w['vehicles'][1]} from t = {w['t_start']:.4f} s to t = {w['t_end']:.4f} s" in line
        assert f"minimum distance {w['min_distance']:.4f} m" in line


# ---- 8. argument errors -----------------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    import torch

    lib, hnd = ctx.lib, ctx.h
    N, K, D, R = 5, 4, 2, 0.8
    dev, _, _ = random_case(ctx, N, K, D, 1)
    pp, vp, ap = (x.data_ptr() for x in dev)
    out = torch.zeros(16 * 48, dtype=torch.uint8, device=ctx.tdev)
    n = torch.zeros(1, dtype=torch.int64, device=ctx.tdev)
    op, np_ = out.data_ptr(), n.data_ptr()
    pairs = N * (N - 1) // 2
    call = lambda *x: lib.scp_list_conflicts(*x)  # noqa: E731
    assert call(hnd, N, K, D, H, R, 0, pairs, pp, vp, ap, op, 16, np_) == 0
    for ptrs in ((None, vp, ap, op, 16, np_), (pp, None, ap, op, 16, np_), (pp, vp, None, op, 16, np_), (pp, vp, ap, None, 16, np_),
                 (pp, vp, ap, op, 16, None)):
        assert call(hnd, N, K, D, H, R, 0, pairs, *ptrs) == -1
        assert "list_conflicts" in lib.scp_last_error(hnd).decode()
    for h in (0.0, -0.2, float("inf"), float("nan")):
        assert call(hnd, N, K, D, h, R, 0, pairs, pp, vp, ap, op, 16, np_) == -1
    assert "list_conflicts: bad time step" in lib.scp_last_error(hnd).decode()
    for q0, q1 in ((-1, pairs), (3, 2), (0, pairs + 1)):
        assert call(hnd, N, K, D, H, R, q0, q1, pp, vp, ap, op, 16, np_) == -1
    assert "bad pair range" in lib.scp_last_error(hnd).decode()
    for shape in ((N, K, 4), (0, K, D), (N, 0, D)):
        assert call(hnd, *shape, H, R, 0, 0, pp, vp, ap, op, 16, np_) == -1
    assert call(hnd, N, K, D, H, R, 0, pairs, pp, vp, ap, op, -1, np_) == -1
    assert "list_conflicts: bad capacity" in lib.scp_last_error(hnd).decode()
    assert call(None, N, K, D, H, R, 0, pairs, pp, vp, ap, op, 16, np_) == -1
    assert call(hnd, N, K, D, H, R, 0, pairs, pp, vp, ap, None, 0, np_) == 0  # counting only: no list needed
    assert call(hnd, N, K, D, H, R, 2, 2, pp, vp, ap, op, 16, np_) == 0 and int(n.item()) == 0  # an empty pair range
    ctx.lib.scp_ctx_synchronize(hnd)
    assert ctx.last_pair_ms() >= 0.0
    assert ctypes.sizeof(ctypes.c_void_p) == 8
