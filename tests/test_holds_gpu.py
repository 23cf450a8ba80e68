"""GPU tests of the holds: scp_update_holds and scp_apply_holds against the numpy reference of tests/holds_ref.py (pinned on the
CPU by tests/test_holds_cpu.py), and SCP.repair_conflicts end to end.

Comparison rules:
  update: rows and counts exact; eta and margin within 8 eps relative (each is fewer than ten roundings; a kernel that follows
    the stated order gives the same bits);
  apply: the held entries of the eta planes are bitwise the table's, l within 4 eps max(1, |l|); every other entry of the planes
    and every other bitmap word keeps its bits; the bitmap is the old one with the held bits set; the new rows are the held rows
    that were not selected, ascending;
  end to end: the three ring scenarios have a conflict before the repair (asserted), none after at most 6 passes, the sample
    minimum stays >= R - 0.01, and every bound validate_solution reports stays within the termination tolerance of the QP
    solver, eps_abs + eps_rel * 20 (20: the largest bound among the fixed rows, jerk and position; eps = 1e-3)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conflicts_ref as cr  # noqa: E402
import holds_ref as hr  # noqa: E402

pytestmark = pytest.mark.gpu

H = 0.2
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def tunnels(N, D, pairs, K=8):
    """conflicts_ref.tunnelling_case for several disjoint pairs: everybody far apart and at rest, except the pairs, whose
    relative position is 0.4 - 4 t along axis 0 in segment 3 (0.4 m apart at the end of segment 2 and the start of segment 4)"""
    pos = np.zeros((N, K, D))
    vel = np.zeros((N, K, D))
    acc = np.zeros((N, K, D))
    pos[:, :, 0] = 100.0 * (1 + np.arange(N))[:, None]
    pos[:, :, D - 1] += 3.0 * np.arange(N)[:, None]
    rel = 0.4 + 0.8 * (3 - np.arange(K))
    for i, j in pairs:
        pos[j] = pos[i]
        pos[i, :, 0] += 0.5 * rel
        pos[j, :, 0] -= 0.5 * rel
        vel[i, :, 0], vel[j, :, 0] = -2.0, 2.0
    return pos, vel, acc


def two_pieces(D):
    """conflicts_ref.TWO_PIECES in the LAST segment (K = 2, segment 1) of pair (1, 2) of three vehicles"""
    N, K = 3, 2
    d, w, b = cr.TWO_PIECES
    pos = np.zeros((N, K, D))
    vel = np.zeros((N, K, D))
    acc = np.zeros((N, K, D))
    pos[:, :, 0] = 50.0 * np.arange(N)[:, None]
    pos[2, 1, :2], vel[2, 1, :2], acc[2, 1, :2] = pos[1, 1, :2] - d, -w, -b
    return pos, vel, acc


def run_update(ctx, host, R, pad, table=None, q0=0, q1=None, capacity=None, grow=True):
    """conflicts from Context.list_conflicts, then the device update and the reference's -> (got, needed, ref, conflicts)"""
    pos, vel, acc = host
    N, K, D = pos.shape
    dev = tuple(ctx.tensor(x) for x in host)
    found = ctx.list_conflicts(N, K, D, H, R, *dev)
    start = hr.empty_table() if table is None else table
    t_dev, n_dev = ctx.hold_table(start, capacity=capacity)
    t_dev, n_dev, needed = ctx.update_holds(N, K, D, H, R, *dev, found, t_dev, n_dev, pad, q0, q1, grow=grow)
    got = ctx.read_holds(t_dev, n_dev)
    ref = hr.update(start, pos, vel, acc, R, found, pad, q0, q1)
    return got, needed, ref, found


def compare_tables(got, ref, label):
    print(f"{label}: {got.size} holds (reference {ref.size})")
    assert got["row"].tolist() == ref["row"].tolist()
    assert (np.diff(got["row"].astype(np.int64)) > 0).all()
    assert (got["reserved"] == 0).all()
    err_eta = np.abs(got["eta"] - ref["eta"])
    err_m = np.abs(got["margin"] - ref["margin"])
    worst = max(float((err_eta / np.maximum(np.abs(ref["eta"]), 1e-300)).max(initial=0.0)),
                float((err_m / np.maximum(np.abs(ref["margin"]), 1e-300)).max(initial=0.0)))
    print(f"{label}: worst relative difference {worst / EPS:.2f} eps (bound 8), bitwise equal: "
          f"{got.tobytes() == ref.tobytes()}")
    assert (err_eta <= 8 * EPS * np.abs(ref["eta"])).all()
    assert (err_m <= 8 * EPS * np.abs(ref["margin"])).all()
    norms = np.sqrt((got["eta"] ** 2).sum(axis=1))
    assert (np.abs(norms - 1.0) <= 4 * EPS).all()


# ---- 1. the table update against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
def test_update_perpendicular_fallback(ctx, D):
    """R = 0.3: the crossing in segment 3 alone is a conflict, d(t_min) = 0 -> the perpendicular of the relative velocity"""
    pos, vel, acc, row = cr.tunnelling_case(5, D, (1, 3))
    got, needed, ref, found = run_update(ctx, (pos, vel, acc), 0.3, 0.02)
    assert found["row"].tolist() == [row] and found["min_dist"][0] < 1e-6
    compare_tables(got, ref, f"tunnelling D={D}")
    assert needed == 2 and got["row"].tolist() == [row, row + 10]
    # w = (-4, 0[, 0]).  2-D: (-w1, w0) / |w| = (0, -1); 3-D: m = 1 (the lowest of the two zero coordinates), w x e_1 = (-w2, 0, w0)
    expect = [0.0, -1.0, 0.0] if D == 2 else [0.0, 0.0, -1.0]
    assert np.array_equal(got["eta"][0], expect) and np.array_equal(got["eta"][1], expect)
    assert np.abs(got["margin"] - (0.3 - found["min_dist"][0] + 0.02)).max() <= 8 * EPS


@pytest.mark.parametrize("D", [2, 3])
def test_update_two_candidates_on_one_row(ctx, D):
    """R = 0.5: the pair is in conflict in the segments 2, 3 and 4, so two candidates meet on the rows 3 and 4: the crossing's
    shortfall (0.52) beats the 0.12 of its neighbours on both"""
    pos, vel, acc, row = cr.tunnelling_case(5, D, (1, 3))
    got, needed, ref, found = run_update(ctx, (pos, vel, acc), 0.5, 0.02)
    assert found["row"].tolist() == [row - 10, row, row + 10]
    compare_tables(got, ref, f"three segments D={D}")
    assert got["row"].tolist() == [row - 10, row, row + 10, row + 20]
    # (the crossing's distance is the root of a minimum of f that is 0 to a few eps S^2: up to ~1e-7)
    assert np.allclose(got["margin"], [0.12, 0.52, 0.52, 0.12], rtol=0, atol=1e-6)
    assert np.array_equal(got["eta"][1], got["eta"][2]) and got["eta"][0][0] == 1.0 and got["eta"][3][0] == -1.0


@pytest.mark.parametrize("D", [2, 3])
def test_update_two_pieces_in_the_last_segment(ctx, D):
    """a conflict in segment K - 1 proposes one row only: after it comes the final state"""
    host = two_pieces(D)
    got, needed, ref, found = run_update(ctx, host, 0.3, 0.02)
    assert found.size == 1 and int(found["row"][0]) == 1 * 3 + 2 and found["pieces"][0] == 2
    compare_tables(got, ref, f"two pieces D={D}")
    assert got["row"].tolist() == [5]


def test_second_update_adds_the_margins(ctx):
    host = tunnels(6, 2, [(0, 4), (2, 3)])
    first, _, ref1, found = run_update(ctx, host, 0.5, 0.02)
    compare_tables(first, ref1, "first update")
    second, needed, ref2, _ = run_update(ctx, host, 0.5, 0.02, table=first)
    compare_tables(second, ref2, "second update")
    assert needed == first.size == 8 and second["row"].tolist() == first["row"].tolist()
    assert np.abs(second["margin"] - 2 * first["margin"]).max() <= 8 * EPS
    # a table that holds other rows too: they stay as they are, between the new ones
    other = np.zeros(2, dtype=hr.HOLD_DTYPE)
    other["row"], other["margin"] = [1, int(first["row"][3]) + 1], [0.25, 0.5]
    other["eta"][:, 1] = 1.0
    mixed, _, ref3, _ = run_update(ctx, host, 0.5, 0.02, table=other)
    compare_tables(mixed, ref3, "mixed table")
    assert mixed.size == 10 and mixed[0].tobytes() == other[0].tobytes()


def test_update_pair_range_cuts_the_list(ctx):
    host = tunnels(6, 2, [(0, 4), (2, 3)])  # pair indices 3 and 9
    whole, _, _, found = run_update(ctx, host, 0.5, 0.02)
    low, _, ref_low, _ = run_update(ctx, host, 0.5, 0.02, q0=0, q1=9)
    high, _, ref_high, _ = run_update(ctx, host, 0.5, 0.02, q0=9, q1=15)
    compare_tables(low, ref_low, "pairs [0, 9)")
    compare_tables(high, ref_high, "pairs [9, 15)")
    assert low.size == high.size == 4 and set((low["row"] % 15).tolist()) == {3} and set((high["row"] % 15).tolist()) == {9}
    both = np.sort(np.concatenate([low, high]), order="row")
    assert both.tobytes() == whole.tobytes()
    none, needed, _, _ = run_update(ctx, host, 0.5, 0.02, q0=4, q1=9)
    assert none.size == 0 and needed == 0


def test_update_capacity_too_small(ctx):
    host = tunnels(6, 2, [(0, 4), (2, 3)])
    start = np.zeros(2, dtype=hr.HOLD_DTYPE)
    start["row"], start["margin"] = [1, 2], [0.25, 0.5]
    start["eta"][:, 0] = 1.0
    got, needed, ref, _ = run_update(ctx, host, 0.5, 0.02, table=start, capacity=9, grow=False)
    assert needed == ref.size == 10 and got.tobytes() == start.tobytes()  # untouched, the size needed reported
    got, needed, ref, _ = run_update(ctx, host, 0.5, 0.02, table=start, capacity=9)  # ... and the repetition fits
    compare_tables(got, ref, "after growing")
    got, needed, ref, _ = run_update(ctx, host, 0.5, 0.02, table=start, capacity=10, grow=False)  # exactly enough
    compare_tables(got, ref, "capacity 10")


def test_update_longer_than_one_workgroup(ctx):
    """160 disjoint tunnelling pairs: 480 conflicts, 640 holds -- more than the 256 threads of a workgroup at every stage"""
    N = 320
    host = tunnels(N, 2, [(2 * m, 2 * m + 1) for m in range(160)])
    got, needed, ref, found = run_update(ctx, host, 0.5, 0.02)
    assert found.size == 480 and needed == 640
    compare_tables(got, ref, "160 pairs")
    again, _, ref2, _ = run_update(ctx, host, 0.5, 0.02, table=got)
    compare_tables(again, ref2, "160 pairs, second update")


# ---- 2. the plane overwrite --------------------------------------------------------------------------------------------------
def apply_case(ctx, D, q0, q1, seed):
    from path_planning import _hip

    N, K, R, h = 7, 6, 0.8, 0.3
    pairs = N * (N - 1) // 2
    q1 = pairs if q1 is None else q1
    rng = np.random.default_rng(seed)
    pos, p0, v0 = rng.uniform(0.0, 4.0, (N, K, D)), rng.uniform(0.0, 4.0, (N, D)), rng.uniform(-1.0, 1.0, (N, D))
    pp = _hip.PairPass(ctx, N, K, D, R, h, q0, q1)
    d_p0, d_v0 = ctx.tensor(p0), ctx.tensor(v0)
    selected, _, _ = pp.linearize(ctx.tensor(pos), d_p0, d_v0, 0.5)
    selected = selected.cpu().numpy()
    in_range = np.array([k * pairs + q for k in range(K) for q in range(q0, q1)])
    free = np.setdiff1d(in_range, selected)
    assert selected.size >= 3 and free.size >= 5
    outside = np.setdiff1d(np.arange(K * pairs), in_range)
    rows = np.concatenate([rng.choice(selected, 3, replace=False), rng.choice(free, 5, replace=False),
                           rng.choice(outside, min(3, outside.size), replace=False)])
    table = np.zeros(rows.size, dtype=hr.HOLD_DTYPE)
    table["row"] = np.sort(rows)
    e = rng.normal(size=(rows.size, D))
    table["eta"][:, :D] = e / np.linalg.norm(e, axis=1)[:, None]
    table["margin"] = rng.uniform(0.0, 0.4, rows.size)
    return pp, table, (N, K, D, h, R, p0, v0), (d_p0, d_v0)


def plane_state(pp):
    return pp.eta.cpu().numpy().copy(), pp.l.cpu().numpy().copy(), pp.bitmap.cpu().numpy().view(np.uint32).copy()


@pytest.mark.parametrize("D, q0, q1", [(2, 0, None), (3, 0, None), (2, 3, 17), (3, 5, 21)])
def test_apply_against_the_reference(ctx, D, q0, q1):
    pp, table, shape, (d_p0, d_v0) = apply_case(ctx, D, q0, q1, 100 + D)
    N, K, D, h, R, p0, v0 = shape
    eta0, l0, bits0 = plane_state(pp)
    rows0 = (pp.eta_rows().cpu().numpy().copy(), pp.l_rows().cpu().numpy().copy())
    t_dev, n_dev = ctx.hold_table(table)
    new = pp.apply_holds(t_dev, n_dev, d_p0, d_v0).cpu().numpy()
    eta1, l1, bits1 = plane_state(pp)
    ref_eta, ref_l, ref_bits, ref_new = hr.apply(table, N, K, D, h, R, p0, v0, rows0[0], rows0[1], bits0, pp.q_begin, pp.q_end)
    pairs = N * (N - 1) // 2
    held = [int(r) for r in table["row"] if pp.q_begin <= int(r) % pairs < pp.q_end]
    local = np.array([(r // pairs) * pp.nq + (r % pairs - pp.q_begin) for r in held])
    print(f"D={D} pairs [{pp.q_begin}, {pp.q_end}): {len(held)} of {table.size} holds in range, {new.size} new rows")
    assert new.tolist() == ref_new.tolist() and (np.diff(new) > 0).all() and new.size == 5
    assert np.array_equal(bits1, ref_bits)
    # the held entries
    got_eta = pp.eta_rows().cpu().numpy()
    assert got_eta[local].tobytes() == ref_eta[local].tobytes()
    err = np.abs(l1[local] - ref_l[local])
    print(f"worst |l - ref| = {float((err / np.maximum(1.0, np.abs(ref_l[local]))).max()) / EPS:.2f} eps max(1, |l|) (bound 4)")
    assert (err <= 4 * EPS * np.maximum(1.0, np.abs(ref_l[local]))).all()
    # every other entry of the planes (the padding of the strides included) keeps its bits
    keep_eta = np.ones(eta0.size, dtype=bool)
    for d in range(D):
        keep_eta[d * pp.stride + local] = False
    keep_l = np.ones(l0.size, dtype=bool)
    keep_l[local] = False
    assert eta1.view(np.uint64)[keep_eta].tobytes() == eta0.view(np.uint64)[keep_eta].tobytes()
    assert l1.view(np.uint64)[keep_l].tobytes() == l0.view(np.uint64)[keep_l].tobytes()
    # a second call: everything is marked now, nothing is new, the same bytes
    again = pp.apply_holds(t_dev, n_dev, d_p0, d_v0)
    assert again.numel() == 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plane_state(pp), (eta1, l1, bits1)))


def test_apply_list_too_short_writes_nothing(ctx):
    import torch

    pp, table, shape, (d_p0, d_v0) = apply_case(ctx, 2, 0, None, 7)
    before = plane_state(pp)
    t_dev, n_dev = ctx.hold_table(table)
    n_new = torch.zeros(1, dtype=torch.int64, device=ctx.tdev)
    rows = torch.full((8,), -1, dtype=torch.int64, device=ctx.tdev)

    def call(cap):
        ctx.check(ctx.lib.scp_apply_holds(ctx.h, pp.N, pp.K, pp.D, pp.h, pp.R, pp.q_begin, pp.q_end, t_dev.data_ptr(),
                                          n_dev.data_ptr(), d_p0.data_ptr(), d_v0.data_ptr(), pp.eta.data_ptr(), pp.l.data_ptr(),
                                          pp.bitmap.data_ptr(), rows.data_ptr(), cap, n_new.data_ptr()))
        return int(n_new.item())

    assert call(4) == 5  # five holds are not selected yet: the list of four is too short
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plane_state(pp), before))
    assert (rows.cpu().numpy() == -1).all()
    assert call(5) == 5
    assert (np.diff(rows.cpu().numpy()[:5]) > 0).all() and plane_state(pp)[2].tobytes() != before[2].tobytes()


# ---- 3. end to end -----------------------------------------------------------------------------------------------------------
BOUNDS = ("acc_violation", "jerk_violation", "vel_violation", "pos_violation", "final_position_error", "final_velocity_error")
QP_TOL = 1e-3 + 1e-3 * 20.0  # eps_abs + eps_rel * the largest bound of a fixed row (jerk 20, position 20)


def make_solver(N, T, h, p0, pf, R=0.5):
    from path_planning.solvers.scp import SCP

    s = SCP(n_vehicles=N, time_horizon=T, time_step=h, min_distance=R, space_dims=[0, 0, 20, 20], device=0, verbose=False)
    s.set_initial_states(p0)
    s.set_final_states(pf)
    return s


@pytest.mark.parametrize("N, rad, T, h, seed", [(12, 6.0, 7.5, 0.3, 12), (16, 6.0, 7.5, 0.3, 13), (20, 7.0, 8.0, 0.25, 22)])
def test_repair_clears_the_ring_scenarios(N, rad, T, h, seed):
    R = 0.5
    p0, pf = hr.ring_scenario(N, rad, seed)
    s = make_solver(N, T, h, p0, pf, R)
    s.generate_trajectories(max_iterations=15)
    before = s.validate_solution(continuous=True, conflicts=True)
    print(f"ring N={N} seed={seed}: {before['n_conflicts']} conflicts ({before['n_violating_segments']} segments) before")
    assert before["n_conflicts"] >= 1
    rep = s.repair_conflicts()
    after = s.validate_solution(continuous=True, conflicts=True)
    print(f"  repair: {rep}")
    print("  bounds before / after: " + ", ".join(f"{k} {before[k]:.2e} / {after[k]:.2e}" for k in BOUNDS))
    print(f"  sample minimum {after['min_pair_distance']:.6f}, continuous minimum {after['min_pair_distance_continuous']:.6f}")
    assert rep["conflicts_before"] == before["n_violating_segments"]
    assert after["n_conflicts"] == 0 and rep["repaired"] is True and rep["stopped_by"] == "clean"
    assert rep["conflicts_per_pass"][-1] == 0 and len(rep["conflicts_per_pass"]) == rep["passes"] <= 6
    assert after["min_pair_distance"] >= R - 0.01
    for key in BOUNDS:
        assert after[key] <= QP_TOL, key
    assert s.last_info["repair"] is rep and rep["holds"] >= 2 and rep["cost_ratio"] > 0.0
    s.close()


def test_repair_without_a_conflict_changes_nothing():
    N = 4
    p0 = np.stack([np.full(N, 2.0), 2.0 + 3.0 * np.arange(N)], axis=1)
    pf = p0 + [16.0, 0.0]
    s = make_solver(N, 12.0, 0.5, p0, pf)
    with pytest.raises(ValueError):
        s.repair_conflicts()  # nothing stored yet
    s.generate_trajectories(max_iterations=15)
    kept = {k: v.copy() for k, v in s.trajectories.items()}
    stored = s.trajectories
    rep = s.repair_conflicts()
    assert rep["passes"] == 0 and rep["conflicts_before"] == 0 and rep["repaired"] and rep["stopped_by"] == "clean"
    assert rep["conflicts_per_pass"] == [] and rep["holds"] == 0 and rep["cost_ratio"] == 1.0
    assert s.trajectories is stored and all(np.array_equal(kept[k], s.trajectories[k]) for k in kept)
    s.close()


def test_cli_prints_the_repair_report(capsys):
    from path_planning.cli import compute_trajectories

    solver = compute_trajectories.main(["--n-agents", "4", "--time-horizon", "10", "--time-step", "0.5", "--min-distance", "0.8",
                                        "--space", "0", "0", "20", "20", "--seed", "1", "--no-plots", "--repair-conflicts"])
    out = capsys.readouterr().out
    print(out)
    assert solver is not None and "Conflict repair:" in out and "passes" in out
    assert "repair" in solver.last_info
