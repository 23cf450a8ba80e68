"""GPU tests of the order search of the staggered starts -- scp_schedule_starts_batch, SCP.stagger_starts(search=...) and the CLI
flags -- against the reference of tests/stagger_search_ref.py (pinned on the CPU by tests/test_stagger_search_cpu.py) and, where
Python is too slow, against scp_schedule_starts on the same device masks.  Integers only: equality throughout."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stagger_ref as st  # noqa: E402
import stagger_search_ref as ss  # noqa: E402

pytestmark = pytest.mark.gpu

# (N, S, density, seed, B): a word boundary of `pending` (33, 65), shift counts 0 and 63, many unplaced vehicles
CASES = [(1, 0, None, None, 3), (2, 0, 0.5, 7, 2), (33, 5, 0.10, 1, 36), (40, 8, 0.15, 2, 36), (65, 63, 0.30, 4, 8),
         (130, 20, 0.05, 5, 12)]
_REFS = {}


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def case(N, S, density, seed, B, symmetric=True):
    """masks, candidate orders and the reference's (delays, stats) of every candidate, made once"""
    from path_planning.solvers.stagger import candidate_orders

    key = (N, S, density, seed, B, symmetric)
    if key not in _REFS:
        m = np.zeros((1, 1), dtype=np.uint64) if density is None else st.random_masks(N, S, density, seed, symmetric=symmetric)
        orders = candidate_orders(N, B, np.random.default_rng((seed or 0) + 100))
        _REFS[key] = (m, orders) + ss.schedule_all(m, S, orders)
    return _REFS[key]


def assert_matches(got, want_delays, want_stats, objective, label):
    delays, stats, best = got
    B, N = len(want_delays), len(want_delays[0])
    assert delays.dtype == np.int32 and delays.shape == (B, N), label
    assert delays.tolist() == want_delays, label
    for f in ss.FIELDS:
        assert stats[f].shape == (B,) and stats[f].tolist() == [s[f] for s in want_stats], (label, f)
    assert stats["reserved"].shape == (B, 3) and not stats["reserved"].any(), label
    assert best == ss.best_of(want_stats, objective), label


def as_bytes(got):
    delays, stats, best = got
    return delays.tobytes() + b"".join(stats[f].tobytes() for f in sorted(stats)) + bytes([best & 255, best >> 8])


# ---- 1. against the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,density,seed,B", CASES)
def test_batch_vs_reference(ctx, N, S, density, seed, B):
    m, orders, want_delays, want_stats = case(N, S, density, seed, B)
    for objective in ss.OBJECTIVES:
        got = ctx.schedule_starts_batch(m, S, orders, objective)
        assert_matches(got, want_delays, want_stats, objective, (N, S, objective))
        assert as_bytes(ctx.schedule_starts_batch(m, S, orders, objective)) == as_bytes(got)  # a second run: the same bytes
    u = [s["n_unplaced"] for s in want_stats]
    print(f"batch N={N} S={S} B={B}: unplaced {min(u)} .. {max(u)}, best {[ss.best_of(want_stats, o) for o in ss.OBJECTIVES]}")
    if N >= 65:
        assert min(u) > 0


def test_batch_vs_reference_asymmetric_masks(ctx):
    """bit 0 is NOT symmetric: the schedule must read mask[v][u] for d >= d_u and mask[u][v] for d < d_u, as the rule says"""
    m, orders, want_delays, want_stats = case(65, 7, 0.05, 11, 6, symmetric=False)
    assert (m & np.uint64(1) != m.T & np.uint64(1)).any()
    for objective in ss.OBJECTIVES:
        assert_matches(ctx.schedule_starts_batch(m, 7, orders, objective), want_delays, want_stats, objective, objective)


def test_objectives_pick_different_candidates(ctx):
    """the inputs of tests/test_stagger_search_cpu.py::test_reference_objectives_can_disagree"""
    from path_planning.solvers.stagger import candidate_orders

    m = st.random_masks(12, 6, 0.2, 8)
    orders = candidate_orders(12, 8, np.random.default_rng(8))
    want_delays, want_stats = ss.schedule_all(m, 6, orders)
    want = [ss.best_of(want_stats, o) for o in ss.OBJECTIVES]
    assert want[0] != want[1]
    for objective, b in zip(ss.OBJECTIVES, want):
        got = ctx.schedule_starts_batch(m, 6, orders, objective)
        assert_matches(got, want_delays, want_stats, objective, objective)
        assert got[2] == b


# ---- 2. against scp_schedule_starts where Python is too slow --------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,B", [(1025, 10, 4), (6200, 10, 2)])  # threads loop twice over the vehicles; LDS above 48 KiB
def test_batch_vs_single_schedule_on_device_masks(ctx, N, S, B):
    import torch

    from path_planning.solvers.stagger import candidate_orders

    gen = torch.Generator(device=ctx.tdev).manual_seed(N)
    mask = torch.zeros((N, N), dtype=torch.int64, device=ctx.tdev)
    for s in range(S + 1):  # every bit 0 .. S of every off-diagonal word with probability 1.5 / N
        mask |= (torch.rand((N, N), device=ctx.tdev, generator=gen) < 1.5 / N).to(torch.int64) << s
    mask.fill_diagonal_(0)
    orders = candidate_orders(N, B, np.random.default_rng(N))
    singles = [ctx.schedule_starts(mask, S, order) for order in orders]
    want_stats = [s for _, s in singles]
    assert all(s["n_delayed"] > 0 for s in want_stats) and any(s["n_unplaced"] > 0 for s in want_stats)  # the masks bite
    for objective in ss.OBJECTIVES:
        got = ctx.schedule_starts_batch(mask, S, orders, objective)
        assert_matches(got, [d.tolist() for d, _ in singles], want_stats, objective, (N, objective))
    print(f"batch N={N}: {[(s['n_unplaced'], s['max_delay'], s['total_delay']) for s in want_stats]}")


# ---- 3. one candidate -------------------------------------------------------------------------------------------------------------------
def test_one_candidate_is_the_single_schedule(ctx):
    m, orders, want_delays, want_stats = case(130, 20, 0.05, 5, 12)
    d1, s1 = ctx.schedule_starts(m, 20)
    delays, stats, best = ctx.schedule_starts_batch(m, 20, np.arange(130, dtype=np.int32)[None, :])
    assert best == 0 and delays.shape == (1, 130) and delays[0].tobytes() == d1.tobytes()
    assert {f: int(stats[f][0]) for f in ss.FIELDS} == s1 == want_stats[0] and not stats["reserved"].any()


# ---- 4. more workgroups than compute units -----------------------------------------------------------------------------------------
def test_three_hundred_candidates(ctx):
    m, orders, want_delays, want_stats = case(40, 8, 0.15, 9, 300)
    for objective in ss.OBJECTIVES:
        assert_matches(ctx.schedule_starts_batch(m, 8, orders, objective), want_delays, want_stats, objective, objective)
    assert len({tuple(d) for d in want_delays}) > 100  # the candidates do differ


# ---- 5. threads per workgroup, transposed copy ------------------------------------------------------------------------------------------
def test_threads_per_workgroup_do_not_show():
    from path_planning import _hip

    N, S, density, seed, B = CASES[-1]
    m, orders, want_delays, want_stats = case(N, S, density, seed, B)
    c = _hip.Context(0)
    try:
        seen = []
        for threads in (256, 1024, 0):
            c.set_option("stg_batch_threads", threads)
            got = c.schedule_starts_batch(m, S, orders, "total")
            assert_matches(got, want_delays, want_stats, "total", threads)
            seen.append(as_bytes(got))
        assert seen[0] == seen[1] == seen[2]
        am, aorders, adelays, astats = case(65, 7, 0.05, 11, 6, symmetric=False)  # (a mask that is not its own transpose)
        for transposed in (1, 0, -1):  # the columns of the masks read from a transposed copy: always, never, chosen by the call
            c.set_option("stg_batch_transposed", transposed)
            for threads in (256, 1024):
                c.set_option("stg_batch_threads", threads)
                got = c.schedule_starts_batch(m, S, orders, "total")
                assert_matches(got, want_delays, want_stats, "total", (transposed, threads))
                assert as_bytes(got) == seen[0]
                assert_matches(c.schedule_starts_batch(am, 7, aorders), adelays, astats, "makespan", (transposed, threads))
        for bad in (-2, 2):
            with pytest.raises(_hip.HipError):
                c.set_option("stg_batch_transposed", bad)
        for bad in (-1, 64, 512):
            with pytest.raises(_hip.HipError) as err:
                c.set_option("stg_batch_threads", bad)
            assert err.value.code == -1
    finally:
        c.close()


# ---- 6. invalid input -----------------------------------------------------------------------------------------------------------------
def test_a_non_permutation_is_named(ctx):
    import ctypes as C

    import torch

    from path_planning import _hip

    N, S = 130, 5
    m = st.random_masks(N, S, 0.01, 5)
    good = np.stack([np.random.default_rng(i).permutation(N) for i in range(3)]).astype(np.int32)
    twice, beyond, below = good.copy(), good.copy(), good.copy()
    twice[2] = np.where(good[2] == 7, 8, good[2])   # vehicle 8 named twice, 7 never
    beyond[2] = np.where(good[2] == 7, N, good[2])  # an entry out of range
    below[2] = np.where(good[2] == 7, -1, good[2])
    for bad in (twice, beyond, below):
        with pytest.raises(_hip.HipError) as err:
            ctx.schedule_starts_batch(m, S, bad)
        assert err.value.code == -1 and "scp_schedule_starts_batch: candidate 2 is not a permutation" in str(err.value)
    both = twice.copy()
    both[1] = beyond[2]
    with pytest.raises(_hip.HipError) as err:
        ctx.schedule_starts_batch(m, S, both)
    assert "candidate 1 is not a permutation" in str(err.value)  # the lowest one
    want_delays, want_stats = ss.schedule_all(m, S, good)  # the context is still usable
    assert_matches(ctx.schedule_starts_batch(m, S, good), want_delays, want_stats, "makespan", "after the errors")

    dm = torch.as_tensor(m.view(np.int64)).to(ctx.tdev)
    od = torch.as_tensor(good).to(ctx.tdev)
    delay = torch.zeros((3, N), dtype=torch.int32, device=ctx.tdev)
    stats = torch.zeros(3 * 48, dtype=torch.uint8, device=ctx.tdev)
    best = C.c_int32(-1)
    ptrs = [dm.data_ptr(), od.data_ptr(), delay.data_ptr(), stats.data_ptr(), C.byref(best)]

    def call(N=N, S=S, B=3, objective=0, null=None, h=ctx.h):
        p = [None if i == null else x for i, x in enumerate(ptrs)]
        return ctx.lib.scp_schedule_starts_batch(h, N, S, p[0], B, p[1], objective, p[2], p[3], p[4])

    assert call() == 0 and best.value == ss.best_of(want_stats, "makespan")
    for kw in ({"B": 0}, {"B": -1}, {"B": 65536}, {"objective": 2}, {"objective": -1}, {"N": 0}, {"N": 16385}, {"S": -1}, {"S": 64}):
        assert call(**kw) == -1, kw
        assert "scp_schedule_starts_batch" in ctx.lib.scp_last_error(ctx.h).decode()
    for null in range(5):  # mask, orders, delay, stats, best
        assert call(null=null) == -1 and "null pointer" in ctx.lib.scp_last_error(ctx.h).decode()
    assert call(h=None) == -1
    assert call(objective=1) == 0 and best.value == ss.best_of(want_stats, "total")
    assert ctx.last_pair_ms() >= 0.0
    for shape in ((3, N - 1), (N,), (0, N)):  # the binding checks the shape on the host
        with pytest.raises(ValueError):
            ctx.schedule_starts_batch(m, S, np.zeros(shape, dtype=np.int32))
    with pytest.raises(ValueError):
        ctx.schedule_starts_batch(m, S, good, objective="shortest")


# ---- 7. SCP.stagger_starts ---------------------------------------------------------------------------------------------------------------
def ring_problem(N, jitter_seed=None):
    """starts on half a circle, every goal opposite its start: everybody straight through the centre"""
    u = np.zeros(N) if jitter_seed is None else np.random.default_rng(jitter_seed).uniform(-1, 1, N)
    ang = np.pi * (np.arange(N) + 0.25 * u) / N
    p0 = np.stack([10.0 + 5.0 * np.cos(ang), 10.0 + 5.0 * np.sin(ang)], axis=1)
    return p0, 20.0 - p0


@pytest.mark.parametrize("N,jitter_seed", [(8, None), (12, 1)])
def test_stagger_starts_search(N, jitter_seed):
    from path_planning.solvers.scp import SCP
    from path_planning.solvers.stagger import schedule_key

    p0, pf = ring_problem(N, jitter_seed)
    s = SCP(n_vehicles=N, time_horizon=10.0, time_step=0.5, min_distance=0.8, space_dims=[0, 0, 20, 20], device=0, verbose=False)
    s.set_initial_states(p0)
    s.set_final_states(pf)
    s.generate_trajectories(max_iterations=0)  # QP#0
    stored = {k: v.copy() for k, v in s.trajectories.items()}
    S = 12
    plain = s.stagger_starts(S)
    assert "search" not in plain
    keys = list(plain)
    one = s.stagger_starts(S, search=1, rounds=1)
    assert list(one) == keys + ["search"] and one is s.last_info["stagger"]
    assert one["delays"].tolist() == plain["delays"].tolist() and one["search"]["best_candidate"] == 0
    assert not one["search"]["improved"] and one["search"]["rounds_run"] == 1

    dev = tuple(s._ctx.tensor(stored[k]) for k in ("positions", "velocities", "accelerations"))
    mask = s._ctx.lag_conflicts(N, s.K, s.D, s.h, s.R, *dev, S)
    for objective in ss.OBJECTIVES:
        info = s.stagger_starts(S, search=16, rounds=3, seed=4, objective=objective)
        se = info["search"]
        assert list(se) == ["candidates", "rounds_run", "best_round", "best_candidate", "best_order", "baseline", "improved",
                            "objective"]
        assert se["baseline"] == {k: plain[k] for k in ("n_unplaced", "max_delay", "total_delay", "n_delayed")}
        key = schedule_key(info["n_unplaced"], info["max_delay"], info["total_delay"], objective)
        base = schedule_key(plain["n_unplaced"], plain["max_delay"], plain["total_delay"], objective)
        print(f"ring N={N} {objective}: baseline {base} -> {key}, round {se['best_round']} candidate {se['best_candidate']} of "
              f"{se['rounds_run']} rounds")
        assert key <= base and se["improved"] == (key < base) and se["objective"] == objective and se["candidates"] == 16
        assert 1 <= se["rounds_run"] <= 3 and 0 <= se["best_round"] < se["rounds_run"] and 0 <= se["best_candidate"] < 16
        assert sorted(se["best_order"].tolist()) == list(range(N))
        want, wstats = st.greedy(mask, S, se["best_order"])  # the best order's schedule, by the reference
        assert info["delays"].tolist() == want and info["n_delayed"] == wstats["n_delayed"]
        assert (info["n_unplaced"], info["max_delay"], info["total_delay"]) == (wstats["n_unplaced"], wstats["max_delay"],
                                                                                wstats["total_delay"])
        fleet = tuple(s._ctx.tensor(s.staggered[k]) for k in ("positions", "velocities", "accelerations"))
        after = s._ctx.check_separation(N, info["horizon_steps"], s.D, s.h, s.R, *fleet)
        assert info["conflicts_after"] == int(after["n_violating"]) and (s.staggered["delays"] == info["delays"]).all()
        assert info["schedule_ms"] >= 0.0
        again = s.stagger_starts(S, search=16, rounds=3, seed=4, objective=objective)  # the same seed: the same result
        assert again["delays"].tolist() == info["delays"].tolist()
        assert again["search"]["best_order"].tolist() == se["best_order"].tolist()
        assert (again["search"]["best_round"], again["search"]["best_candidate"]) == (se["best_round"], se["best_candidate"])
    order = np.arange(N)[::-1].copy()  # the search starts from the given order
    rev = s.stagger_starts(S, order=order, search=4)
    base_rev = s.stagger_starts(S, order=order)
    assert rev["search"]["baseline"]["total_delay"] == base_rev["total_delay"]
    assert all(s.trajectories[k].tobytes() == stored[k].tobytes() for k in stored)  # the plans are left as they are
    for bad in ({"search": -1}, {"search": 65536}, {"search": 2.5}, {"search": True}, {"search": 4, "rounds": 0},
                {"search": 4, "rounds": 1.5}, {"rounds": True}, {"search": 4, "objective": "shortest"}, {"objective": None}):
        with pytest.raises(ValueError):
            s.stagger_starts(S, **bad)
    with pytest.raises(TypeError):
        s.stagger_starts(S, None, 4)  # keyword only


# ---- 8. the CLIs ----------------------------------------------------------------------------------------------------------------------
def test_batch_cli_stagger_search(tmp_path):
    from path_planning.cli import compute_trajectories_batch as ctb

    def records(name, extra):
        out = tmp_path / name
        ctb.main(["--Ns", "4", "--trials", "2", "--seed", "5", "--results-dir", str(out)] + extra)
        return json.load(open(next(out.glob("*.json"))))

    without = records("without", [])
    plain = records("plain", ["--stagger-starts", "3"])
    found = records("search", ["--stagger-starts", "3", "--stagger-search", "8", "--stagger-rounds", "2", "--stagger-seed", "1",
                               "--stagger-objective", "makespan"])
    four = ["stagger_max_delay", "stagger_n_delayed", "stagger_n_unplaced", "stagger_conflicts_after"]
    three = ["stagger_search_candidates", "stagger_baseline_n_unplaced", "stagger_baseline_max_delay"]
    assert "stagger_search" not in plain["meta"]["config"] and "stagger_search" not in without["meta"]["config"]
    assert found["meta"]["config"]["stagger_search"] == {"search": 8, "rounds": 2, "seed": 1, "objective": "makespan"}
    for a, b, c in zip(without["runs"], plain["runs"], found["runs"]):
        assert a["status"] == b["status"] == c["status"] == "success"
        assert list(b) == list(a) + four  # without the new flags: today's keys
        assert list(c) == list(b) + three  # with them: three more, at the end
        assert all(isinstance(c[k], int) for k in four + three) and c["stagger_search_candidates"] == 8
        assert (c["stagger_n_unplaced"], c["stagger_max_delay"]) <= (c["stagger_baseline_n_unplaced"], c["stagger_baseline_max_delay"])
        assert 0 <= c["stagger_baseline_max_delay"] <= 3


def test_compute_trajectories_cli_stagger_search(capsys):
    from path_planning.cli import compute_trajectories as ct

    args = ["--n-agents", "4", "--time-horizon", "10", "--time-step", "0.5", "--space", "0", "0", "20", "20", "--seed", "1",
            "--no-plots", "--stagger-starts", "5"]
    solver = ct.main(args)
    assert "order search" not in capsys.readouterr().out and "search" not in solver.last_info["stagger"]
    solver = ct.main(args + ["--stagger-search", "6", "--stagger-rounds", "2", "--stagger-objective", "total"])
    out = capsys.readouterr().out
    info = solver.last_info["stagger"]
    se = info["search"]
    assert se["candidates"] == 6 and se["objective"] == "total" and 1 <= se["rounds_run"] <= 2
    line = [x for x in out.split("\n") if x.startswith("  order search (total): 6 candidates x ")]
    assert len(line) == 1 and f"{se['baseline']['n_unplaced']} unplaced" in line[0]
    assert len([x for x in out.split("\n") if x.startswith("Staggered starts: ")]) == 1
