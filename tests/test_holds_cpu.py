"""Holds on the CPU: the reference of the table update and of the plane overwrite (tests/holds_ref.py) against the rule's own
claims -- the sufficient condition, the repair loop on the QP oracle -- and the binding's struct against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import conflicts_ref as cr
import holds_ref as hr
from oracle import qp_oracle as qo
from oracle import scp_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def conflict_array(rec):
    """conflicts_ref.records -> the fields of scp_conflict the rule reads"""
    out = np.zeros(rec["rows"].size, dtype=[("row", np.uint64), ("min_dist", np.float64), ("t_min", np.float64)])
    out["row"], out["t_min"] = rec["rows"], rec["t_min"]
    out["min_dist"] = np.sqrt(np.maximum(rec["f"], 0.0))
    return out


def test_sufficient_condition_on_random_held_segments():
    """the rows k and k + 1 of a pair hold the same eta with margin c -> eta . d(t) >= R + c - |eta . da| h^2 / 8 over segment k"""
    rng = np.random.default_rng(7)
    R, h = 0.5, 0.25
    checked = 0
    while checked < 200:
        D = 2 + checked % 2
        eta = rng.normal(size=D)
        eta /= np.linalg.norm(eta)
        c = rng.uniform(0.0, 0.3)
        da = rng.uniform(-30.0, 30.0, D) / np.sqrt(D)  # |da| <= 30
        dv = rng.uniform(-4.0, 4.0, D)
        dp = rng.uniform(-2.0, 2.0, D)
        end = dp + h * dv + 0.5 * h * h * da
        if eta @ dp < R + c or eta @ end < R + c:
            # move the pair along eta until both ends of the segment are held (the motion within the segment is unchanged)
            dp = dp + eta * (R + c - min(eta @ dp, eta @ end) + rng.uniform(0.0, 0.05))
        assert np.linalg.norm(da) <= 30.0
        low = hr.held_minimum(eta, dp, dv, da, h)
        assert low >= R + c - abs(eta @ da) * h * h / 8 - 1e-12
        # and the distance is at least the held component, all along the segment
        t = np.linspace(0.0, h, 101)[:, None]
        d = dp + t * dv + 0.5 * t * t * da
        assert (np.linalg.norm(d, axis=1) >= d @ eta - 1e-12).all()
        assert (d @ eta).min() >= low - 1e-12
        checked += 1


def test_reference_update_rules():
    """two candidates on one row: the larger shortfall wins; a second update adds the margins; the last segment gives one row"""
    pos, vel, acc, row = cr.tunnelling_case(5, 2, (1, 3))
    N, K, D = pos.shape
    pairs = N * (N - 1) // 2
    h, R = 0.2, 0.5
    every = conflict_array(cr.records(pos, vel, acc, h, R))
    # the pair approaches in segment 2 (0.4 m at its end), crosses in segment 3 and parts in segment 4
    assert every["row"].tolist() == [row - pairs, row, row + pairs]
    t0 = hr.update(hr.empty_table(), pos, vel, acc, R, every, 0.02)
    assert t0["row"].tolist() == [row - pairs, row, row + pairs, row + 2 * pairs]
    assert np.allclose(t0["margin"], [0.12, 0.52, 0.52, 0.12])  # the crossing's shortfall wins on both of its rows
    assert np.allclose(t0["eta"][:, :2], [[1, 0], [0, -1], [0, -1], [-1, 0]])
    rec = every[1:2]
    t1 = hr.update(hr.empty_table(), pos, vel, acc, R, rec, 0.02)
    assert t1["row"].tolist() == [row, row + pairs]
    # d(t_min) = 0: the perpendicular of the relative velocity (-4, 0) -> (0, -1)
    assert np.allclose(t1["eta"][0], [0.0, -1.0, 0.0]) and np.array_equal(t1["eta"][0], t1["eta"][1])
    assert np.allclose(t1["margin"], R - rec["min_dist"][0] + 0.02)
    t2 = hr.update(t1, pos, vel, acc, R, rec, 0.02)
    assert t2["row"].tolist() == t1["row"].tolist() and np.allclose(t2["margin"], 2 * t1["margin"])
    # conflicts in the segments 3 and 4 of one pair meet on row 4
    two = np.concatenate([rec, rec])
    two["row"][1] += pairs
    two["min_dist"] = [0.3, 0.1]
    t3 = hr.update(hr.empty_table(), pos, vel, acc, R, two, 0.0)
    assert t3["row"].tolist() == [row, row + pairs, row + 2 * pairs]
    assert np.allclose(t3["margin"], [0.2, 0.4, 0.4])
    last = rec.copy()
    last["row"] = (K - 1) * pairs + row % pairs
    assert hr.update(hr.empty_table(), pos, vel, acc, R, last, 0.0)["row"].tolist() == [int(last["row"][0])]


def oracle_repair(prob, max_passes, pad=0.02, max_iterations=15):
    """the repair loop of SCP.repair_conflicts on the QP oracle -> conflicts before and after every pass, the statuses, and the
    smallest sampled distance of the last accepted pass"""
    st = qo.Settings(max_iter=10000)
    out = qo.scp_solve(prob, max_iterations, st)
    x, pos, vel = out["accelerations"], out["positions"], out["velocities"]
    found = conflict_array(cr.records(pos, vel, x, prob.h, prob.R))
    counts, statuses = [int(found.size)], []
    table = hr.empty_table()
    while found.size and len(counts) <= max_passes:
        table = hr.update(table, pos, vel, x, prob.R, found, pad)
        held = table["row"].astype(np.int64)
        for _ in range(max_iterations):
            prev_pos, _ = so.kinematics(prob, x)
            eta, l_col, dist = so.linearize_pairs(prob, prev_pos)
            for t in table:
                eta[int(t["row"])] = t["eta"][: prob.D]
                l_col[int(t["row"])] = hr.hold_bound(t, prob.N, prob.D, prob.h, prob.R, prob.p0, prob.v0)
            rows0 = np.union1d(np.nonzero(dist - prob.R < st.margin)[0], held).astype(np.int64)
            x_new, _, info = qo.admm_structured(prob, eta, l_col, dist, x0=x, st=st, rows0=rows0)
            statuses.append(info["status_val"])
            if info["status_val"] not in (1, 2):
                return counts, statuses, None
            rel = float(np.linalg.norm((x_new - x).ravel()) / np.linalg.norm(x.ravel()))
            x = x_new
            if rel <= prob.convergence_tolerance:
                break
        pos, vel = so.kinematics(prob, x)
        found = conflict_array(cr.records(pos, vel, x, prob.h, prob.R))
        counts.append(int(found.size))
    return counts, statuses, so.min_pair_distance(prob, pos)


@pytest.mark.parametrize("N, rad, T, h, seed", [(6, 4.0, 5.0, 0.25, 2), (10, 5.0, 6.0, 0.25, 4)])
def test_repair_loop_on_the_oracle_clears_the_random_cases(N, rad, T, h, seed):
    R = 0.5
    p0, pf = hr.ring_scenario(N, rad, seed, random_angles=True)
    prob = so.make_problem(N, T, h, R, [0, 0, 20, 20], p0, pf)
    counts, statuses, sample_min = oracle_repair(prob, max_passes=3)
    print(f"N={N} seed={seed}: conflicts {counts}, QP statuses {sorted(set(statuses))}, sample minimum {sample_min}")
    assert counts[0] > 0, "the scenario has no conflict to repair"
    assert counts[-1] == 0 and len(counts) - 1 <= 3
    assert set(statuses) <= {1, 2}
    assert sample_min >= R - 0.01


class _FakeSolver:
    """stands in for SCP in run_single_trial (no GPU here): records the repairs that were asked for"""
    K, T, h = 5, 1.0, 0.2
    calls = []

    def __init__(self, **kw):
        step = {"time_sec": 0.0, "rel_step": 0.0, "iter": 1, "status": "solved", "r_prim": 0.0, "r_dual": 0.0, "working_rows": 0}
        self.last_info = {"n_iterations": 1, "converged": True, "qp0": dict(step), "iterations": [dict(step)]}

    def set_initial_states(self, p):
        pass

    def set_final_states(self, p):
        pass

    def generate_trajectories(self, max_iterations):
        return {}

    def repair_conflicts(self, max_passes=6, pad=0.02, max_iterations=15):
        _FakeSolver.calls.append(max_passes)
        return {"conflicts_before": 4, "conflicts_per_pass": [2, 0], "passes": 2}


def test_surface_and_batch_record_schema(monkeypatch):
    """the flag on both CLIs, opt-in; a batch record gains its three fields only with the flag; the CSV fields are unchanged"""
    import inspect

    from path_planning.cli import compute_trajectories
    from path_planning.cli import compute_trajectories_batch as ctb
    from path_planning.solvers.scp import SCP

    sig = inspect.signature(SCP.repair_conflicts)
    assert [sig.parameters[k].default for k in ("max_passes", "pad", "max_iterations")] == [6, 0.02, 15]
    for cli in (compute_trajectories, ctb):
        parse = cli.build_parser().parse_args
        assert parse([]).repair_conflicts is None and parse(["--repair-conflicts"]).repair_conflicts == 6
        assert parse(["--repair-conflicts", "3"]).repair_conflicts == 3
    assert "repair_conflicts" not in ctb.CONFIG
    assert ctb.CSV_FIELDS == ["N", "trial_index", "status", "time_sec", "K", "T", "h", "error"]
    monkeypatch.setattr(ctb, "SCP", _FakeSolver)
    cfg = dict(ctb.CONFIG, validate=False)
    scen = (np.zeros((2, 2)), np.ones((2, 2)), [0, 0, 20, 20])
    base = ctb.run_single_trial(2, cfg, scenario=scen)
    assert not _FakeSolver.calls
    rec = ctb.run_single_trial(2, dict(cfg, repair_conflicts=3), scenario=scen)
    assert list(rec) == list(base) + ["conflicts_before", "conflicts_after", "repair_passes"] and _FakeSolver.calls == [3]
    assert (rec["conflicts_before"], rec["conflicts_after"], rec["repair_passes"]) == (4, 0, 2)


def test_hold_struct_matches_the_header():
    from path_planning import _hip

    assert C.sizeof(_hip.Hold) == 48 == _hip.HOLD_DTYPE.itemsize == hr.HOLD_DTYPE.itemsize
    offsets = {"row": 0, "eta": 8, "margin": 32, "reserved": 40}
    for name, off in offsets.items():
        assert getattr(_hip.Hold, name).offset == off == _hip.HOLD_DTYPE.fields[name][1] == hr.HOLD_DTYPE.fields[name][1]
    text = open(os.path.join(ROOT, "include", "scp_hip.h")).read()
    body = re.search(r"typedef struct scp_hold \{(.*?)\} scp_hold;", text, re.S).group(1)
    fields = re.findall(r"^\s*(uint64_t|double)\s+(\w+)(\[3\])?;", body, re.M)
    assert [(t, n, bool(a)) for t, n, a in fields] == [("uint64_t", "row", False), ("double", "eta", True),
                                                         ("double", "margin", False), ("uint64_t", "reserved", False)]
    assert "scp_update_holds" in _hip.EXPORTS and "scp_apply_holds" in _hip.EXPORTS
    assert int(re.search(r"#define SCP_HOLD_MAX_TABLE \(1 << (\d+)\)", text).group(1)) == 20 and _hip.HOLD_MAX_TABLE == 1 << 20
