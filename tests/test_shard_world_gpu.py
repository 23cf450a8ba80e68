"""The sharded SCP step (scp_solver_shard_*) in simulated worlds of many ranks, one process, against the one-rank step
(scp_solver_step, bit for bit) and against the numpy oracle (which ids each rank finds, what its last violations pass
reports).  tests/shard_cases.py places the cuts so that the ranks of one world run different forms of the pairwise passes;
the near-pass counters of each rank's context tell that they did."""
import numpy as np
import pytest

import shard_cases as sc
from oracle import scp_oracle as so

pytestmark = pytest.mark.gpu

POS_IN = [False, True]
MAX_V_TOL = 1e-11  # (test_collision_violations_pass's)
_REF, _WORLD = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    scp_of(None)
    _REF.clear()
    _WORLD.clear()


def same_records(a, b):
    keys = ("status_val", "iter", "rho_updates", "cg_iters_total", "working_rows", "rounds", "added", "unresolved_rows",
            "status")
    for k in keys:
        assert a[k] == b[k], (k, a[k], b[k])
    for k in ("r_prim", "r_dual", "rho", "max_violation"):
        assert a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])), (k, a[k], b[k])


def scenario_key(case):
    return (case.n, case.dim, case.seed, case.T, case.working_set_margin)  # (cases that differ in their cuts only share it)


def scp_of(case, _live=[None, None]):
    """the one-rank SCP object of a case; ONE is alive at a time (with the ranks of a world: at most 8 contexts), None: none"""
    key = scenario_key(case) if case is not None else None
    if _live[0] != key:
        if _live[1] is not None:
            _live[1].close()
        _live[:] = [key, sc.make_scp(case, reuse_native=False) if case is not None else None]
    return _live[1]


def reference(case):
    """the one-rank step of a case from QP#0's solution, computed once: {"acc0", "acc" (numpy), "info"}"""
    key = scenario_key(case)
    if key not in _REF:
        s = scp_of(case)
        s._precompute_constraint_matrices()
        acc0 = s._solve_initial_trajectory()
        new, info = s.scp_iteration(acc0)
        _REF[key] = {"acc0": acc0.cpu().numpy().copy(), "acc": new.cpu().numpy().copy(), "info": info}
        print(f"[{case.name}] reference: status {info['status_val']} rounds {info['rounds']} added {info['added']} "
              f"working_rows {info['working_rows']} unresolved {info['unresolved_rows']} iter {info['iter']}")
    return _REF[key]


def world(case, pos_in):
    key = (case.name, pos_in)
    if key not in _WORLD:
        _WORLD[key] = sc.run_world(scp_of(case), reference(case)["acc0"], case.cuts, pos_in=pos_in)
    return _WORLD[key]


def oracle(case):
    """the linearisation of a case around acc0 by the numpy oracle, computed once"""
    ref = reference(case)
    if "oracle" not in ref:
        p0, pf, space = sc.scenario(case)
        prob = so.make_problem(case.n, case.T, sc.H, sc.R, space, p0, pf)
        assert prob.K == case.K
        pos0, _ = so.kinematics(prob, ref["acc0"])
        eta, l, dist = so.linearize_pairs(prob, pos0)
        ref["oracle"] = (prob, eta, l, dist)
    return ref["oracle"]


def assert_is_reference(got, ref):
    for rank in got["ranks"]:
        np.testing.assert_array_equal(rank["acc"].view(np.int64), ref["acc"].view(np.int64))
        same_records(rank["info"], ref["info"])
        assert rank["info"]["rel_step"] == ref["info"]["rel_step"] and rank["info"]["pipeline"] == ref["info"]["pipeline"]
    for rank in got["ranks"][1:]:
        np.testing.assert_array_equal(rank["acc"].view(np.int64), got["ranks"][0]["acc"].view(np.int64))


def rank_rows(case, r, per_row):
    """the entries of an all-rows array (row k P + q) that belong to rank r's pair range"""
    return per_row.reshape(case.K, case.pairs)[:, case.cuts[r]:case.cuts[r + 1]]


CASE_IDS = [c.name for c in sc.CASES]
ORACLE_CASES = [c for c in sc.CASES if c.n <= sc.ORACLE_MAX_N]


# ---- e. what the cases are there for holds on the reference ------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.CASES, ids=CASE_IDS)
def test_reference_step_is_solved(case):
    info = reference(case)["info"]
    assert info["status_val"] in (1, 2), info
    assert info["rounds"] >= 1 and np.isfinite(reference(case)["acc"]).all()


def test_a_large_case_needs_a_second_round():
    infos = {c.name: reference(c)["info"] for c in sc.CASES if c.n >= 300}
    assert any(i["rounds"] >= 2 and i["added"][0] > 0 for i in infos.values()), \
        {k: (i["rounds"], i["added"]) for k, i in infos.items()}


# ---- a. bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos_in", POS_IN, ids=["acc", "pos_in"])
@pytest.mark.parametrize("case", sc.CASES, ids=CASE_IDS)
def test_world_is_the_one_rank_step(case, pos_in):
    assert_is_reference(world(case, pos_in), reference(case))


# ---- b. the ids of the selection against the oracle --------------------------------------------------------------------------
@pytest.mark.parametrize("pos_in", POS_IN, ids=["acc", "pos_in"])
@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c.name for c in ORACLE_CASES])
def test_selected_ids_are_the_oracles(case, pos_in):
    got = world(case, pos_in)
    prob, eta, l, dist = oracle(case)
    near = dist - prob.R < case.working_set_margin
    seen = []
    for r, rank in enumerate(got["ranks"]):
        ids = rank["begin_ids"]
        assert (np.diff(ids) > 0).all()
        mask = np.zeros((case.K, case.pairs), dtype=bool)
        mask[:, case.cuts[r]:case.cuts[r + 1]] = True
        np.testing.assert_array_equal(ids, np.nonzero(near & mask.ravel())[0])
        seen.append(ids)
    merged = np.concatenate(seen)
    assert np.unique(merged).size == merged.size  # (pairwise disjoint)
    np.testing.assert_array_equal(got["fed"][0], np.nonzero(near)[0])


# ---- c. the last round against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos_in", POS_IN, ids=["acc", "pos_in"])
@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c.name for c in ORACLE_CASES])
def test_last_round_is_the_oracles(case, pos_in):
    got, ref = world(case, pos_in), reference(case)
    prob, eta, l, dist = oracle(case)
    x = got["ranks"][0]["acc"]
    viol = l - so.collision_apply(prob, eta, x.ravel())
    worst = 0.0
    for r, rank in enumerate(got["ranks"]):
        mine = rank_rows(case, r, viol)
        if mine.size == 0:
            assert rank["max_v"][-1] == -np.inf
            continue
        err = abs(rank["max_v"][-1] - mine.max())
        worst = max(worst, err)
        print(f"[{case.name} pos_in={pos_in}] rank {r}: max_v {rank['max_v'][-1]:.6e} oracle {mine.max():.6e} |diff| {err:.2e}")
        assert err < MAX_V_TOL, (r, rank["max_v"][-1], mine.max())
    print(f"[{case.name} pos_in={pos_in}] largest |max_v - oracle| {worst:.2e} (bound {MAX_V_TOL:g})")
    assert got["ranks"][0]["info"]["max_violation"] == max(rank["max_v"][-1] for rank in got["ranks"])
    # the rows the last pass found = the rows the oracle finds violated outside everything that was fed to the QP
    fed = np.concatenate(got["fed"])
    assert np.unique(fed).size == fed.size
    outside = np.ones(viol.size, dtype=bool)
    outside[fed] = False
    want = np.nonzero((viol > scp_of(case).feasibility_tol) & outside)[0]
    last = np.sort(np.concatenate([rank["round_ids"][-1] for rank in got["ranks"]]))
    np.testing.assert_array_equal(last, want)
    assert want.size == ref["info"]["unresolved_rows"]
    assert fed.size == ref["info"]["working_rows"]


# ---- d. the forms really ran -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos_in", POS_IN, ids=["acc", "pos_in"])
@pytest.mark.parametrize("case", sc.CASES, ids=CASE_IDS)
def test_forms_ran(case, pos_in):
    got = world(case, pos_in)
    assert len(got["fed"]) >= 1 and len(got["fed"]) == reference(case)["info"]["rounds"]
    for r, rank in enumerate(got["ranks"]):
        nq = case.cuts[r + 1] - case.cuts[r]
        _, viol_small = sc.pass_forms(case.n, case.K, case.dim, nq)
        print(f"[{case.name} pos_in={pos_in}] rank {r}: {nq} pairs, forms {case.forms[r]}, near passes (ran, fell back) "
              f"{rank['near']}, ids {rank['begin_ids'].size} + {[i.size for i in rank['round_ids']]}")
        assert len(rank["max_v"]) == len(got["fed"])
        if nq > 0 and not viol_small:
            # one near pass per round; the exhaustive pass followed where the near pass found nothing close to active
            assert rank["near"][0] == len(got["fed"]) > 0, (r, rank["near"])
            assert rank["near"][1] == sum(mv < -0.5 * sc.NEAR_TAU for mv in rank["max_v"]), (r, rank["near"], rank["max_v"])
            if r in case.falls_back:  # (far pairs only: in every round)
                assert rank["near"][1] == rank["near"][0]
        else:
            assert rank["near"] == (0, 0), (r, rank["near"])


# ---- further tests on n40_w3 -------------------------------------------------------------------------------------------------
N40 = sc.BY_NAME["n40_w3"]


@pytest.mark.parametrize("pos_in", POS_IN, ids=["acc", "pos_in"])
def test_chain_of_three_steps(pos_in):
    """three consecutive steps on the same rank solvers, each fed the previous output, against the one-rank chain"""
    ref, s = reference(N40), scp_of(N40)
    acc_ref = acc = s._ctx.tensor(ref["acc0"])
    with sc.World(s, N40.cuts) as w:
        for step in range(3):
            new_ref, info_ref = s.scp_iteration(acc_ref)
            got = w.step(acc, pos_in)
            assert_is_reference(got, {"acc": new_ref.cpu().numpy(), "info": info_ref})
            assert not np.array_equal(got["ranks"][0]["acc"], acc.cpu().numpy())  # (the chain moves)
            acc_ref, acc = new_ref, s._ctx.tensor(got["ranks"][-1]["acc"])


def test_short_rows_buffer():
    """a rows buffer of 8 ids: every longer list is fetched again (scp_solver_shard_rows)"""
    ref = reference(N40)
    got = sc.run_world(scp_of(N40), ref["acc0"], N40.cuts, pos_in=False, rows_buffer=8)
    assert max(rank["begin_ids"].size for rank in got["ranks"]) > 8
    assert_is_reference(got, ref)
    default = world(N40, False)
    for a, b in zip(got["ranks"], default["ranks"]):
        np.testing.assert_array_equal(a["begin_ids"], b["begin_ids"])
        assert len(a["round_ids"]) == len(b["round_ids"])
        for x, y in zip(a["round_ids"], b["round_ids"]):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("case", [N40, sc.BY_NAME["n300_w1cut"]], ids=lambda c: c.name)
def test_small_row_capacity(case):
    """a QP workspace of 16 rows on every rank: it grows in the first round (no state yet) and, where a later round adds
    rows, again with the state of the solve in flight (scp_qp_clone_state)"""
    ref = reference(case)
    got = sc.run_world(scp_of(case), ref["acc0"], case.cuts, pos_in=False, row_capacity=16)
    assert ref["info"]["working_rows"] > 16 and got["fed"][0].size > 16
    if case.n >= 300:  # (the first growth leaves a workspace that is exactly full: the second round's rows grow it again)
        assert len(got["fed"]) >= 2 and got["fed"][1].size > 0
    assert_is_reference(got, ref)


def test_one_rank_step_with_a_small_row_capacity():
    """the same growth inside scp_solver_step: the workspace that had to grow in the middle of a solve (scp_qp_clone_state)
    continues the solve of the one that did not, bit for bit"""
    case = sc.BY_NAME["n300_w1cut"]
    ref = reference(case)
    s = sc.make_scp(case, qp_row_capacity=16, reuse_native=False)
    try:
        new, info = s.scp_iteration(ref["acc0"])
        assert info["rounds"] >= 2 and info["added"][0] > 0 and info["working_rows"] > 16
        np.testing.assert_array_equal(new.cpu().numpy().view(np.int64), ref["acc"].view(np.int64))
        same_records(info, ref["info"])
        assert info["rel_step"] == ref["info"]["rel_step"] and info["pipeline"] == ref["info"]["pipeline"]
    finally:
        s.close()


def test_phases_need_a_begin():
    import torch
    from path_planning import _hip

    ref = reference(N40)
    with sc.World(scp_of(N40), N40.cuts[:2]) as w:
        nat, rec = w.solvers[0], _hip.QpRecord()
        rows = torch.zeros(1, dtype=torch.int64, device=w.ctxs[0].tdev)
        for call in (lambda: nat.shard_qp(rows, rec), nat.shard_violations, lambda: nat.shard_round_done(0, 0.0, rec),
                     lambda: nat.shard_end(rec)):
            with pytest.raises(_hip.HipError):
                call()
        # a complete step brings the solver back to that state
        w.step(ref["acc0"], False)
        with pytest.raises(_hip.HipError):
            nat.shard_end(rec)


def test_bad_begins_raise():
    from path_planning import _hip

    ref = reference(N40)
    s, P = scp_of(N40), N40.pairs
    acc0 = s._ctx.tensor(ref["acc0"])
    with sc.World(s, N40.cuts) as w:
        for q_range in ((0, P + 1), (5, 4), (-1, 3)):
            with pytest.raises(_hip.HipError):
                w.begin(0, acc0, False, q_range=q_range)
        opts = s._native_options()
        opts.row_free = 0
        with pytest.raises(_hip.HipError):
            w.begin(0, acc0, False, opts=opts)
        with pytest.raises(_hip.HipError):  # (none of them began a step)
            w.solvers[0].shard_violations()
        assert_is_reference(w.step(ref["acc0"], False), ref)


@pytest.mark.parametrize("abandon_after", ["begin", "qp", "violations"])
def test_abandoned_step_leaves_nothing_behind(abandon_after):
    """a step given up between two phases (the per-round iteration budget is in the solver's settings by then), then a
    complete sharded step and a plain scp_solver_step on the same rank solvers: both are the reference"""
    ref, s = reference(N40), scp_of(N40)
    acc0 = s._ctx.tensor(ref["acc0"])
    other = s._ctx.tensor(0.5 * ref["acc"])  # (another linearisation point: its selection must not survive either)
    with sc.World(s, N40.cuts) as w:
        recs, ids = zip(*[w.begin(r, other, True) for r in range(w.world)])
        if abandon_after != "begin":
            rows = w.gather(list(ids))
            for r in range(w.world):
                w.solvers[r].shard_qp(rows, recs[r])
            if abandon_after == "violations":
                for r in range(w.world):
                    w.solvers[r].shard_violations()
        assert_is_reference(w.step(ref["acc0"], False), ref)
        p0, v0, pf, vf = s._states()
        for nat in w.solvers:
            new, rec = nat.step(s._limits(), s._space(), p0, v0, pf, vf, s._native_options(), acc0)
            np.testing.assert_array_equal(new.cpu().numpy().view(np.int64), ref["acc"].view(np.int64))
            same_records(sc.record_dict(rec), ref["info"])
            assert float(rec.rel_step) == ref["info"]["rel_step"]


@pytest.mark.parametrize("case", [N40, sc.BY_NAME["n3_w5"], sc.BY_NAME["n300_w1cut"]], ids=lambda c: c.name)
def test_rank_order_within_a_phase_does_not_matter(case):
    ref = reference(case)
    got = sc.run_world(scp_of(case), ref["acc0"], case.cuts, pos_in=True, reverse=True)
    assert_is_reference(got, ref)
    forward = world(case, True)
    for a, b in zip(got["ranks"], forward["ranks"]):
        np.testing.assert_array_equal(a["begin_ids"], b["begin_ids"])
        assert a["max_v"] == b["max_v"] and a["near"] == b["near"]
