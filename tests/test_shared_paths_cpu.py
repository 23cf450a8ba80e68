"""Shared paths without a GPU: the premises of the cases of tests/shared_path_cases.py, the definitions of
tests/shared_path_ref.py checked independently of its own code path, the two limits (no rounds, no share weight), the ABI rows,
the planner's surface and the CLI parser."""
import inspect
import os
import re

import numpy as np
import pytest

import shared_path_cases as sc
import shared_path_ref as sp
import weighted_path_ref as wr

import ctx_state_cases as cs
import shared_path_ctx_case as scc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c.name: c for c in sc.all_cases()}
CTX_CASE = scc.register()  # (the table of tests/ctx_state_cases.py gains the case of the three new entry points)


def test_the_context_state_case():
    """what tests/test_ctx_state_cpu.py asks of every case of its table: the entry points are covered, the reference satisfies
    the case's own criterion and is deterministic, and the family's grower leaves the shared workspace larger than the case
    needs"""
    from path_planning import _hip

    assert cs.CASES_BY_NAME[scc.NAME] is CTX_CASE and CTX_CASE in cs.CASES and CTX_CASE.family in cs.POISON_BETWEEN_CALLS
    covered = {e for c in cs.CASES for e in c.entries}
    assert set(scc.SHARED_ENTRIES) <= covered <= set(_hip.PROTOTYPES) and not set(scc.SHARED_ENTRIES) & set(cs.EXEMPT)
    inp, ref = CTX_CASE.inputs(), CTX_CASE.ref()
    out = CTX_CASE.from_ref(ref, inp)
    CTX_CASE.compare(out, ref, inp)
    cs.assert_no_canary(out)
    cs.assert_same_bits(CTX_CASE.from_ref(CTX_CASE.reference(inp), inp), out, scc.NAME)
    grown = cs.GROWERS[CTX_CASE.family].ws()
    (low, high), = CTX_CASE.ws().values()
    assert 0 < low <= high < grown["sep_ws"][0]


def test_premises():
    """what the cases are there for holds on the restatement: the negotiation lowers the overuse in the door cases, the best
    round is neither the first nor the last somewhere, with one group the fleet swings and round 0 stays the best, the clamp is
    reached, a re-routed vehicle keeps its path, and every status and a start on its goal are in the fleet"""
    for name in sc.DOOR_CASES:
        w = CASES[name].want()
        assert w["overuse"][w["best_round"]] < w["overuse"][0], name
        assert w["overuse"][w["best_round"]] == min(w["overuse"]) and w["overuse"].index(min(w["overuse"])) == w["best_round"]
    assert CASES["two_doors"].want()["overuse"][0] == 60 and CASES["two_doors"].want()["overuse"][-1] == 19
    inside = [n for n, c in CASES.items() if 0 < c.want()["best_round"] < c.rounds]
    assert {"wide_doors", "groups_3", "slab_3d"} <= set(inside), inside
    g1 = CASES["groups_1"]
    assert g1.groups == 1 and g1.want()["best_round"] == 0 and g1.want()["overuse"] == [12, 24, 14, 22, 14]
    assert CASES["groups_3"].N % CASES["groups_3"].groups != 0
    assert CASES["large"].nodes > 8192 and CASES["stride_2"].stride == 2 and CASES["slab_3d"].D == 3
    # the clamp: some vehicle's unclamped penalty exceeds the limit at some node of some round
    c = CASES["clamp"]
    w, pen = c.want(), c.map()["pen"]
    reached = 0
    for r, load in enumerate(w["loads"]):
        for i in range(r % c.groups, c.N, c.groups):
            own = set(sp.nodes_of(w["sets"][r][1], w["sets"][r][2], i))
            raw = [int(pen[u]) + c.share_weight * max(0, int(load[u]) - (u in own) + 1 - c.capacity) for u in range(c.nodes)]
            got = sp.shared_penalty(pen, load, own, c.share_weight, c.capacity)
            reached += sum(v > sp.MAX_PRODUCT for v in raw)
            assert [min(v, sp.MAX_PRODUCT) for v in raw] == got.tolist()
    assert reached > 0 and pen.any()
    k = CASES["short_max_path"].want()
    assert k["n_kept"] > 0 and k["n_failed"] == 0 and k["overuse"][k["best_round"]] < k["overuse"][0]
    st = CASES["statuses"].want()
    assert st["info"]["status"].tolist() == [0, 1, 0, 2, 0, 3, 0, 0] and st["n_failed"] == 3
    assert st["info"]["start_node"][6] == st["info"]["goal_node"][6] and st["info"]["n_nodes"][6] == 1
    assert {c.weight is None for c in CASES.values()} == {True, False}  # pen both NULL and made from the distance field


@pytest.mark.parametrize("name", ["two_doors", "wide_doors", "statuses", "slab_3d"])
def test_definitions_independently(name):
    """the load by np.bincount, the overuse from it, pen_i by a per-node loop, one field by dense Bellman-Ford rounds, and
    what a re-routing must leave alone"""
    c = CASES[name]
    w, m = c.want(), c.map()
    for r, (_, path, info, _) in enumerate(w["sets"]):
        used = np.concatenate([path[i, :info["n_nodes"][i]] for i in range(c.N) if info["status"][i] == 0])
        load = np.bincount(used, minlength=c.nodes)
        got, over = sp.path_load(path, info, c.nodes, c.capacity)
        np.testing.assert_array_equal(got, load)
        assert over == int(np.maximum(load - c.capacity, 0).sum()) == w["overuse"][r]
        for i in range(c.N):  # no path visits a node twice; the rows end in -1
            n = info["n_nodes"][i]
            assert len(set(path[i, :n].tolist())) == n and (path[i, n:] == -1).all()
    r = 0
    load, (_, path, info, _) = w["loads"][r], w["sets"][r]
    i = next(i for i in range(r % c.groups, c.N, c.groups) if info["status"][i] == 0)
    own = sp.nodes_of(path, info, i)
    pen_i = np.empty(c.nodes, dtype=np.int64)
    for u in range(c.nodes):
        others = sum(u in sp.nodes_of(path, info, j) for j in range(c.N) if j != i)
        base = 0 if m["pen"] is None else int(m["pen"][u])
        pen_i[u] = min(base + c.share_weight * max(0, others + 1 - c.capacity), 32768)
    np.testing.assert_array_equal(sp.shared_penalty(m["pen"], load, own, c.share_weight, c.capacity), pen_i)
    field = wr.bellman_ford(c.L, m["edges"], pen_i.astype(np.uint32), int(info["goal_node"][i]))
    np.testing.assert_array_equal(w["costs"][r][i], field)
    after = w["sets"][r + 1]
    if after[2]["n_nodes"][i] and w["n_kept"] == 0:
        assert after[3][i] == field[info["start_node"][i]]
    for j in range(c.N):  # an inactive or skipped vehicle: all four outputs and its row of cost_out untouched
        if j % c.groups != r % c.groups or info["status"][j] != 0:
            assert all(a[j].tobytes() == b[j].tobytes() for a, b in zip(w["sets"][r], after))
            assert (w["costs"][r][j] == sc.COST_SENTINEL).all()


def test_kept_vehicles_keep_everything():
    c = CASES["short_max_path"]
    w = c.want()
    kept = 0
    for r in range(c.rounds):
        before, after = w["sets"][r], w["sets"][r + 1]
        for i in range(r % c.groups, c.N, c.groups):
            field = w["costs"][r][i]
            same = all(a[i].tobytes() == b[i].tobytes() for a, b in zip(before, after))
            walked = wr.walk(c.L, c.map()["edges"], sp.shared_penalty(c.map()["pen"], w["loads"][r], sp.nodes_of(before[1], before[2], i),
                                                                      c.share_weight, c.capacity),
                             field, int(before[2]["start_node"][i]), int(before[2]["goal_node"][i]), c.nodes)
            if len(walked) > c.max_path:
                kept += 1
                assert same and (field != sc.COST_SENTINEL).any()
            else:
                assert after[1][i, :len(walked)].tolist() == walked
    assert kept == w["n_kept"] > 0


@pytest.mark.parametrize("name", ["wide_doors", "statuses", "slab_3d"])
def test_no_rounds_and_no_share_weight(name):
    """rounds = 0 is the weighted search exactly; with share_weight = 0 every round reproduces round 0"""
    c = CASES[name]
    m = c.map()
    plain = wr.reference_paths_weighted(c.D, c.origin, c.cell, m["sat"], c.stride, m["edges"], m["pen"], c.p0, c.pf, c.K, c.max_path,
                                        c.ref_in())
    none = c.negotiate(rounds=0)
    for got, want in zip((none["ref"], none["path"], none["info"], none["path_cost"]), plain[:4]):
        assert got.tobytes() == want.tobytes()
    assert none["n_failed"] == plain[5] and none["best_round"] == 0 and none["n_kept"] == 0 and len(none["overuse"]) == 1
    free = c.negotiate(share_weight=0)
    assert free["best_round"] == 0 and len(set(free["overuse"])) == 1 and len(free["sets"]) == c.rounds + 1
    for s in free["sets"]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(s, plain[:4]))


def test_the_abi_rows():
    from path_planning import _hip

    header = open(os.path.join(ROOT, "include", "scp_hip.h")).read()
    assert _hip.ABI_VERSION == 7 == int(re.search(r"#define SCP_ABI_VERSION (\d+)", header).group(1))
    assert int(re.search(r"#define SCP_NEGOTIATE_MAX_ROUNDS (\d+)", header).group(1)) == _hip.NEGOTIATE_MAX_ROUNDS == sp.MAX_ROUNDS
    lib = _hip.load_library()
    for name, arity in (("scp_path_load", 9), ("scp_reference_paths_shared", 22), ("scp_negotiate_paths", 23)):
        assert name in _hip.EXPORTS and len(_hip.PROTOTYPES[name][1]) == arity and hasattr(lib, name)
        assert re.search(rf"^int {name}\(scp_ctx\* ctx,", header, flags=re.M), name
    for name in ("path_load", "reference_paths_shared", "negotiate_paths"):
        assert callable(getattr(_hip.Context, name))
    sig = inspect.signature(_hip.Context.negotiate_paths).parameters
    assert [sig[k].default for k in ("capacity", "groups", "rounds", "pen", "want_path")] == [1, 1, 0, None, True]


def test_the_python_surface():
    from path_planning.solvers._obstacles import path_sharing
    from path_planning.solvers.scp import SCP

    sig = inspect.signature(SCP.set_path_sharing).parameters
    assert [(k, p.default) for k, p in sig.items()][1:] == [("share", 0.0), ("capacity", 1), ("groups", 4), ("rounds", None)]
    assert SCP._sharing is None
    assert path_sharing(0.0, 1, 4, None) is None and path_sharing(0, 3, 2, 5) is None
    assert path_sharing(1.0, 1, 4, None) == (70, 1, 4, None) and path_sharing(0.5, 2, 3, 0) == (35, 2, 3, 0)
    assert path_sharing(32768 / 70, 1, 1, 64) == (32768, 1, 1, 64)
    for bad in ((-0.1, 1, 4, None), (float("nan"), 1, 4, None), (float("inf"), 1, 4, None), (469.0, 1, 4, None), ("1", 1, 4, None),
                (True, 1, 4, None), (1.0, 0, 4, None), (1.0, 1.0, 4, None), (1.0, 1, 0, None), (1.0, 1, True, None),
                (1.0, 1, 4, -1), (1.0, 1, 4, 65), (1.0, 1, 4, 2.0)):
        with pytest.raises(ValueError):
            path_sharing(*bad)

    class Ranks:
        def __init__(self, world):
            self.world = world

    s = SCP.__new__(SCP)
    s.shard, s.N, s.D = Ranks(2), 3, 2
    with pytest.raises(ValueError, match="one rank"):
        s.set_path_sharing(share=1.0)
    s.shard = Ranks(1)
    s.set_path_sharing(share=2.0, capacity=2, groups=3)
    assert s._sharing == (140, 2, 3, None)
    # with sharing on and the search by hops, the searches refuse and name the setting that is missing
    for call in (s.find_reference, s.shorten_reference, lambda: s.set_corridors(reference="search"),
                 lambda: s.set_corridors(reference="shortened")):
        with pytest.raises(ValueError, match=r'set_search_metric\("length"\)'):
            call()
    s.set_space_dims([0.0, 0.0, 1.0, 1.0])
    assert s._sharing is None and s._metric == ("hops", 0, 0)
    s.set_path_sharing(share=1.0)
    s.set_path_sharing()
    assert s._sharing is None
    # the signatures other tests pin stay as they are
    pinned = {"set_search_metric": ["metric", "keep_clear", "clear_weight"],
              "find_reference": ["stride", "clearance", "max_path", "allow_unreachable"],
              "shorten_reference": ["stride", "clearance", "max_path", "allow_unreachable"],
              "set_corridors": ["reference", "max_grow", "pad", "allow_open"]}
    for name, names in pinned.items():
        assert list(inspect.signature(getattr(SCP, name)).parameters)[1:] == names, name


def test_the_cli_parser():
    from path_planning.cli import compute_trajectories as ct

    parser = ct.build_parser()
    base = ["--obstacle-discs", "5,5,1", "--corridor-search", "--corridor-metric", "length"]
    args = parser.parse_args(base + ["--corridor-share", "1.5", "--corridor-share-capacity", "2", "--corridor-share-groups", "3",
                                     "--corridor-share-rounds", "5"])
    assert (args.corridor_share, args.corridor_share_capacity, args.corridor_share_groups, args.corridor_share_rounds) == (1.5, 2, 3, 5)
    assert ct.obstacle_discs(parser, args) == [(5.0, 5.0, 1.0)]
    none = parser.parse_args([])
    assert [getattr(none, "corridor_share" + k) for k in ("", "_capacity", "_groups", "_rounds")] == [None] * 4
    for argv in (["--corridor-share", "1"], ["--obstacle-discs", "5,5,1", "--corridor-share", "1"],
                 ["--obstacle-discs", "5,5,1", "--corridor-search", "--corridor-share", "1"],
                 ["--obstacle-discs", "5,5,1", "--corridor-search", "--corridor-metric", "hops", "--corridor-share", "1"],
                 ["--obstacle-discs", "5,5,1", "--corridor-metric", "length", "--corridor-share", "1"],
                 base + ["--corridor-share-capacity", "2"], base + ["--corridor-share-groups", "2"],
                 base + ["--corridor-share-rounds", "2"]):
        with pytest.raises(SystemExit):
            ct.obstacle_discs(parser, parser.parse_args(argv))
    fr = {"sharing": {"overuse": [60, 46, 35], "best_round": 2, "rounds": 2}}
    assert ct.shared_summary(fr) == ", overuse 60 -> 35 (round 2 of 2)" and ct.shared_summary({}) == ""
