"""CPU checks behind tests/test_shard_world_gpu.py: the cuts of every case of tests/shard_cases.py are a partition of the pair
range, pass_forms (small_pass_ok restated) puts every rank and the one-rank step into the form the table claims, the even
split tiles the range at every world size, and every scenario is reachable within its horizon."""
import numpy as np
import pytest

import shard_cases as sc

VEL_MAX = 2.0  # scp.py:67-68


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_cuts_partition_the_pair_range(case):
    cuts = list(case.cuts)
    assert cuts[0] == 0 and cuts[-1] == case.pairs
    assert all(a <= b for a, b in zip(cuts[:-1], cuts[1:]))
    assert 1 <= case.world <= sc.World.MAX_RANKS and len(case.forms) == case.world


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_forms_are_the_table(case):
    got = tuple(sc.form_name(case.n, case.K, case.dim, b - a) for a, b in zip(case.cuts[:-1], case.cuts[1:]))
    assert got == case.forms
    assert sc.form_name(case.n, case.K, case.dim, case.pairs) == case.ref_forms


def test_table_reaches_what_it_is_there_for():
    forms = {c.name: c.forms for c in sc.CASES}
    assert forms["n300_w1cut"] == ("LL", "SS") and forms["n300_w2"] == ("SS", "SS")
    assert forms["n1100_mixed"] == ("SL", "LL", "SL")
    assert forms["n3_w5"].count("--") == 2 and list(sc.BY_NAME["n3_w5"].cuts) == [0, 0, 1, 1, 2, 3]
    assert all(sc.BY_NAME[n].ref_forms == "LL" for n in ("n300_w1cut", "n300_w2", "n1100_mixed"))
    assert {c.K for c in sc.CASES} == {50, 10} and {c.dim for c in sc.CASES} == {2, 3}
    # rank 1 of n1100_mixed: its map is beyond what one workgroup compacts (the three-launch compaction)
    c = sc.BY_NAME["n1100_mixed"]
    assert (c.K * (c.cuts[2] - c.cuts[1]) + 31) // 32 > sc.SMALL_MAX_WORDS
    # one-pair shards next to the boundaries of the triangle's rows
    c = sc.BY_NAME["n40_inside_rows"]
    sizes = [b - a for a, b in zip(c.cuts[:-1], c.cuts[1:])]
    assert sizes.count(1) == 3 and {39, 77} <= set(c.cuts)  # (pairs (0, 39) | (1, 2) and (1, 39) | (2, 3))


def test_pass_forms_at_its_thresholds():
    # 2 M rows: the bitmap of one workgroup
    assert sc.pass_forms(300, 50, 2, 41943) == (True, True)  # 2 097 150 rows
    assert sc.pass_forms(300, 50, 2, 41944) == (False, False)  # 2 097 200 rows = 65 537 words
    # 32 KiB of slices
    assert sc.pass_forms(1024, 50, 2, 1000) == (True, True)  # 2 x 16 KiB
    assert sc.pass_forms(1025, 50, 2, 1000) == (True, False)
    assert sc.pass_forms(2048, 3, 2, 1000) == (True, False) and sc.pass_forms(2049, 3, 2, 1000) == (False, False)
    # 2048 workgroups of 2048 rows (nq + 1 rows per time step: the pass's lane pairs)
    assert sc.pass_forms(100, 2048, 2, 1000) == (True, True) and sc.pass_forms(100, 2049, 2, 10) == (False, False)
    assert sc.pass_forms(100, 1024, 2, 2047) == (True, True)  # one workgroup per time step: 2047 + 1 rows
    assert sc.pass_forms(100, 500, 2, 4095) == (True, True) and sc.pass_forms(100, 683, 2, 3000) == (True, True)
    assert sc.pass_forms(100, 700, 2, 2995) == (True, True) and sc.pass_forms(100, 1025, 2, 2045) == (True, True)
    assert sc.pass_forms(40, 50, 2, 0) == (False, False)


@pytest.mark.parametrize("n", [3, 40])
def test_even_split_tiles_at_every_world_size(n):
    pairs = sc.pairs_of(n)
    for world in range(1, pairs + 4):
        cuts = sc.even_cuts(n, world)
        assert len(cuts) == world + 1 and cuts[0] == 0 and cuts[-1] == pairs
        sizes = np.diff(cuts)
        assert (sizes >= 0).all() and sizes.max() - sizes.min() <= 1
    assert sc.even_cuts(3, 5) == [0, 0, 1, 1, 2, 3]


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_scenarios_are_reachable(case):
    p0, pf, space = sc.scenario(case)
    assert p0.shape == pf.shape == (case.n, case.dim) and len(space) == 2 * case.dim
    trip = float(np.sqrt(((pf - p0) ** 2).sum(axis=1)).max())
    assert 2.0 * trip <= VEL_MAX * case.T, trip


@pytest.mark.parametrize("case", [c for c in sc.CASES if c.falls_back], ids=lambda c: c.name)
def test_far_ranks_hold_far_pairs_only(case):
    """a rank that is to fall back: its vehicles start and end further apart than R plus the two longest trips"""
    from oracle import scp_oracle as so

    p0, pf, _ = sc.scenario(case)
    trip = float(np.sqrt(((pf - p0) ** 2).sum(axis=1)).max())
    iu, ju = so.pair_index(case.n)
    for r in case.falls_back:
        assert case.forms[r][1] == "L"  # (only the multi-launch violations pass has the near form)
        i, j = iu[case.cuts[r]:case.cuts[r + 1]], ju[case.cuts[r]:case.cuts[r + 1]]
        for p in (p0, pf):
            assert float(np.sqrt(((p[i] - p[j]) ** 2).sum(axis=1)).min()) > sc.R + 2.0 * trip + 1.0
